// device_buf.hpp -- the owner of the device memory of every resident handle (part of the C ABI layer; DESIGN.md 5,
// "Relative-LZ handles: who owns device memory").  A DeviceBuf is one device_alloc allocation -- not arena memory, which
// the next call on the device recycles -- with the bytes asked for and its device.  It moves, never copies; a
// zero-filled object is an empty buffer whose destructor does nothing.
#pragma once
#include <atomic>
#include <utility>

#include "pipeline.hpp"

namespace nolzss {
namespace api {

// hipMalloc with one retry after trimming the idle arenas (c_abi.hip).  DeviceBuf::alloc is its only caller.
void *device_alloc(Context &ctx, size_t bytes);

// every DeviceBuf of the process that holds memory, and their bytes (nolzss_debug_device_buffers): changed in alloc and
// reset only
inline std::atomic<size_t> g_device_buffers{0}, g_device_buffer_bytes{0};

class DeviceBuf {
    void *p_ = nullptr;
    size_t bytes_ = 0;
    int device_ = 0;

public:
    DeviceBuf() = default;
    DeviceBuf(DeviceBuf &&o) noexcept { swap(o); }
    DeviceBuf &operator=(DeviceBuf &&o) noexcept {
        DeviceBuf taken(std::move(o));
        swap(taken);  // (what this held goes with `taken`)
        return *this;
    }
    DeviceBuf(const DeviceBuf &) = delete;
    DeviceBuf &operator=(const DeviceBuf &) = delete;
    ~DeviceBuf() { reset(); }

    void swap(DeviceBuf &o) noexcept {
        std::swap(p_, o.p_);
        std::swap(bytes_, o.bytes_);
        std::swap(device_, o.device_);
    }
    // `bytes` on the device of ctx, which a Session has made current; what the buffer held before is freed first.
    // Zero bytes leave it empty.
    void alloc(Context &ctx, size_t bytes) {
        reset();
        p_ = device_alloc(ctx, bytes);
        if (!p_) return;
        bytes_ = bytes;
        device_ = ctx.device;
        g_device_buffers += 1;
        g_device_buffer_bytes += bytes;
    }
    // Frees on the buffer's device and leaves the calling thread's current device what it was; errors are ignored.
    void reset() noexcept {
        if (!p_) return;
        int current = -1;
        const bool known = hipGetDevice(&current) == hipSuccess;
        (void)hipSetDevice(device_);
        (void)hipFree(p_);
        if (known && current != device_) (void)hipSetDevice(current);
        g_device_buffers -= 1;
        g_device_buffer_bytes -= bytes_;
        p_ = nullptr;
        bytes_ = 0;
    }
    // A new allocation of new_bytes with the first keep_bytes copied over on ctx.stream and waited for (no copy and no
    // wait for keep_bytes = 0), then the old one freed.  A throw frees the new one and leaves the buffer as it was.
    void grow_keeping(Context &ctx, size_t new_bytes, size_t keep_bytes) {
        DeviceBuf fresh;
        fresh.alloc(ctx, new_bytes);
        if (keep_bytes) {
            HIP_CHECK(hipMemcpyAsync(fresh.p_, p_, keep_bytes, hipMemcpyDeviceToDevice, ctx.stream));
            HIP_CHECK(hipStreamSynchronize(ctx.stream));
        }
        swap(fresh);
    }

    template <class T> T *as() const { return static_cast<T *>(p_); }
    void *get() const { return p_; }
    size_t bytes() const { return bytes_; }
    explicit operator bool() const { return p_ != nullptr; }
};

}  // namespace api
}  // namespace nolzss
