// lookback.hpp -- decoupled look-back over per-tile descriptors in HBM: [status : value] in one 64-bit word, status 1 =
// the tile's own aggregate, 2 = inclusive prefix.  Shared by the regroup kernel (sa_regroup.hip) and the sub-bucket
// sort that does the regroup of round 0 on the way (local_sort.hpp: local_sort_kernel).
#pragma once
#include "common.hpp"

namespace nolzss {

constexpr uint32_t kSpinLimit = 1u << 24;  // look-back polls before the kernel gives up (sets err)

__device__ __forceinline__ uint64_t desc_load(const uint64_t *p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void desc_store(uint64_t *p, uint64_t v) {
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Run by the first wavefront of a workgroup: publishes the tile's aggregate, combines the
// descriptors of the tiles in front (64 per step, nearest first) up to the first inclusive one,
// publishes the tile's inclusive prefix and returns its exclusive prefix.
template <typename Op>
__device__ __forceinline__ uint32_t lookback_exclusive(uint64_t *desc, uint32_t tile, uint32_t aggregate, Op op,
                                                       uint32_t *err) {
    const int lane = lane_id();
    if (tile == 0) {
        if (lane == 0) desc_store(desc, (2ull << 32) | aggregate);
        return Op::identity();
    }
    if (lane == 0) desc_store(desc + tile, (1ull << 32) | aggregate);
    uint32_t excl = Op::identity();
    int64_t look = (int64_t)tile - 1;
    for (;;) {
        const int64_t idx = look - lane;
        uint64_t d, need, inc;
        uint32_t spins = 0;
        for (;;) {
            d = idx >= 0 ? desc_load(desc + idx) : (2ull << 32);  // in front of tile 0: inclusive identity
            const uint32_t st = (uint32_t)(d >> 32);
            inc = __ballot(st == 2);
            // every lane up to and including the first inclusive one must have been published
            need = inc ? (((inc & (~inc + 1ull)) << 1) - 1ull) : ~0ull;
            const uint64_t missing = __ballot(st == 0) & need;
            if (!missing) break;
            if (++spins > kSpinLimit) {  // cannot happen with ticket order; never hang the GPU
                if (lane == 0) atomicExch(err, 1u);
                return excl;
            }
            __builtin_amdgcn_s_sleep(1);
        }
        const uint32_t v = ((need >> lane) & 1ull) ? (uint32_t)d : Op::identity();
        excl = op(excl, wave_reduce(v, op));
        if (inc) break;  // an inclusive prefix was reached
        look -= 64;
    }
    if (lane == 0) desc_store(desc + tile, (2ull << 32) | op(excl, aggregate));
    return excl;
}

// The same for sums with kWin windows of 64 descriptors per round trip, nearest first: a walk that goes back over a few
// hundred tiles in flight (one workgroup per CU, every one of them a predecessor) takes one trip instead of four.
// (spin_limit: polls before it gives up and sets err -- a caller whose tiles are NOT dealt out in start order passes a small
// one: a tile in front may belong to a workgroup that is not resident yet, and the walk then has to end in a fallback)
//
// In two halves, for a caller that can put other work between them (local_sort_kernel walks a whole turn after it has
// published: every aggregate the walk needs is a turn old by then).  Both are run by one wavefront.
// The first half: the tile's own aggregate (tile 0 has nothing in front: its aggregate is its inclusive prefix).
__device__ __forceinline__ void lookback_publish_add(uint64_t *desc, uint32_t tile, uint32_t aggregate) {
    if (lane_id() == 0) desc_store(desc + tile, ((tile == 0 ? 2ull : 1ull) << 32) | aggregate);
}

// The second half: sums the descriptors in front back to the first inclusive prefix, publishes the tile's inclusive prefix
// and returns its exclusive one.  `aggregate` is what lookback_publish_add was given for the tile.
// `pre` (optional): what lookback_walk_preload read for this tile, taken for the first round trip.
template <int kWin>
__device__ __forceinline__ uint32_t lookback_walk_add_wide(uint64_t *desc, uint32_t tile, uint32_t aggregate, uint32_t *err,
                                                           uint32_t spin_limit = kSpinLimit, bool *gave_up = nullptr,
                                                           const uint64_t *pre = nullptr) {
    const int lane = lane_id();
    if (tile == 0) return 0u;
    uint32_t part = 0, spins = 0;  // (part: this lane's share of the sum -- ONE reduction over the wave, at the end)
    int64_t look = (int64_t)tile - 1;
    for (bool first = pre != nullptr;; first = false) {
        uint64_t d[kWin];
#pragma unroll
        for (int j = 0; j < kWin; ++j) {
            const int64_t idx = look - 64 * j - lane;
            d[j] = idx >= 0 ? (first ? pre[j] : desc_load(desc + idx)) : (2ull << 32);  // in front of tile 0: inclusive identity
        }
        bool done = false, stalled = false;
#pragma unroll
        for (int j = 0; j < kWin; ++j) {
            if (done || stalled) continue;  // (wave-uniform)
            const uint32_t st = (uint32_t)(d[j] >> 32);
            const uint64_t inc = __ballot(st == 2);
            // every lane up to and including the first inclusive one must have been published
            const uint64_t need = inc ? (((inc & (~inc + 1ull)) << 1) - 1ull) : ~0ull;
            const uint64_t missing = __ballot(st == 0) & need;
            if (missing) {  // not published yet: wait and read again from this window on
                stalled = true;
                continue;
            }
            part += ((need >> lane) & 1ull) ? (uint32_t)d[j] : 0u;
            look -= 64;
            if (inc) done = true;  // an inclusive prefix was reached
        }
        if (done) break;
        if (stalled) {
            if (++spins > spin_limit) {  // (never hang the GPU)
                if (lane == 0) atomicExch(err, 1u);
                if (gave_up) *gave_up = true;
                return wave_reduce(part, OpAdd<uint32_t>());
            }
            __builtin_amdgcn_s_sleep(1);
        }
    }
    const uint32_t excl = wave_reduce(part, OpAdd<uint32_t>());
    if (lane == 0) desc_store(desc + tile, (2ull << 32) | (uint64_t)(excl + aggregate));
    return excl;
}

// The first round trip of a walk asked for AHEAD of it: the kWin windows in front of `tile` into pre[], for
// lookback_walk_add_wide to take when the answers have long arrived -- a walk is a dependent read through the fabric, 2 - 3 us
// under load, and it waits behind every store its wave has issued before.  Buffer loads, served past the L2 like the
// agent-scope loads of desc_load; a lane without work (on = false, or in front of tile 0) is sent out of bounds and gets 0
// without a memory access: no branch around a load, the compiler can count what is in flight.  bytes: the size of desc[].
__device__ __forceinline__ uint64_t desc_load_buf(__amdgpu_buffer_rsrc_t rsrc, bool on, int64_t idx) {
    typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
    const u32x2 v = __builtin_amdgcn_raw_buffer_load_b64(rsrc, (on && idx >= 0) ? (uint32_t)idx * 8u : 0xfffffff0u, 0, 16 /* sc1 */);
    return ((uint64_t)v.y << 32) | (uint64_t)v.x;
}
template <int kWin>
__device__ __forceinline__ void lookback_walk_preload(uint64_t *desc, uint32_t bytes, uint32_t tile, bool on, uint64_t *pre) {
    const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(desc, 0, (int)bytes, 0x00020000);
    const int64_t look = (int64_t)tile - 1;
#pragma unroll
    for (int j = 0; j < kWin; ++j) pre[j] = desc_load_buf(rsrc, on, look - 64 * j - lane_id());
}

// ... and both at once, for a caller with nothing to put between them
template <int kWin>
__device__ __forceinline__ uint32_t lookback_exclusive_add_wide(uint64_t *desc, uint32_t tile, uint32_t aggregate, uint32_t *err,
                                                                uint32_t spin_limit = kSpinLimit, bool *gave_up = nullptr) {
    lookback_publish_add(desc, tile, aggregate);
    return lookback_walk_add_wide<kWin>(desc, tile, aggregate, err, spin_limit, gave_up);
}

}  // namespace nolzss
