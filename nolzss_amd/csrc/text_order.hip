// text_order.hip -- the permutation into text order (text_order.hpp): out[idx[k]] = val[k] for pairs in list order.
// Not a sort, but built on the partition pass of one (radix_pass.hpp):
//   * the scatter kernels: plain_*_scatter_kernel (small inputs and what is left of a partial scatter),
//     window_scatter*_kernel and record_window_scatter*_kernel (a window of the target assembled in LDS and written
//     out as full lines), separator_scatter_kernel;
//   * lb_partition_kernel and packed_text_order: the two-value permutation of up to 2^30 targets without histograms;
//   * the host side: record_scatter_plan, bucketed_scatter -- a chooser over one function per form -- and
//     permute_packed.
// Its sources (RankSrc, PairSrc, LocalIdxSrc, LocalRankSrc) are instantiated here only (radix_pass_low16: radix_sort.hip).
#include "text_order.hpp"

#include "lookback.hpp"
#include "radix_pass.hpp"

#include <algorithm>
#include <cstdio>

namespace nolzss {
namespace {

// (target position, value) pairs in list order that carry a SECOND value: the list position itself + 1 (the rank
// of the suffix in the pipeline's 1-based convention).  The two values travel as ONE 64-bit value (first value in
// the low half): two output streams per pass, the value stream in runs of a full 128-byte line, where three
// streams of 4-byte values ran at 2.8 TB/s.  The permutation that brings the factor-length codes into text order
// delivers the inverse suffix array on the way (bucketed_scatter with out2).
struct RankSrc {
    using Raw = uint32_t;
    static constexpr bool kFromText = false;
    const uint32_t *__restrict__ keys;
    const uint32_t *__restrict__ vals;
    __device__ __forceinline__ Raw load(size_t idx, const TileExtent &) const { return keys[idx]; }
    __device__ __forceinline__ uint32_t key_of(Raw raw, size_t, const TileExtent &) const { return raw; }
    __device__ __forceinline__ uint32_t hist_digit_of(Raw raw, size_t, int shift, const TileExtent &) const { return digit_of(raw, shift); }
    __device__ __forceinline__ uint64_t val(size_t idx) const { return (uint64_t)vals[idx] | ((uint64_t)((uint32_t)idx + 1u) << 32); }
    __device__ __forceinline__ bool digits_from_window(int) const { return false; }
    __device__ __forceinline__ uint64_t window(size_t) const { return 0; }
};
struct PairSrc {
    using Raw = uint32_t;
    static constexpr bool kFromText = false;
    const uint32_t *__restrict__ keys;
    const uint64_t *__restrict__ vals;
    __device__ __forceinline__ Raw load(size_t idx, const TileExtent &) const { return keys[idx]; }
    __device__ __forceinline__ uint32_t key_of(Raw raw, size_t, const TileExtent &) const { return raw; }
    __device__ __forceinline__ uint32_t hist_digit_of(Raw raw, size_t, int shift, const TileExtent &) const { return digit_of(raw, shift); }
    __device__ __forceinline__ uint64_t val(size_t idx) const { return vals[idx]; }
    __device__ __forceinline__ bool digits_from_window(int) const { return false; }
    __device__ __forceinline__ uint64_t window(size_t) const { return 0; }
};
// (position, value) pairs of a block-diagonal permutation (RecordScatterPlan): the key is the position
// inside the record, ext.aux = first position of the tile's record
struct LocalIdxSrc {
    using Raw = uint32_t;
    static constexpr bool kFromText = false;
    const uint32_t *__restrict__ idx;
    const uint32_t *__restrict__ vals;
    __device__ __forceinline__ Raw load(size_t i, const TileExtent &) const { return idx[i]; }
    __device__ __forceinline__ uint32_t key_of(Raw raw, size_t, const TileExtent &ext) const { return raw - ext.aux; }
    __device__ __forceinline__ uint32_t hist_digit_of(Raw raw, size_t, int shift, const TileExtent &ext) const { return digit_of(raw - ext.aux, shift); }
    __device__ __forceinline__ uint32_t val(size_t i) const { return vals[i]; }
    __device__ __forceinline__ bool digits_from_window(int) const { return false; }
    __device__ __forceinline__ uint64_t window(size_t) const { return 0; }
};

// the same with the list position + 1 as a second value (RankSrc): the block-diagonal permutation of a merged batch
// delivers the inverse suffix array on the way, too
struct LocalRankSrc {
    using Raw = uint32_t;
    static constexpr bool kFromText = false;
    const uint32_t *__restrict__ idx;
    const uint32_t *__restrict__ vals;
    __device__ __forceinline__ Raw load(size_t i, const TileExtent &) const { return idx[i]; }
    __device__ __forceinline__ uint32_t key_of(Raw raw, size_t, const TileExtent &ext) const { return raw - ext.aux; }
    __device__ __forceinline__ uint32_t hist_digit_of(Raw raw, size_t, int shift, const TileExtent &ext) const { return digit_of(raw - ext.aux, shift); }
    __device__ __forceinline__ uint64_t val(size_t i) const { return (uint64_t)vals[i] | ((uint64_t)((uint32_t)i + 1u) << 32); }
    __device__ __forceinline__ bool digits_from_window(int) const { return false; }
    __device__ __forceinline__ uint64_t window(size_t) const { return 0; }
};

__global__ __launch_bounds__(kThreads) void plain_scatter_kernel(const uint32_t *__restrict__ idx,
                                                                 const uint32_t *__restrict__ val, size_t count,
                                                                 uint32_t *__restrict__ out, uint32_t n_out,
                                                                 uint32_t num_tiles) {
    const uint32_t tile = xcd_tile(blockIdx.x, num_tiles);
    if (tile == 0xffffffffu) return;
    const size_t base = (size_t)tile * kTile;
#pragma unroll
    for (int j = 0; j < kKeysPerThread; ++j) {
        const size_t k = base + (size_t)j * kThreads + threadIdx.x;
        if (k < count) {
            const uint32_t i = idx[k];
            if (i < n_out) out[i] = val[k];
        }
    }
}

// out[idx[k]] = low half, out2[idx[k]] = high half of packed[k] (small inputs of permute_packed)
__global__ __launch_bounds__(kThreads) void plain_packed_scatter_kernel(const uint32_t *__restrict__ idx,
                                                                        const uint64_t *__restrict__ packed, size_t count,
                                                                        uint32_t *__restrict__ out, uint32_t *__restrict__ out2) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x; k < count; k += stride) {
        const uint32_t i = idx[k];
        const uint64_t v = packed[k];
        if (i < count) {
            out[i] = (uint32_t)v;
            out2[i] = (uint32_t)(v >> 32);
        }
    }
}

// out2[idx[k]] = k + 1 (small inputs: the second value of bucketed_scatter's out2 form, written directly)
__global__ __launch_bounds__(kThreads) void plain_rank_scatter_kernel(const uint32_t *__restrict__ idx, size_t count,
                                                                      uint32_t *__restrict__ out2, uint32_t n_out) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x; k < count; k += stride) {
        const uint32_t i = idx[k];
        if (i < n_out) out2[i] = (uint32_t)k + 1u;
    }
}

constexpr int kWindowBitsMax = 14;  // 2^14 entries = 64 KiB of LDS

// permutation scatter, final step: the pairs of window w sit at list positions [w*W, (w+1)*W)
// (IdxT = uint16_t: the last partition pass kept only the low 16 bits of every index -- what lies above the
// window bits is implied by the position in the list)
template <typename IdxT>
__global__ __launch_bounds__(kThreads) void window_scatter_kernel(const IdxT *__restrict__ idx,
                                                                  const uint32_t *__restrict__ val,
                                                                  uint32_t *__restrict__ out, uint32_t n_out,
                                                                  int window_bits) {
    __shared__ uint32_t s_out[1 << kWindowBitsMax];
    const uint32_t W = 1u << window_bits;
    const size_t base = (size_t)blockIdx.x << window_bits;
    const uint32_t len = (uint32_t)((n_out - base < (size_t)W) ? (n_out - base) : (size_t)W);
    // eight (index, value) pairs per thread in flight at a time
    constexpr int kBatch = 8;
    for (uint32_t t0 = 0; t0 < len; t0 += kBatch * kThreads) {
        uint32_t ii[kBatch], vv[kBatch];
#pragma unroll
        for (int j = 0; j < kBatch; ++j) {
            const uint32_t t = t0 + (uint32_t)j * kThreads + threadIdx.x;
            const size_t at = base + (t < len ? t : 0u);  // (no branch around the loads)
            ii[j] = (uint32_t)idx[at];
            vv[j] = val[at];
        }
#pragma unroll
        for (int j = 0; j < kBatch; ++j) {
            const uint32_t t = t0 + (uint32_t)j * kThreads + threadIdx.x;
            if (t < len) s_out[ii[j] & (W - 1u)] = vv[j];  // (the window starts at a multiple of W)
        }
    }
    __syncthreads();
    for (uint32_t t = threadIdx.x; t < len; t += kThreads) out[base + t] = s_out[t];
}

// the same for pairs that carry two values in one 64-bit word (low half -> out, high half -> out2): both windows
// are assembled side by side in 128 KiB of LDS by one workgroup of 1024 threads per CU
constexpr int kWindow2Threads = 1024;
__global__ __launch_bounds__(kWindow2Threads) void window_scatter2_kernel(const uint16_t *__restrict__ idx,
                                                                          const uint64_t *__restrict__ val,
                                                                          uint32_t *__restrict__ out,
                                                                          uint32_t *__restrict__ out2, uint32_t n_out,
                                                                          int window_bits) {
    __shared__ uint32_t s_out[2 << kWindowBitsMax];
    const uint32_t W = 1u << window_bits;
    uint32_t *s_a = s_out, *s_b = s_out + W;
    const size_t base = (size_t)blockIdx.x << window_bits;
    const uint32_t len = (uint32_t)((n_out - base < (size_t)W) ? (n_out - base) : (size_t)W);
    constexpr int kBatch = 4;
    for (uint32_t t0 = 0; t0 < len; t0 += kBatch * kWindow2Threads) {
        uint32_t ii[kBatch];
        uint64_t vv[kBatch];
#pragma unroll
        for (int j = 0; j < kBatch; ++j) {
            const uint32_t t = t0 + (uint32_t)j * kWindow2Threads + threadIdx.x;
            const size_t at = base + (t < len ? t : 0u);  // (no branch around the loads)
            ii[j] = (uint32_t)idx[at];
            vv[j] = val[at];
        }
#pragma unroll
        for (int j = 0; j < kBatch; ++j) {
            const uint32_t t = t0 + (uint32_t)j * kWindow2Threads + threadIdx.x;
            if (t < len) {
                s_a[ii[j] & (W - 1u)] = (uint32_t)vv[j];
                s_b[ii[j] & (W - 1u)] = (uint32_t)(vv[j] >> 32);
            }
        }
    }
    __syncthreads();
    for (uint32_t t = threadIdx.x; t < len; t += kWindow2Threads) {
        out[base + t] = s_a[t];
        out2[base + t] = s_b[t];
    }
}

// the same for the windows of a RecordScatterPlan: window b = list elements [win[3b], +win[3b+2]) -> target
// elements [win[3b+1], +win[3b+2]); the low window_bits of an index are its place in the window
template <typename IdxT>
__global__ __launch_bounds__(kThreads) void record_window_scatter_kernel(const IdxT *__restrict__ idx,
                                                                         const uint32_t *__restrict__ val,
                                                                         uint32_t *__restrict__ out,
                                                                         const uint32_t *__restrict__ win,
                                                                         int window_bits) {
    __shared__ uint32_t s_out[1 << kWindowBitsMax];
    const uint32_t W = 1u << window_bits;
    const size_t base = win[3 * (size_t)blockIdx.x];
    const size_t obase = win[3 * (size_t)blockIdx.x + 1];
    const uint32_t len = win[3 * (size_t)blockIdx.x + 2];
    constexpr int kBatch = 8;
    for (uint32_t t0 = 0; t0 < len; t0 += kBatch * kThreads) {
        uint32_t ii[kBatch], vv[kBatch];
#pragma unroll
        for (int j = 0; j < kBatch; ++j) {
            const uint32_t t = t0 + (uint32_t)j * kThreads + threadIdx.x;
            const size_t at = base + (t < len ? t : 0u);  // (no branch around the loads)
            ii[j] = (uint32_t)idx[at];
            vv[j] = val[at];
        }
#pragma unroll
        for (int j = 0; j < kBatch; ++j) {
            const uint32_t t = t0 + (uint32_t)j * kThreads + threadIdx.x;
            if (t < len) s_out[ii[j] & (W - 1u)] = vv[j];
        }
    }
    __syncthreads();
    for (uint32_t t = threadIdx.x; t < len; t += kThreads) out[obase + t] = s_out[t];
}

// two values per pair in one 64-bit word (low half -> out, high half -> out2), as window_scatter2_kernel
__global__ __launch_bounds__(kWindow2Threads) void record_window_scatter2_kernel(const uint16_t *__restrict__ idx,
                                                                                 const uint64_t *__restrict__ val,
                                                                                 uint32_t *__restrict__ out,
                                                                                 uint32_t *__restrict__ out2,
                                                                                 const uint32_t *__restrict__ win,
                                                                                 int window_bits) {
    __shared__ uint32_t s_out[2 << kWindowBitsMax];
    const uint32_t W = 1u << window_bits;
    uint32_t *s_a = s_out, *s_b = s_out + W;
    const size_t base = win[3 * (size_t)blockIdx.x];
    const size_t obase = win[3 * (size_t)blockIdx.x + 1];
    const uint32_t len = win[3 * (size_t)blockIdx.x + 2];
    constexpr int kBatch = 4;
    for (uint32_t t0 = 0; t0 < len; t0 += kBatch * kWindow2Threads) {
        uint32_t ii[kBatch];
        uint64_t vv[kBatch];
#pragma unroll
        for (int j = 0; j < kBatch; ++j) {
            const uint32_t t = t0 + (uint32_t)j * kWindow2Threads + threadIdx.x;
            const size_t at = base + (t < len ? t : 0u);  // (no branch around the loads)
            ii[j] = (uint32_t)idx[at];
            vv[j] = val[at];
        }
#pragma unroll
        for (int j = 0; j < kBatch; ++j) {
            const uint32_t t = t0 + (uint32_t)j * kWindow2Threads + threadIdx.x;
            if (t < len) {
                s_a[ii[j] & (W - 1u)] = (uint32_t)vv[j];
                s_b[ii[j] & (W - 1u)] = (uint32_t)(vv[j] >> 32);
            }
        }
    }
    __syncthreads();
    for (uint32_t t = threadIdx.x; t < len; t += kWindow2Threads) {
        out[obase + t] = s_a[t];
        out2[obase + t] = s_b[t];
    }
}

__global__ void separator_scatter_kernel(const uint32_t *__restrict__ sep, uint32_t count,
                                         const uint32_t *__restrict__ idx, const uint32_t *__restrict__ val,
                                         uint32_t *__restrict__ out, uint32_t *__restrict__ err,
                                         uint32_t *__restrict__ out2) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= count) return;
    const uint32_t r = sep[2 * k], p = sep[2 * k + 1];
    if (idx[r] != p) atomicOr(err, 1u);  // the separator suffix is the first of its record
    out[p] = val[r];
    if (out2) out2[p] = r + 1u;
}

// ---- the two-value permutation without histograms (bucketed_scatter, texts of up to 2^30 symbols) ----------------
// idx is a permutation of [0, n): bin d of the first pass is exactly the target range [d << (wb + 8), (d + 1) << (wb + 8)),
// sub-bin (d, e) of the second pass exactly window d * 256 + e.  A tile's offset inside its bin is the count of the
// digit in the tiles in front of it, found by a decoupled look-back per digit (thread d walks digit d, so the
// descriptor reads of a step are one 2 KiB row) instead of a histogram pass and a scan.  The pair travels as ONE word
// [code : c | rank : nb | low wb + 8 index bits] (c = 64 - nb - (wb + 8) >= 12 bits): the first pass keeps only the
// index bits below its digit, the second pass moves the words unchanged (its digit is bits [wb, wb + 8)), the window
// kernel takes the low wb bits as the place in the window.  A code that does not fit its field is stored as `esc` and
// its rank goes to an exception list; escape_fixup_kernel writes those codes behind the windows.
// 16 Ki pairs per tile and one ticket per tile: tiles start in ticket order, so a look-back only ever waits on tiles
// that are already running (forward progress), and 2^16 tickets at 2^30 pairs stay far below the rate one atomic
// word can hand out.  128 KiB of staged words: one workgroup of 1024 threads per CU.  (NOLZSS_LB_TILE_BITS=13: 8 Ki pairs
// on 512 threads, two workgroups per CU -- within 0.15 ms per step of this, profiles/r05_text_order_ab.txt.)
#ifndef NOLZSS_LB_TILE_BITS
#define NOLZSS_LB_TILE_BITS 14
#endif
constexpr int kLbTileBits = NOLZSS_LB_TILE_BITS;
constexpr int kLbTile = 1 << kLbTileBits;
constexpr int kLbThreads = kLbTile / kKeysPerThread;
constexpr int kLbWaves = kLbThreads / 64;
static_assert(kLbTileBits == 13 || kLbTileBits == 14, "512 or 1024 threads, 16 pairs each");
static_assert(kLbThreads >= kBins && kWaveSpan * kLbWaves == kLbTile, "one thread per digit");
constexpr int kLbLook = 4;  // descriptors per lane and round trip of the walk

struct LbPass {
    const uint32_t *idx = nullptr;   // first pass: target positions (sa) ...
    const uint32_t *code = nullptr;  // ... and the codes, in list (rank) order
    const uint64_t *in = nullptr;    // second pass: the words of the first
    uint64_t *out = nullptr;
    uint64_t *desc = nullptr;  // kBins descriptors per tile, zero on entry
    uint32_t *ctl = nullptr;   // [0] ticket, [1] look-back gave up, [2] exceptions (may exceed the cap)
    uint32_t *exc = nullptr;   // ranks of the escaped codes
    uint32_t exc_cap = 0;
    uint32_t esc = 0;  // codes >= esc are escaped (esc < 2^c)
    uint32_t n = 0;
    int dshift = 0;     // digit = (target position >> dshift) & 255
    int low_bits = 0;   // wb + 8
    int rank_bits = 0;  // nb
};

template <bool kFirst>
__global__ __launch_bounds__(kLbThreads, 4) void lb_partition_kernel(LbPass p) {  // (16 wavefronts per CU: 128 VGPRs)
    __shared__ __align__(16) uint64_t s_rec[kLbTile];
    __shared__ __align__(16) uint32_t s_whist[kLbWaves * kBins];  // per-wave digit counts; then the staged digits
    __shared__ uint32_t s_glob[kBins];
    __shared__ uint32_t s_scan[kLbWaves];
    __shared__ uint32_t s_tile;
    uint8_t *s_dig = reinterpret_cast<uint8_t *>(s_whist);
    static_assert(sizeof(s_whist) >= kLbTile, "one digit byte per staged word");

    const int tid = threadIdx.x;
    const int w = tid >> 6;
    const int lane = tid & 63;
    if (tid == 0) s_tile = atomicAdd(p.ctl, 1u);  // tiles in start order
    for (int i = tid; i < kLbWaves * kBins; i += kLbThreads) s_whist[i] = 0;
    __syncthreads();
    const uint32_t tile = s_tile;  // < gridDim.x: one ticket per workgroup
    const size_t first = (size_t)tile << kLbTileBits;
    const uint32_t count = (uint32_t)((size_t)p.n - first < (size_t)kLbTile ? (size_t)p.n - first : (size_t)kLbTile);

    // The words go to LDS in list order first and only the digits stay in registers through the ranking: words, ranks
    // and the ranking's own state do not fit the 128 VGPRs of 16 wavefronts per CU (43 of them spilled).  They are
    // moved to their sorted places inside LDS once the ranks are known.
    uint32_t lrank[kKeysPerThread];
    uint32_t dpk[kKeysPerThread / 4] = {0, 0, 0, 0};  // the digits, four per register
    auto digit_at = [&](int row) -> uint32_t { return (dpk[row >> 2] >> (8 * (row & 3))) & 255u; };
    const uint32_t local0 = (uint32_t)w * kWaveSpan + lane;  // element of row `row`: local0 + 64 * row
    if constexpr (kFirst) {
        uint32_t ii[kKeysPerThread], cc[kKeysPerThread];
#pragma unroll
        for (int row = 0; row < kKeysPerThread; ++row) {
            const uint32_t local = local0 + (uint32_t)row * 64;
            const size_t at = first + (local < count ? local : 0u);  // (past the end: the first element again)
            ii[row] = p.idx[at];
            cc[row] = p.code[at];
        }
        const uint64_t low_mask = (1ull << p.low_bits) - 1ull;
#pragma unroll
        for (int row = 0; row < kKeysPerThread; ++row) {
            const uint32_t local = local0 + (uint32_t)row * 64;
            const uint32_t r = (uint32_t)first + local;
            const bool escaped = local < count && cc[row] >= p.esc;
            s_rec[local] = ((uint64_t)ii[row] & low_mask) | ((uint64_t)r << p.low_bits) |
                           ((uint64_t)(escaped ? p.esc : cc[row]) << (p.low_bits + p.rank_bits));
            dpk[row >> 2] |= ((ii[row] >> p.dshift) & 255u) << (8 * (row & 3));
            const uint64_t bal = __ballot(escaped);
            if (bal) {  // (wave-uniform; rare) one atomic per wavefront
                const int leader = __builtin_ctzll(bal);
                uint32_t slot = 0;
                if (lane == leader) slot = atomicAdd(p.ctl + 2, (uint32_t)__popcll(bal));
                slot = (uint32_t)__shfl((int)slot, leader, 64) + (uint32_t)__popcll(bal & lanemask_lt());
                if (escaped && slot < p.exc_cap) p.exc[slot] = r;
            }
        }
    } else {
        uint64_t x[kKeysPerThread];
#pragma unroll
        for (int row = 0; row < kKeysPerThread; ++row) {
            const uint32_t local = local0 + (uint32_t)row * 64;
            x[row] = p.in[first + (local < count ? local : 0u)];
        }
#pragma unroll
        for (int row = 0; row < kKeysPerThread; ++row) {
            s_rec[local0 + (uint32_t)row * 64] = x[row];
            dpk[row >> 2] |= ((uint32_t)(x[row] >> p.dshift) & 255u) << (8 * (row & 3));
        }
    }
    // rank inside the wavefront, as in rs_scatter_kernel (rows of 64 in list order: stable)
    uint32_t *wcount = s_whist + w * kBins;
#pragma unroll
    for (int row = 0; row < kKeysPerThread; ++row) {
        const bool valid = (uint32_t)w * kWaveSpan + (uint32_t)row * 64 + lane < count;
        const uint32_t d = digit_at(row);
        uint32_t diff_lo = 0, diff_hi = 0;
#pragma unroll
        for (int b = 0; b < kRadixBits; ++b) {
            const uint32_t m = (uint32_t)__builtin_amdgcn_sbfe((int)d, (unsigned)b, 1u);
            const uint64_t bal = __ballot((int)m < 0);
            diff_lo = __builtin_amdgcn_bitop3_b32(m, diff_lo, (uint32_t)bal, 0xde);
            diff_hi = __builtin_amdgcn_bitop3_b32(m, diff_hi, (uint32_t)(bal >> 32), 0xde);
        }
        const uint64_t peers = ~(((uint64_t)diff_hi << 32) | diff_lo) & __ballot(valid);
        const uint64_t below = peers & lanemask_lt();
        uint32_t seen = 0;
        if (valid && below == 0) seen = atomicAdd(&wcount[d], (uint32_t)__popcll(peers));
        lrank[row] = seen | ((uint32_t)__popcll(below) << 11) | ((uint32_t)(peers ? __builtin_ctzll(peers) : 0) << 17);
    }
#pragma unroll
    for (int row = 0; row < kKeysPerThread; ++row) {
        const uint32_t packed = lrank[row];
        lrank[row] = ((uint32_t)__shfl((int)packed, (int)(packed >> 17), 64) & 0x7ffu) + ((packed >> 11) & 63u);
    }
    __syncthreads();

    // thread = digit (the first kBins threads): tile-local bin starts; the tile's count of the digit is published at once
    const int d = tid;
    const bool owner = tid < kBins;
    const uint32_t chain = (uint32_t)(first >> (p.dshift + kRadixBits));  // second pass: the bucket of the first
    const uint32_t t0 = (uint32_t)(((size_t)chain << (p.dshift + kRadixBits)) >> kLbTileBits);  // its first tile
    uint64_t *my_desc = p.desc + (size_t)tile * kBins + d;
    uint32_t bin_start, total = 0;
    {
        if (owner)
            for (int k = 0; k < kLbWaves; ++k) total += s_whist[k * kBins + d];
        if (owner) desc_store(my_desc, ((tile == t0 ? 2ull : 1ull) << 32) | total);
        uint32_t tile_total;
        bin_start = block_scan_exclusive<kLbWaves>(total, OpAdd<uint32_t>(), s_scan, tile_total);
        if (owner) {
            uint32_t run = bin_start;
            for (int k = 0; k < kLbWaves; ++k) {
                const uint32_t c = s_whist[k * kBins + d];
                s_whist[k * kBins + d] = run;
                run += c;
            }
        }
    }
    __syncthreads();
    uint64_t rec[kKeysPerThread];
#pragma unroll
    for (int row = 0; row < kKeysPerThread; ++row) {
        lrank[row] += s_whist[w * kBins + digit_at(row)];
        rec[row] = s_rec[local0 + (uint32_t)row * 64];
    }
    __syncthreads();  // (s_whist becomes s_dig; s_rec is read)
#pragma unroll
    for (int row = 0; row < kKeysPerThread; ++row) {
        if (local0 + (uint32_t)row * 64 < count) {
            s_rec[lrank[row]] = rec[row];
            if constexpr (kFirst) s_dig[lrank[row]] = (uint8_t)digit_at(row);
        }
    }
    // the walk, as late as possible: the tiles in front have had the whole staging to publish their prefixes
    if (owner) {
        uint32_t excl = 0;
        if (tile != t0) {
            int64_t look = (int64_t)tile - 1;
            uint32_t spins = 0;
            for (;;) {
                uint64_t v[kLbLook];
#pragma unroll
                for (int j = 0; j < kLbLook; ++j) {
                    const int64_t k = look - j;  // in front of the chain's first tile: inclusive identity
                    v[j] = k >= (int64_t)t0 ? desc_load(p.desc + (size_t)k * kBins + d) : (2ull << 32);
                }
                bool done = false, stalled = false;
#pragma unroll
                for (int j = 0; j < kLbLook; ++j) {
                    if (done || stalled) continue;
                    const uint32_t st = (uint32_t)(v[j] >> 32);
                    if (st == 0) {
                        stalled = true;
                    } else {
                        excl += (uint32_t)v[j];
                        --look;
                        done = st == 2;
                    }
                }
                if (done) break;
                if (stalled) {
                    if (++spins > kSpinLimit) {  // cannot happen with ticket order; never hang the GPU
                        atomicExch(p.ctl + 1, 1u);
                        break;
                    }
                    __builtin_amdgcn_s_sleep(1);
                }
            }
            desc_store(my_desc, (2ull << 32) | (uint64_t)(excl + total));
        }
        s_glob[d] = ((((uint32_t)chain << kRadixBits) | (uint32_t)d) << p.dshift) + excl - bin_start;
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < kKeysPerThread; ++j) {
        const uint32_t q = (uint32_t)j * kLbThreads + tid;
        if (q < count) {
            const uint64_t x = s_rec[q];
            const uint32_t dq = kFirst ? (uint32_t)s_dig[q] : (uint32_t)(x >> p.dshift) & 255u;
            const uint32_t g = s_glob[dq] + q;
            if (g < p.n) p.out[g] = x;  // (always, for a permutation)
        }
    }
}

// the windows of the packed words: out[i] = code, out2[i] = rank + 1 for the words of window blockIdx.x (16 B per pair)
__global__ __launch_bounds__(kWindow2Threads) void window_unpack_kernel(const uint64_t *__restrict__ in,
                                                                        uint32_t *__restrict__ out,
                                                                        uint32_t *__restrict__ out2, uint32_t n_out,
                                                                        int window_bits, int low_bits, int rank_bits) {
    __shared__ uint32_t s_out[2 << kWindowBitsMax];
    const uint32_t W = 1u << window_bits;
    uint32_t *s_a = s_out, *s_b = s_out + W;
    const size_t base = (size_t)blockIdx.x << window_bits;
    const uint32_t len = (uint32_t)((n_out - base < (size_t)W) ? (n_out - base) : (size_t)W);
    const uint32_t rank_mask = (uint32_t)((1ull << rank_bits) - 1ull);
    constexpr int kBatch = 4;
    for (uint32_t t0 = 0; t0 < len; t0 += kBatch * kWindow2Threads) {
        uint64_t vv[kBatch];
#pragma unroll
        for (int j = 0; j < kBatch; ++j) {
            const uint32_t t = t0 + (uint32_t)j * kWindow2Threads + threadIdx.x;
            vv[j] = in[base + (t < len ? t : 0u)];  // (no branch around the loads)
        }
#pragma unroll
        for (int j = 0; j < kBatch; ++j) {
            const uint32_t t = t0 + (uint32_t)j * kWindow2Threads + threadIdx.x;
            if (t < len) {
                const uint32_t at = (uint32_t)vv[j] & (W - 1u);
                s_a[at] = (uint32_t)(vv[j] >> (low_bits + rank_bits));
                s_b[at] = ((uint32_t)(vv[j] >> low_bits) & rank_mask) + 1u;
            }
        }
    }
    __syncthreads();
    for (uint32_t t = threadIdx.x; t < len; t += kWindow2Threads) {
        out[base + t] = s_a[t];
        out2[base + t] = s_b[t];
    }
}

// The 16-bit form of the codes (code16.hpp): the codes of a window are staged as uint16_t and leave 16 bytes per lane,
// the ranks as above -- 96 KiB of LDS, 8 + 6 bytes per pair.  A code of wl.max or more is stored as wl.max and goes to
// the wide-code list (an escaped code too, with the threshold as its value: escape_fixup_kernel appends the true one).
__global__ __launch_bounds__(kWindow2Threads) void window_unpack16_kernel(const uint64_t *__restrict__ in,
                                                                          uint16_t *__restrict__ out,
                                                                          uint32_t *__restrict__ out2, uint32_t n_out,
                                                                          int window_bits, int low_bits, int rank_bits,
                                                                          WideCodes wl) {
    __shared__ __align__(16) uint32_t s_b[1 << kWindowBitsMax];
    __shared__ __align__(16) uint16_t s_a[1 << kWindowBitsMax];
    const uint32_t W = 1u << window_bits;
    const size_t base = (size_t)blockIdx.x << window_bits;
    const uint32_t len = (uint32_t)((n_out - base < (size_t)W) ? (n_out - base) : (size_t)W);
    const uint32_t rank_mask = (uint32_t)((1ull << rank_bits) - 1ull);
    constexpr int kBatch = 4;
    for (uint32_t t0 = 0; t0 < len; t0 += kBatch * kWindow2Threads) {
        uint64_t vv[kBatch];
#pragma unroll
        for (int j = 0; j < kBatch; ++j) {
            const uint32_t t = t0 + (uint32_t)j * kWindow2Threads + threadIdx.x;
            vv[j] = in[base + (t < len ? t : 0u)];  // (no branch around the loads)
        }
#pragma unroll
        for (int j = 0; j < kBatch; ++j) {
            const uint32_t t = t0 + (uint32_t)j * kWindow2Threads + threadIdx.x;
            const uint32_t at = (uint32_t)vv[j] & (W - 1u);
            const uint32_t code = (uint32_t)(vv[j] >> (low_bits + rank_bits));
            const bool big = t < len && code >= wl.max;
            if (t < len) {
                s_a[at] = (uint16_t)(big ? wl.max : code);
                s_b[at] = ((uint32_t)(vv[j] >> low_bits) & rank_mask) + 1u;
            }
            append_wide_code(wl, (uint32_t)base + at, code, big);
        }
    }
    __syncthreads();
    for (uint32_t t = threadIdx.x; t < len; t += kWindow2Threads) out2[base + t] = s_b[t];
    // (a window starts at a multiple of 1024 codes: the 16-byte stores are aligned)
    for (uint32_t t = threadIdx.x * 8u; t < len; t += kWindow2Threads * 8u) {
        if (t + 8u <= len) {
            *reinterpret_cast<uint4 *>(out + base + t) = *reinterpret_cast<const uint4 *>(s_a + t);
        } else {
            for (uint32_t k = t; k < len; ++k) out[base + k] = s_a[k];
        }
    }
}

// out[idx[r]] = code[r] for the escaped ranks (none when the list overflowed: the caller then starts over)
__global__ __launch_bounds__(kThreads) void escape_fixup_kernel(const uint32_t *__restrict__ exc, const uint32_t *__restrict__ ctl,
                                                                uint32_t cap, const uint32_t *__restrict__ idx,
                                                                const uint32_t *__restrict__ code, LstarCodes out) {
    const uint32_t cnt = ctl[2];
    if (cnt > cap) return;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x; k < cnt; k += stride) {
        const uint32_t r = exc[k];
        store_code(out, idx[r], code[r]);
    }
}

// (NOLZSS_TRACE) cnt[k] = codes >= 2^(10 + k), k < 7: how often the escape would be taken at each field width
__global__ __launch_bounds__(kThreads) void code_census_kernel(const uint32_t *__restrict__ code, size_t count,
                                                               unsigned long long *__restrict__ cnt) {
    uint32_t c[7] = {0, 0, 0, 0, 0, 0, 0};
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x; k < count; k += stride) {
        const uint32_t v = code[k];
#pragma unroll
        for (int b = 0; b < 7; ++b) c[b] += v >= (1u << (10 + b)) ? 1u : 0u;
    }
#pragma unroll
    for (int b = 0; b < 7; ++b) {
        const uint32_t t = wave_reduce(c[b], OpAdd<uint32_t>());
        if (lane_id() == 0 && t) atomicAdd(cnt + b, (unsigned long long)t);
    }
}

// lstar[sa[r]] = code[r], isa[sa[r]] = r + 1 by the kernels above; false (nothing usable written) when the exception
// list overflowed or a look-back gave up -- the caller then runs the histogram form.  out.narrow: the codes leave as
// uint16_t (code16.hpp).
bool packed_text_order(const uint32_t *idx, const uint32_t *code, size_t count, const LstarCodes &out, uint32_t *out2, int nb, int wb,
                       uint64_t *buf_a, Arena &arena, hipStream_t stream, Profiler *prof, TextOrderReport &report) {
    const bool trace = sort_knobs().trace;
    const int low_bits = wb + kRadixBits;
    const int code_bits = 64 - nb - low_bits;  // >= 12 for nb <= 30
    uint32_t esc = (uint32_t)((1ull << code_bits) - 1ull);
    if (sort_knobs().text_order_esc >= 0) esc = std::min<uint32_t>(esc, (uint32_t)sort_knobs().text_order_esc);
    const uint32_t num_tiles = (uint32_t)div_up(count, kLbTile);
    const uint32_t cap = (uint32_t)std::max<size_t>(count / 64, 1024);
    uint64_t *buf_b = arena.alloc<uint64_t>(count);
    uint64_t *desc = arena.alloc<uint64_t>((size_t)kBins * num_tiles);
    uint32_t *exc = arena.alloc<uint32_t>(cap);
    uint32_t *ctl = arena.alloc<uint32_t>(8);  // [0, 1, 2] first pass, [4, 5, 6] second pass
    HIP_CHECK(hipMemsetAsync(ctl, 0, 8 * sizeof(uint32_t), stream));
    LbPass p;
    p.n = (uint32_t)count;
    p.exc = exc;
    p.exc_cap = cap;
    p.esc = esc;
    p.low_bits = low_bits;
    p.rank_bits = nb;
    p.desc = desc;
    {
        ProfScope ps(prof, "rs_scatter.u32", stream, 16.0 * (double)count);
        HIP_CHECK(hipMemsetAsync(desc, 0, (size_t)kBins * num_tiles * sizeof(uint64_t), stream));
        p.idx = idx;
        p.code = code;
        p.out = buf_a;
        p.ctl = ctl;
        p.dshift = wb + kRadixBits;
        lb_partition_kernel<true><<<num_tiles, kLbThreads, 0, stream>>>(p);
        KERNEL_CHECK();
    }
    {
        ProfScope ps(prof, "rs_scatter.u32", stream, 16.0 * (double)count);
        HIP_CHECK(hipMemsetAsync(desc, 0, (size_t)kBins * num_tiles * sizeof(uint64_t), stream));
        p.idx = p.code = nullptr;
        p.in = buf_a;
        p.out = buf_b;
        p.ctl = ctl + 4;
        p.dshift = wb;
        lb_partition_kernel<false><<<num_tiles, kLbThreads, 0, stream>>>(p);
        KERNEL_CHECK();
    }
    {
        ProfScope ps(prof, "window_scatter", stream, (out.narrow ? 14.0 : 16.0) * (double)count);
        const unsigned windows = (unsigned)div_up(count, (size_t)1 << wb);
        if (out.narrow)
            window_unpack16_kernel<<<windows, kWindow2Threads, 0, stream>>>(buf_b, out.narrow, out2, (uint32_t)count, wb, low_bits,
                                                                           nb, out.list);
        else
            window_unpack_kernel<<<windows, kWindow2Threads, 0, stream>>>(buf_b, out.wide, out2, (uint32_t)count, wb, low_bits, nb);
        KERNEL_CHECK();
        escape_fixup_kernel<<<256, kThreads, 0, stream>>>(exc, ctl, cap, idx, code, out);
        KERNEL_CHECK();
    }
    uint32_t h[8];
    HIP_CHECK(hipMemcpyAsync(h, ctl, sizeof(h), hipMemcpyDeviceToHost, stream));
    HIP_CHECK(hipStreamSynchronize(stream));
    const bool ok = h[1] == 0 && h[5] == 0 && h[2] <= cap;
    report.packed_tried = true;
    report.escaped = h[2];
    report.list_overflow = h[2] > cap;
    report.lookback_gave_up = h[1] != 0 || h[5] != 0;
    if (trace) {
        unsigned long long *d_cnt = arena.alloc<unsigned long long>(7), hc[7];
        HIP_CHECK(hipMemsetAsync(d_cnt, 0, sizeof(hc), stream));
        code_census_kernel<<<1024, kThreads, 0, stream>>>(code, count, d_cnt);
        KERNEL_CHECK();
        HIP_CHECK(hipMemcpyAsync(hc, d_cnt, sizeof(hc), hipMemcpyDeviceToHost, stream));
        HIP_CHECK(hipStreamSynchronize(stream));
        fprintf(stderr, "[nolzss] text order: %zu codes, >= 2^10..2^16: %llu %llu %llu %llu %llu %llu %llu\n", count, hc[0], hc[1],
                hc[2], hc[3], hc[4], hc[5], hc[6]);
    }
    if (trace)
        fprintf(stderr, "[nolzss] text order: packed look-back partition, %u escaped codes (cap %u, threshold %u)%s\n", h[2], cap,
                esc, ok ? "" : (h[2] > cap ? ": list overflow, histogram form instead" : ": look-back gave up, histogram form instead"));
    return ok;
}

}  // namespace

bool record_scatter_plan(const std::vector<uint32_t> &h_terms, uint32_t n, Arena &arena, hipStream_t stream,
                         RecordScatterPlan &plan) {
    plan = RecordScatterPlan{};
    const uint32_t nb = (uint32_t)h_terms.size();
    // (partial tiles and windows cost 4096 / the average record: NOLZSS_REC_BUCKET_MIN, as for the key sort)
    const uint64_t rec_min = sort_knobs().rec_bucket_min;
    if (nb < 2 || h_terms.back() != n || rec_min == 0 || (uint64_t)nb * rec_min > (uint64_t)n) return false;
    constexpr int wb = kWindowBitsMax;
    // bucket k = the BASES of record k: ranks [first_k, end_k) hold positions [start_k, start_k + len_k)
    // (the separator behind a record is the smallest suffix of the record: its first rank)
    std::vector<uint32_t> tab(5 * ((size_t)nb + 1)), sep(2 * ((size_t)nb - 1));
    uint32_t *h_first = tab.data(), *h_tile0 = h_first + nb + 1, *h_prev = h_tile0 + nb + 1, *h_next = h_prev + nb + 1,
             *h_aux = h_next + nb + 1;
    std::vector<uint32_t> win;
    uint32_t start = 0, dense = 0;
    h_tile0[0] = 0;
    for (uint32_t k = 0; k < nb; ++k) {
        const uint32_t end = k + 1 < nb ? h_terms[k] + 1 : n;     // end of the record's ranks / positions
        const uint32_t len = (k + 1 < nb ? h_terms[k] : n) - start;  // bases
        if (len == 0 || len > (1u << (wb + kRadixBits))) return false;
        h_first[k] = k + 1 < nb ? start + 1 : start;  // first base rank
        h_aux[k] = start;
        {
            // tiles behind the first one start at multiples of 64 elements: a wavefront's 64-lane loads are
            // then aligned to their 256 bytes (a bucket starts wherever its record does; unaligned, every row
            // of a tile touches three lines instead of two and the pass ran 1.4 x slower)
            const uint32_t f0 = k + 1 < nb ? start + 1 : start;
            const uint32_t c0 = (uint32_t)kTile - f0 % 64u;
            h_tile0[k + 1] = h_tile0[k] + (len <= c0 ? 1u : 1u + (uint32_t)div_up((size_t)(len - c0), kTile));
        }
        h_prev[k] = k ? k - 1 : 0xffffffffu;
        h_next[k] = k + 1 < nb ? k + 1 : 0xffffffffu;
        if (k + 1 < nb) {
            sep[2 * (size_t)k] = start;             // rank of the separator suffix
            sep[2 * (size_t)k + 1] = h_terms[k];    // its position
        }
        for (uint32_t w0 = 0; w0 < len; w0 += 1u << wb) {
            win.push_back(dense + w0);
            win.push_back(start + w0);
            win.push_back(len - w0 < (1u << wb) ? len - w0 : (1u << wb));
        }
        dense += len;
        start = end;
    }
    h_first[nb] = n;
    h_prev[nb] = h_next[nb] = h_aux[nb] = 0;
    // (the separator ranks lie between the buckets and belong to none: the tile descriptors are written here,
    // on the host, instead of by seg_desc_kernel, whose buckets follow each other without gaps)
    const uint32_t num_tiles = h_tile0[nb];
    std::vector<uint32_t> desc((size_t)num_tiles * kSegDescWords);
    {
        uint32_t s0 = 0;
        for (uint32_t k = 0; k < nb; ++k) {
            const uint32_t len = (k + 1 < nb ? h_terms[k] : n) - s0;
            const uint32_t first = h_first[k], t0 = h_tile0[k], nt = h_tile0[k + 1] - t0;
            const uint32_t c0 = (uint32_t)kTile - first % 64u;  // elements of the first tile (see above)
            for (uint32_t local = 0; local < nt; ++local) {
                uint32_t *d = desc.data() + (size_t)(t0 + local) * kSegDescWords;
                const uint32_t f = local == 0 ? first : first + c0 + (local - 1) * (uint32_t)kTile, e = first + len;
                d[0] = f;
                const uint32_t room = local == 0 ? c0 : (uint32_t)kTile;
                d[1] = e - f < room ? e - f : room;
                d[2] = k;
                d[3] = t0 * (uint32_t)kBins + local;
                d[4] = nt;
                d[5] = first;
                d[6] = e;
                d[7] = h_prev[k];
                d[8] = h_next[k];
                d[9] = h_aux[k];
                d[10] = d[11] = 0;
            }
            s0 = k + 1 < nb ? h_terms[k] + 1 : n;
        }
    }
    uint32_t *d_desc = arena.alloc<uint32_t>(desc.size() + 4);
    uint32_t *d_win = arena.alloc<uint32_t>(win.size());
    uint32_t *d_sep = arena.alloc<uint32_t>(sep.size() + 2);
    HIP_CHECK(hipMemcpyAsync(d_desc, desc.data(), desc.size() * sizeof(uint32_t), hipMemcpyHostToDevice, stream));
    HIP_CHECK(hipMemcpyAsync(d_win, win.data(), win.size() * sizeof(uint32_t), hipMemcpyHostToDevice, stream));
    HIP_CHECK(hipMemcpyAsync(d_sep, sep.data(), sep.size() * sizeof(uint32_t), hipMemcpyHostToDevice, stream));
    HIP_CHECK(hipStreamSynchronize(stream));  // local vectors
    plan.seg.desc = d_desc;
    plan.seg.num_tiles = num_tiles;
    plan.win = d_win;
    plan.num_windows = (uint32_t)(win.size() / 3);
    plan.sep = d_sep;
    plan.num_seps = nb - 1;
    plan.n = n;
    plan.window_bits = wb;
    return true;
}

namespace {

// bits of a target position below n_out
int index_bits(uint64_t n_out) {
    int nb = 1;
    while (nb < 32 && (1ull << nb) < n_out) ++nb;
    return nb;
}
// window bits of a permutation of 2^nb targets by two partition passes: what the two digits leave, 2^10 entries at least
int window_bits_of(int nb) { return nb > 2 * kRadixBits + 10 ? nb - 2 * kRadixBits : 10; }

// out2[idx[k]] = k + 1 by a scatter of its own: small inputs and the shapes that have no two-value form
void rank_scatter(const uint32_t *idx, size_t count, uint32_t *out2, uint32_t n_out, hipStream_t stream, Profiler *prof) {
    ProfScope ps(prof, "bucket_scatter", stream, 8.0 * (double)count);
    const unsigned g = (unsigned)std::min<size_t>(div_up(count, kThreads), 256u * 16u);
    plain_rank_scatter_kernel<<<g, kThreads, 0, stream>>>(idx, count, out2, n_out);
    KERNEL_CHECK();
}

// The tail the two-value forms share (two_value_hist_form, permute_packed): the second partition pass, by the top
// digit, of pairs whose two values travel as one 64-bit word -- only the low 16 bits of an index travel on -- and the
// windows, both assembled side by side in LDS.
void pair_pass_and_windows(const uint32_t *idx_in, const uint64_t *packed_in, uint16_t *idx16, uint64_t *packed_out, size_t count,
                           int wb, uint32_t *hist, uint32_t num_tiles, uint32_t *out, uint32_t *out2, uint32_t n_out, Arena &arena,
                           hipStream_t stream, Profiler *prof) {
    radix_pass<uint32_t, uint16_t, PairSrc, uint64_t>(PairSrc{idx_in, packed_in}, idx16, packed_out, count, wb + kRadixBits, hist,
                                                      num_tiles, 4.0 * (double)count, 22.0 * (double)count, arena, stream, prof);
    ProfScope ps(prof, "window_scatter", stream, 18.0 * (double)count);
    const uint32_t W = 1u << wb;
    window_scatter2_kernel<<<(unsigned)div_up(n_out, W), kWindow2Threads, 0, stream>>>(idx16, packed_out, out, out2, n_out, wb);
    KERNEL_CHECK();
}

// The permutation with TWO values per pair, with histograms: out[idx[k]] = val[k] and out2[idx[k]] = k + 1.  The list
// position is generated by the first pass and travels along as a second value: 20 + 22 + 18 bytes per pair where two
// permutations of their own take 2 * (16 + 14 + 10) -- and, above all, the second one no longer has to exist before
// the first (suffix_array.hip: rank[] is not written at all when the direct rounds finish the suffix array).  The two
// values travel as one 64-bit word (RankSrc).  Scratch: idx[1], val[1] (2 * count words in this form) and, unless
// keep_input, idx[0].
void two_value_hist_form(uint32_t *idx[2], uint32_t *val[2], size_t count, uint32_t *out, uint32_t *out2, uint32_t n_out, int wb,
                         bool keep_input, Arena &arena, hipStream_t stream, Profiler *prof) {
    const uint32_t num_tiles = (uint32_t)div_up(count, kTile);
    uint32_t *hist = arena.alloc<uint32_t>((size_t)kBins * num_tiles);
    uint32_t *idx_b = keep_input ? arena.alloc<uint32_t>(count) : idx[0];
    uint64_t *packed1 = reinterpret_cast<uint64_t *>(val[1]);
    uint64_t *packed2 = arena.alloc<uint64_t>(count);
    radix_pass<uint32_t, uint32_t, RankSrc, uint64_t>(RankSrc{idx[0], val[0]}, idx[1], packed1, count, wb, hist, num_tiles,
                                                      4.0 * (double)count, 20.0 * (double)count, arena, stream, prof);
    pair_pass_and_windows(idx[1], packed1, reinterpret_cast<uint16_t *>(idx_b), packed2, count, wb, hist, num_tiles, out, out2,
                          n_out, arena, stream, prof);
}

// The block-diagonal permutation of a RecordScatterPlan: one pass by the window inside the record, then the windows
// and the separators.  idx[0] / val[0] survive; idx[1] / val[1] (2 * count words with out2) are the only scratch.
// false: a separator suffix is not the first of its record (the text is not what the plan was made for).
bool record_plan_form(uint32_t *idx[2], uint32_t *val[2], size_t count, uint32_t *out, uint32_t *out2, const RecordScatterPlan &plan,
                      Arena &arena, hipStream_t stream, Profiler *prof) {
    uint16_t *idx16 = reinterpret_cast<uint16_t *>(idx[1]);
    uint32_t *hist = arena.alloc<uint32_t>((size_t)kBins * plan.seg.num_tiles);
    uint32_t *err = arena.alloc<uint32_t>(1);
    HIP_CHECK(hipMemsetAsync(err, 0, sizeof(uint32_t), stream));
    // (32-bit indices out of this pass measured 10 % slower end to end than the low 16 bits)
    if (out2) {  // two values per pair, as one 64-bit word
        uint64_t *packed = reinterpret_cast<uint64_t *>(val[1]);
        radix_pass<uint32_t, uint16_t, LocalRankSrc, uint64_t>(LocalRankSrc{idx[0], val[0]}, idx16, packed, count, plan.window_bits,
                                                               hist, plan.seg.num_tiles, 4.0 * (double)count, 18.0 * (double)count,
                                                               arena, stream, prof, plan.seg);
        ProfScope ps(prof, "window_scatter", stream, 18.0 * (double)count);
        record_window_scatter2_kernel<<<plan.num_windows, kWindow2Threads, 0, stream>>>(idx16, packed, out, out2, plan.win,
                                                                                       plan.window_bits);
        KERNEL_CHECK();
    } else {
        radix_pass<uint32_t, uint16_t>(LocalIdxSrc{idx[0], val[0]}, idx16, val[1], count, plan.window_bits, hist, plan.seg.num_tiles,
                                       4.0 * (double)count, 14.0 * (double)count, arena, stream, prof, plan.seg);
        ProfScope ps(prof, "window_scatter", stream, 10.0 * (double)count);
        record_window_scatter_kernel<uint16_t><<<plan.num_windows, kThreads, 0, stream>>>(idx16, val[1], out, plan.win,
                                                                                         plan.window_bits);
        KERNEL_CHECK();
    }
    if (plan.num_seps) {
        separator_scatter_kernel<<<(unsigned)div_up(plan.num_seps, kThreads), kThreads, 0, stream>>>(plan.sep, plan.num_seps, idx[0],
                                                                                                   val[0], out, err, out2);
        KERNEL_CHECK();
    }
    uint32_t h_err = 0;
    HIP_CHECK(hipMemcpyAsync(&h_err, err, sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
    HIP_CHECK(hipStreamSynchronize(stream));
    return h_err == 0;
}

// idx is a permutation of [0, n_out): radix passes by the digits above the window bits leave window
// w = [w*W, (w+1)*W) exactly at list positions [w*W, (w+1)*W); each window is assembled in LDS and written out as full
// lines.  Two passes reach 2^30 targets; above that a third pass takes the top bits (few bins, long runs): 17 ms per
// 2^30 pairs where the windowed partial scatter needed 29.
void window_perm_form(uint32_t *idx[2], uint32_t *val[2], size_t count, uint32_t *out, uint32_t n_out, int wb, bool three,
                      bool keep_input, bool keep_val, Arena &arena, hipStream_t stream, Profiler *prof) {
    const int shifts[3] = {wb, wb + kRadixBits, wb + 2 * kRadixBits};
    // pass 1: buffer 0 -> 1; pass 2: 1 -> 0, or 1 -> a third buffer if the input must survive;
    // (pass 3: that buffer -> 1)
    radix_sort_pairs(idx, val, count, shifts, 1, arena, stream, prof);
    uint32_t *idx2[2] = {idx[1], keep_input ? arena.alloc<uint32_t>(count) : idx[0]};
    uint32_t *val2[2] = {val[1], (keep_input && keep_val) ? arena.alloc<uint32_t>(count) : val[0]};
    if (three) {
        radix_sort_pairs(idx2, val2, count, shifts + 1, 1, arena, stream, prof);
        std::swap(idx2[0], idx2[1]);
        std::swap(val2[0], val2[1]);
    }
    // last pass (top digit): only the low 16 bits of an index travel on -- the window scatter needs the
    // bits below the window size, and everything above them is the position in the list (6 instead of 8
    // bytes per pair written here and read there)
    uint16_t *idx16 = reinterpret_cast<uint16_t *>(idx2[1]);
    radix_pass_low16(idx2[0], val2[0], idx16, val2[1], count, shifts[three ? 2 : 1], arena, stream, prof);
    ProfScope ps(prof, "window_scatter", stream, 10.0 * (double)count);
    const uint32_t W = 1u << wb;
    window_scatter_kernel<uint16_t><<<(unsigned)div_up(n_out, W), kThreads, 0, stream>>>(idx16, val2[1], out, n_out, wb);
    KERNEL_CHECK();
}

// Everything else: the plain scatter -- for a large target behind a partial scatter, one or two partition passes after
// which all writes in flight fall into 2 MiB windows of the target, which one XCD's L2 can merge.  idx[1] / val[1] may be
// pointed at other buffers (the arrays are local copies of the caller's pointers).  Returns the partition passes it made.
int partial_then_plain_form(uint32_t *idx[2], uint32_t *val[2], size_t count, uint32_t *out, uint32_t n_out, int nbits, bool big,
                             bool keep_input, bool keep_val, Arena &arena, hipStream_t stream, Profiler *prof) {
    int cur = 0, passes = 0;
    const int window_bits = 19;
    if (big && nbits > window_bits) {
        int shift = window_bits;
        radix_sort_pairs(idx, val, count, &shift, 1, arena, stream, prof);
        cur = passes = 1;
        if (nbits > window_bits + kRadixBits) {
            uint32_t *idx2[2] = {idx[1], keep_input ? arena.alloc<uint32_t>(count) : idx[0]};
            uint32_t *val2[2] = {val[1], (keep_input && keep_val) ? arena.alloc<uint32_t>(count) : val[0]};
            shift = window_bits + kRadixBits;
            radix_sort_pairs(idx2, val2, count, &shift, 1, arena, stream, prof);
            idx[1] = idx2[1];
            val[1] = val2[1];
            passes = 2;
        }
    }
    ProfScope ps(prof, "bucket_scatter", stream, 12.0 * (double)count);
    const uint32_t num_tiles = (uint32_t)div_up(count, kTile);
    plain_scatter_kernel<<<xcd_grid(num_tiles), kThreads, 0, stream>>>(idx[cur], val[cur], count, out, n_out, num_tiles);
    KERNEL_CHECK();
    return passes;
}

}  // namespace

// Chooses the form; the forms allocate from the arena, which is released here.
bool bucketed_scatter(uint32_t *idx[2], uint32_t *val[2], size_t count, uint32_t *out, uint32_t n_out, Arena &arena,
                      hipStream_t stream, Profiler *prof, bool keep_input, bool keep_val, const RecordScatterPlan *plan,
                      uint32_t *out2, bool short_codes, const LstarCodes *narrow, TextOrderReport *report) {
    TextOrderReport unread;
    TextOrderReport &rep = report ? *report : unread;
    rep = TextOrderReport{};
    if (count == 0) return narrow == nullptr;
    const size_t amark = arena.mark();
    const int nbits = index_bits(n_out);
    const bool two_passes = nbits <= 2 * kRadixBits + kWindowBitsMax;  // two digits and a window cover the target
    const int wb = two_passes ? window_bits_of(nbits) : kWindowBitsMax;
    rep.nbits = nbits;
    rep.wb = wb;
    const bool big = (size_t)n_out * 4 > (size_t(64) << 20) && count > (size_t(1) << 22);
    const bool perm = big && count == n_out;  // (a permutation of the whole target: the callers' contract)
    const bool has_plan = plan && plan->seg.desc;
    const bool plan_form = has_plan && count == n_out && n_out == plan->n;
    const bool two_value = out2 && perm && two_passes && !has_plan;
    if (two_value && short_codes && !sort_knobs().text_order_hist) {
        // one 8-byte word per pair, no histograms: 16 + 16 + 16 bytes per pair; the inputs are only read, so the
        // histogram form can still run when the exception list overflows or a look-back gives up
        const bool done = packed_text_order(idx[0], val[0], count, narrow ? *narrow : LstarCodes::of(out), out2, nbits, wb,
                                            reinterpret_cast<uint64_t *>(val[1]), arena, stream, prof, rep);
        arena.rewind(amark);
        if (done) {
            rep.form = TextOrderForm::kPacked;
            return true;
        }
    }
    if (narrow) return false;  // (no other form writes 16-bit codes)
    bool separators_ok = true;
    if (two_value) {
        two_value_hist_form(idx, val, count, out, out2, n_out, wb, keep_input, arena, stream, prof);
        rep.form = TextOrderForm::kTwoValueHist;
    } else {
        if (out2 && !plan_form) rank_scatter(idx[0], count, out2, n_out, stream, prof);
        if (plan_form) {
            separators_ok = record_plan_form(idx, val, count, out, out2, *plan, arena, stream, prof);
            rep.form = out2 ? TextOrderForm::kRecordPlan2 : TextOrderForm::kRecordPlan;
            rep.wb = plan->window_bits;
        } else if (perm) {
            window_perm_form(idx, val, count, out, n_out, wb, !two_passes, keep_input, keep_val, arena, stream, prof);
            rep.form = TextOrderForm::kWindowPerm;
        } else {
            rep.partition_passes = partial_then_plain_form(idx, val, count, out, n_out, nbits, big, keep_input, keep_val, arena,
                                                           stream, prof);
            rep.form = rep.partition_passes ? TextOrderForm::kPartialThenPlain : TextOrderForm::kPlain;
        }
    }
    arena.rewind(amark);
    if (!separators_ok) throw HipError("record scatter: a separator suffix is not the first of its record");
    return true;
}

bool packed_text_order_applies(size_t count, bool has_plan) {
    const int nbits = index_bits(count);
    return count > (size_t(1) << 24) && nbits <= 2 * kRadixBits + kWindowBitsMax && !has_plan && !sort_knobs().text_order_hist;
}

void permute_packed(uint32_t *idx, uint64_t *packed, size_t count, uint32_t *out, uint32_t *out2, Arena &arena,
                    hipStream_t stream, Profiler *prof, TextOrderReport *report) {
    TextOrderReport unread;
    TextOrderReport &rep = report ? *report : unread;
    rep = TextOrderReport{};
    if (count == 0) return;
    const int nb = index_bits(count);
    rep.nbits = nb;
    rep.wb = window_bits_of(nb);
    rep.form = TextOrderForm::kPermuteWindows;
    if (count <= (size_t(1) << 22) || nb > 2 * kRadixBits + kWindowBitsMax) {
        rep.form = TextOrderForm::kPermutePlain;
        ProfScope ps(prof, "bucket_scatter", stream, 20.0 * (double)count);
        const unsigned g = (unsigned)std::min<size_t>(div_up(count, kThreads), 256u * 16u);
        plain_packed_scatter_kernel<<<g, kThreads, 0, stream>>>(idx, packed, count, out, out2);
        KERNEL_CHECK();
        return;
    }
    // two partition passes by the digits above the window bits, then the windows: the first pass here, the rest as in
    // the two-value form of bucketed_scatter
    const size_t amark = arena.mark();
    const int wb = window_bits_of(nb);
    const uint32_t num_tiles = (uint32_t)div_up(count, kTile);
    uint32_t *hist = arena.alloc<uint32_t>((size_t)kBins * num_tiles);
    uint32_t *idx_b = arena.alloc<uint32_t>(count);
    uint64_t *packed_b = arena.alloc<uint64_t>(count);
    radix_pass<uint32_t, uint32_t, PairSrc, uint64_t>(PairSrc{idx, packed}, idx_b, packed_b, count, wb, hist, num_tiles,
                                                      4.0 * (double)count, 24.0 * (double)count, arena, stream, prof);
    // (the inputs are free now)
    pair_pass_and_windows(idx_b, packed_b, reinterpret_cast<uint16_t *>(idx), packed, count, wb, hist, num_tiles, out, out2,
                          (uint32_t)count, arena, stream, prof);
    arena.rewind(amark);
}

}  // namespace nolzss
