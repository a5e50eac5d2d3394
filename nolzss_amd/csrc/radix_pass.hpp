// radix_pass.hpp -- one pass of the stable LSD radix sort for gfx950.  Internal to radix_sort.hip (the sorts) and
// text_order.hip (the permutation into text order), each of which instantiates it with its OWN sources only: the kernels
// have internal linkage, an instantiation made in both files would be compiled twice (radix_sort.hpp, radix_pass_low16).
//
// One pass = three launches:
//   rs_hist_kernel     per 4096-key tile, a 256-bin digit histogram (LDS atomics) written
//                      bin-major, so one linear exclusive scan yields every (bin, tile) base;
//   scan               exclusive add-scan of the 256 x num_tiles table (scan.hip);
//   rs_scatter_kernel  loads the whole tile (all loads in flight before anything else), ranks
//                      every key inside its wavefront -- 8 ballots give the lanes with the same
//                      digit, the first lane of each digit group does one returning LDS atomic on
//                      the wave's counter, the atomics of all 16 rows are issued back to back --
//                      sorts the tile by digit through LDS, and writes each bin's run with
//                      consecutive lanes on consecutive addresses.
// The pairs of a pass come from a SOURCE: arrays (ArraySrc, here), the packed text (radix_sort.hip) or the pair
// lists of a permutation (text_order.hip); passes can be SEGMENTED: tiles that never straddle the buckets of a
// SegView (radix_sort.hpp).
// HBM-bound: algorithmic traffic of the scatter kernel = 2 * (sizeof(key) + 4) bytes per pair;
// the histogram kernel reads sizeof(key) bytes per pair.  4.0-4.8 TB/s on MI355X (u32 keys).
//
// Occupancy is what the scatter kernel lives on: keys and values take turns in ONE LDS staging
// buffer (37 KiB per workgroup).  Tiles are dealt to XCDs in contiguous ranges (blockIdx % 8
// shares an XCD) so that the bin runs of neighbouring tiles, adjacent in the output, meet in one
// L2 and their partial cache lines merge there: without it the scatter runs at HALF the speed.
#pragma once
#include "radix_sort.hpp"
#include "scan.hpp"

#include <cstdio>
#include <type_traits>

namespace nolzss {
namespace {

constexpr int kKeysPerThread = 16;  // 12 and 8 measured within 3 % of this on MI355X
constexpr int kTile = kSortTile;    // part of the SegView contract
constexpr int kThreads = kTile / kKeysPerThread;  // 256 (4096-pair tiles) or 512 (8192)
constexpr int kWaves = kThreads / 64;
constexpr int kBins = 1 << kRadixBits;
constexpr int kWaveSpan = 64 * kKeysPerThread;  // 1024 keys per wavefront, 16 rows of 64
// blocks per CU the scatter kernel is compiled for: 3 x 256 or 2 x 512 threads (128 VGPRs at most for the latter)
#ifndef NOLZSS_SCATTER_BLOCKS
#define NOLZSS_SCATTER_BLOCKS 1
#endif
constexpr int kScatterWavesPerSimd = kThreads == 256 ? NOLZSS_SCATTER_BLOCKS : 4;  // (1 = no register cap: the 256-thread form as it always was)

static_assert(kThreads % kBins == 0, "the first kBins threads own one bin each in the offset phase");

// 8-bit digit of a key at a bit offset that is a multiple of 8: the digit never straddles the two
// halves of a 64-bit key, so one v_bfe_u32 on the right half does it (a variable 64-bit shift costs
// several instructions, three times per key)
__device__ __forceinline__ uint32_t digit_of(uint64_t k, int shift) {
    const uint32_t half = shift >= 32 ? (uint32_t)(k >> 32) : (uint32_t)k;
    return (half >> (shift & 31)) & (uint32_t)(kBins - 1);
}
__device__ __forceinline__ uint32_t digit_of(uint32_t k, int shift) { return (k >> shift) & (uint32_t)(kBins - 1); }

// block -> tile.  Blocks b, b + 8, b + 16, .. share an XCD (round-robin dispatch); an XCD takes CHUNKS of
// kXcdChunk consecutive tiles, chunk c going to XCD c % 8: neighbouring tiles of a chunk meet in one L2 (their
// bin runs are adjacent in the output and merge there into full lines), and the eight write fronts of a bin --
// one per XCD -- stay within a few chunks of each other instead of an eighth of the array apart
// (8 / 32 / 64 / 256 / 1024 tiles per chunk: 36.1 / 33.9 / 34.1 / 34.3 / 34.1 ms for the eight large u32 passes,
// 35.2 with one contiguous range per XCD).
#ifndef NOLZSS_XCD_CHUNK
#define NOLZSS_XCD_CHUNK 64
#endif
constexpr uint32_t kXcdChunk = NOLZSS_XCD_CHUNK;
__device__ __forceinline__ uint32_t xcd_tile(uint32_t b, uint32_t num_tiles) {
    const uint32_t x = b % 8, k = b / 8;           // k-th block of XCD x
    const uint32_t chunk = (k / kXcdChunk) * 8 + x;  // chunks of this XCD: x, x + 8, x + 16, ..
    const uint32_t tile = chunk * kXcdChunk + k % kXcdChunk;
    return tile < num_tiles ? tile : 0xffffffffu;
}
// blocks to launch so that every tile is covered by the mapping above
inline uint32_t xcd_grid(uint32_t num_tiles) {
    const uint32_t chunks = (uint32_t)div_up(num_tiles, kXcdChunk);
    return (uint32_t)div_up(chunks, 8) * 8 * kXcdChunk;
}

// where a pass reads its pairs from: arrays, or (first pass of the suffix sort) the packed text.
// Every source splits a key into load() -- nothing but the loads -- and key_of() / hist_digit_of() -- the
// arithmetic: the kernels issue the loads of a whole tile first.  (With the arithmetic inside the load loop
// the compiler waited for every load on its own, `s_waitcnt vmcnt(0)` sixteen times per thread: the passes
// that compute their keys ran 1.4 x slower than the passes that only read them.)
// kFromText says which of the two a source is: it names the profiler class of the pass (radix_pass).
template <typename KeyT> struct ArraySrc {
    using Raw = KeyT;
    static constexpr bool kFromText = false;
    const KeyT *__restrict__ keys;
    const uint32_t *__restrict__ vals;
    __device__ __forceinline__ Raw load(size_t idx, const TileExtent &) const { return keys[idx]; }
    __device__ __forceinline__ KeyT key_of(Raw raw, size_t, const TileExtent &) const { return raw; }
    __device__ __forceinline__ uint32_t hist_digit_of(Raw raw, size_t, int shift, const TileExtent &) const { return digit_of(raw, shift); }
    __device__ __forceinline__ uint32_t val(size_t idx) const { return vals[idx]; }
    __device__ __forceinline__ bool digits_from_window(int) const { return false; }
    __device__ __forceinline__ uint64_t window(size_t) const { return 0; }
};

template <typename S, typename = void> struct HasWindowDigits : std::false_type {};
template <typename S> struct HasWindowDigits<S, std::void_t<decltype(&S::window_digit)>> : std::true_type {};

template <typename KeyT, typename Src>
__global__ __launch_bounds__(kThreads) void rs_hist_kernel(Src src, size_t n, int shift,
                                                           uint32_t *__restrict__ tile_hist,
                                                           uint32_t num_tiles, SegView seg) {
    // four interleaved copies of the histogram, one per lane & 3: a pass whose digit takes only a few
    // values (the lowest key byte is mostly the length tag) would otherwise send all 64 lanes of an
    // LDS atomic to the same few addresses, which the LDS executes one after the other
    constexpr int kCopies = 4;
    __shared__ __align__(16) uint32_t hist[kBins * kCopies];
    for (int i = threadIdx.x; i < kBins * kCopies; i += kThreads) hist[i] = 0;
    // XCD-contiguous tile ranges, as in the scatter kernel: the table is bin-major, so the 256 counts of a
    // tile go to 256 different lines, each shared with the 15 neighbouring tiles -- written from one XCD
    // those 4-byte writes merge in its L2; dealt round-robin over the XCDs every one of them reached HBM
    // as a partial line (67 M of them per pass at 2^30 keys): 11.7 -> 8.6 ms per step for all histograms.
    const uint32_t tile = xcd_tile(blockIdx.x, num_tiles);
    if (tile == 0xffffffffu) return;
    __syncthreads();
    const TileExtent ext = tile_extent(tile, n, num_tiles, seg);
    const uint32_t copy = threadIdx.x & (kCopies - 1);
    bool windowed = false;
    if constexpr (HasWindowDigits<Src>::value) {
        if (src.digits_from_window(shift)) {
            static_assert(kKeysPerThread == 16, "16 two-bit symbols and an 8-bit digit fit one 64-bit window");
            windowed = true;
            const uint32_t local0 = threadIdx.x * (uint32_t)kKeysPerThread;
            const uint64_t w = local0 < ext.count ? src.window(ext.first + local0) : 0ull;
#pragma unroll
            for (int j = 0; j < kKeysPerThread; ++j)
                if (local0 + (uint32_t)j < ext.count)
                    atomicAdd(&hist[src.window_digit(w, j, ext.first + local0) * kCopies + copy], 1u);
        }
    }
    if (!windowed) {
        // all loads first: the compiler does not move loads across the LDS atomics (elements past the end of
        // the tile load its first element again: no branch around a load, nothing waits in between)
        typename Src::Raw k[kKeysPerThread];
#pragma unroll
        for (int j = 0; j < kKeysPerThread; ++j) {
            const uint32_t local = (uint32_t)j * kThreads + threadIdx.x;
            k[j] = src.load(ext.first + (local < ext.count ? local : 0u), ext);
        }
#pragma unroll
        for (int j = 0; j < kKeysPerThread; ++j) {
            const uint32_t local = (uint32_t)j * kThreads + threadIdx.x;
            if (local < ext.count)
                atomicAdd(&hist[src.hist_digit_of(k[j], ext.first + local, shift, ext) * kCopies + copy], 1u);
        }
    }
    __syncthreads();
    if (threadIdx.x < kBins) {
        const uint4 c4 = reinterpret_cast<const uint4 *>(hist)[threadIdx.x];
        tile_hist[ext.hist0 + (size_t)threadIdx.x * ext.hstride] = c4.x + c4.y + c4.z + c4.w;
    }
}

// (kTimed, NOLZSS_SCATTER_PHASES: cycles per phase of a workgroup, summed over every 64th workgroup by its first thread;
// the timed instantiation waits for its loads before it ranks so that the two can be told apart.  Round 4, a segmented
// u32 pass at 2^30 pairs, 28.8 k cycles = 12 us per workgroup of which: start-up, descriptor, counters zeroed 2.0 k; the
// 32 loads ISSUED 5.6 k (the memory pipe takes them at its own pace; they have arrived when the last one is out);
// ranking 6.9 k; offsets 3.2 k (half of it the gather of the tile's 256 base offsets); keys staged 1.2 k, stored 3.8 k;
// values staged 0.7 k, stored 2.4 k, drained 2.9 k.  Half memory phases throttled by back-pressure, half compute: nothing
// to shave off one without the other growing -- asking for the base offsets first made the first key wait behind a
// gather of 256 lines (+2.7 ms per step), barriers that wait for the LDS only between the two stagings let key and
// value stores overlap and cost 1 ms, a software-pipelined form with the next tile's loads in flight needs 211 VGPRs
// (two workgroups per CU: 33.6 instead of 23.4 ms): profiles/r04_ab/scatter_phases_and_variants.txt.)
// (One returning LDS atomic per key instead of the ballots -- what local_sort_kernel does -- loses here: the u32 passes
// 5.2 -> 6.2 ms each at 2^30 pairs, three workgroups per CU already hide the ballots' VALU work behind each other's
// memory phases while the conflicting atomics queue up in the one LDS; only the pass that makes its keys from the text
// gained, 4.8 -> 4.45 ms.  gpurun_out/r4_satom, profiles/r04_ab/local_sort.txt.)
template <typename KeyT, typename OutT, typename Src, typename ValT = uint32_t, bool kTimed = false>
__global__ __launch_bounds__(kThreads, kScatterWavesPerSimd) void rs_scatter_kernel(
    Src src, OutT *__restrict__ keys_out, ValT *__restrict__ vals_out, size_t n, int shift,
    const uint32_t *__restrict__ tile_base, uint32_t num_tiles, SegView seg, unsigned long long *__restrict__ phases = nullptr) {
    const bool timed = kTimed && phases != nullptr && (blockIdx.x & 63) == 0 && threadIdx.x == 0;
    unsigned long long ck[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    if (kTimed && timed) ck[0] = __builtin_readcyclecounter();
    const uint32_t tile = xcd_tile(blockIdx.x, num_tiles);
    if (tile == 0xffffffffu) return;
    const TileExtent ext = tile_extent(tile, n, num_tiles, seg);
    // keys, then values, take turns here
    __shared__ __align__(16) unsigned char s_stage[(size_t)kTile * (sizeof(KeyT) > sizeof(ValT) ? sizeof(KeyT) : sizeof(ValT))];
    KeyT *s_keys = reinterpret_cast<KeyT *>(s_stage);
    ValT *s_vals = reinterpret_cast<ValT *>(s_stage);
    __shared__ uint32_t s_whist[kWaves * kBins];
    __shared__ uint32_t s_glob[kBins];
    __shared__ uint32_t s_scan[kWaves];

    const int tid = threadIdx.x;
    const int w = tid >> 6;
    const int lane = tid & 63;

    for (int i = tid; i < kWaves * kBins; i += kThreads) s_whist[i] = 0;
    __syncthreads();
    if (kTimed && timed) ck[1] = __builtin_readcyclecounter();  // (includes the descriptor load: ext is used above)

    const size_t base = ext.first;
    KeyT key[kKeysPerThread];
    ValT val[kKeysPerThread];
    uint32_t lrank[kKeysPerThread];

    // all loads of the tile go out before anything is ranked (the ranking below goes through
    // volatile LDS counters, which the compiler will not move loads across: interleaved, every row
    // would wait for its own round trip to HBM)
    // (a source that computes its keys keeps eight raw elements in flight at a time: sixteen would not fit
    // the registers next to the keys)
    constexpr int kBatch = sizeof(typename Src::Raw) > sizeof(KeyT) ? 8 : kKeysPerThread;
#pragma unroll
    for (int r0 = 0; r0 < kKeysPerThread; r0 += kBatch) {
        typename Src::Raw raw[kBatch];
#pragma unroll
        for (int r = 0; r < kBatch; ++r) {
            const uint32_t local = (uint32_t)w * kWaveSpan + (uint32_t)(r0 + r) * 64 + lane;
            raw[r] = src.load(base + (local < ext.count ? local : 0u), ext);  // (past the end: the first element again)
        }
#pragma unroll
        for (int r = 0; r < kBatch; ++r) {
            const uint32_t local = (uint32_t)w * kWaveSpan + (uint32_t)(r0 + r) * 64 + lane;
            const bool valid = local < ext.count;
            key[r0 + r] = valid ? (KeyT)src.key_of(raw[r], base + local, ext) : KeyT(0);
        }
    }
#pragma unroll
    for (int row = 0; row < kKeysPerThread; ++row) {
        const uint32_t local = (uint32_t)w * kWaveSpan + (uint32_t)row * 64 + lane;
        val[row] = local < ext.count ? src.val(base + local) : 0;
    }
    if constexpr (kTimed) {
        if (timed) ck[2] = __builtin_readcyclecounter();  // loads issued
        __builtin_amdgcn_s_waitcnt(0x0f70);                // vmcnt(0): the whole tile has arrived
        if (timed) ck[3] = __builtin_readcyclecounter();
    }
    // rank inside the wavefront: rows of 64 keys in input order (keeps the sort stable).  The lowest
    // lane of every digit group adds the group's size to the wave's counter with ONE returning LDS
    // atomic per row; the atomics of all rows are issued back to back (LDS executes a wave's
    // operations in order, so row r sees rows < r) and the results are handed to the other lanes
    // of the groups afterwards -- no row waits for the LDS round trip of the row in front.
    // lrank[row] packs, until the second loop: counter value seen by the group's first lane (11 bits,
    // <= 1024 keys per wave) | lanes of my group below me << 11 | lane of the first member << 17
    uint32_t *wcount = s_whist + w * kBins;
#pragma unroll
    for (int row = 0; row < kKeysPerThread; ++row) {
        const bool valid = (uint32_t)w * kWaveSpan + (uint32_t)row * 64 + lane < ext.count;
        const uint32_t d = digit_of(key[row], shift);
        // lanes with the same digit: the complement of the lanes that differ in some bit.  Per bit,
        // m = 0 / ~0 (bit clear / set, one v_bfe_i32), and (ballot ^ m) is the set of lanes whose bit
        // differs from mine -- six VALU instructions per bit instead of nine for the select form.
        uint32_t diff_lo = 0, diff_hi = 0;
#pragma unroll
        for (int b = 0; b < kRadixBits; ++b) {
            const uint32_t m = (uint32_t)__builtin_amdgcn_sbfe((int)d, (unsigned)b, 1u);
            const uint64_t bal = __ballot((int)m < 0);
            // diff |= bal ^ m in one v_bitop3 (truth table 0xde = b | (c ^ a)): four VALU per bit and row
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
    if (kTimed && timed) ck[4] = __builtin_readcyclecounter();  // ranked
    __syncthreads();

    // thread = bin (the first kBins threads): turn per-wave counts into tile-local start positions
    {
        const int d = tid;
        const bool owner = tid < kBins;
        uint32_t c[kWaves], total = 0;
#pragma unroll
        for (int k = 0; k < kWaves; ++k) {
            c[k] = owner ? s_whist[k * kBins + d] : 0u;
            total += c[k];
        }
        uint32_t tile_total;
        const uint32_t bin_start = block_scan_exclusive<kWaves>(total, OpAdd<uint32_t>(), s_scan, tile_total);
        if (owner) {
            uint32_t run = bin_start;
#pragma unroll
            for (int k = 0; k < kWaves; ++k) {
                s_whist[k * kBins + d] = run;
                run += c[k];
            }
            s_glob[d] = tile_base[ext.hist0 + (size_t)d * ext.hstride] - bin_start;
        }
    }
    __syncthreads();
    if (kTimed && timed) ck[5] = __builtin_readcyclecounter();  // tile-local offsets (and the tile's bases from the table)

    // tile-local sorted position of every element (reuses lrank)
#pragma unroll
    for (int row = 0; row < kKeysPerThread; ++row) {
        const uint32_t d = digit_of(key[row], shift);
        lrank[row] += s_whist[w * kBins + d];
    }
#pragma unroll
    for (int row = 0; row < kKeysPerThread; ++row) {
        if ((uint32_t)w * kWaveSpan + (uint32_t)row * 64 + lane < ext.count) s_keys[lrank[row]] = key[row];
    }
    __syncthreads();
    if (kTimed && timed) ck[6] = __builtin_readcyclecounter();  // keys staged

    const uint32_t count = ext.count;
    uint32_t gpos[kKeysPerThread];
#pragma unroll
    for (int j = 0; j < kKeysPerThread; ++j) {
        const uint32_t p = (uint32_t)j * kThreads + tid;
        if (p < count) {
            const KeyT k = s_keys[p];
            const uint32_t d = digit_of(k, shift);
            gpos[j] = s_glob[d] + p;
            keys_out[gpos[j]] = (OutT)k;
        }
    }
    __syncthreads();
    if (kTimed && timed) ck[7] = __builtin_readcyclecounter();  // key stores issued (and, through the barrier, drained)
#pragma unroll
    for (int row = 0; row < kKeysPerThread; ++row) {
        if ((uint32_t)w * kWaveSpan + (uint32_t)row * 64 + lane < ext.count) s_vals[lrank[row]] = val[row];
    }
    __syncthreads();
    if (kTimed && timed) ck[8] = __builtin_readcyclecounter();  // values staged
#pragma unroll
    for (int j = 0; j < kKeysPerThread; ++j) {
        const uint32_t p = (uint32_t)j * kThreads + tid;
        if (p < count) vals_out[gpos[j]] = s_vals[p];
    }
    if constexpr (kTimed) {
        if (timed) {
            ck[9] = __builtin_readcyclecounter();  // value stores issued
            for (int k = 0; k < 9; ++k) atomicAdd(phases + k, ck[k + 1] - ck[k]);
            __builtin_amdgcn_s_waitcnt(0x0f70);
            atomicAdd(phases + 9, (unsigned long long)__builtin_readcyclecounter() - ck[9]);  // value stores drained
            atomicAdd(phases + 10, 1ull);
        }
    }
}

// the first two launches of a pass: the tile histograms of the digit at `shift`, and their scan
template <typename KeyT, typename Src>
void hist_and_scan(Src src, size_t n, int shift, uint32_t *hist, uint32_t num_tiles, double hist_bytes, Arena &arena,
                   hipStream_t stream, Profiler *prof, const SegView &seg) {
    {
        ProfScope ps(prof, "rs_hist", stream, hist_bytes);
        rs_hist_kernel<KeyT, Src><<<xcd_grid(num_tiles), kThreads, 0, stream>>>(src, n, shift, hist, num_tiles, seg);
        KERNEL_CHECK();
    }
    ProfScope ps(prof, "rs_scan", stream, 8.0 * (double)kBins * num_tiles);
    scan_exclusive_add_u32(hist, hist, (size_t)kBins * num_tiles, nullptr, arena, stream);
}

// one pass: histogram, scan, scatter
template <typename KeyT, typename OutT, typename Src, typename ValT = uint32_t>
void radix_pass(Src src, OutT *keys_out, ValT *vals_out, size_t n, int shift, uint32_t *hist, uint32_t num_tiles,
                double hist_bytes, double scatter_bytes, Arena &arena, hipStream_t stream, Profiler *prof,
                const SegView &seg = SegView{}) {
    hist_and_scan<KeyT>(src, n, shift, hist, num_tiles, hist_bytes, arena, stream, prof, seg);
    {
        // classes of launches, so that the bandwidth of the large passes can be told from the many
        // small sorts of the doubling rounds: rs_scatter.{text|u64|u32}[.small]
        const bool small = n < (size_t(1) << 24);
        const char *cls = Src::kFromText ? "rs_scatter.text"
                          : sizeof(KeyT) == 8 ? (small ? "rs_scatter.u64.small" : "rs_scatter.u64")
                                              : (small ? "rs_scatter.u32.small" : "rs_scatter.u32");
        ProfScope ps(prof, cls, stream, scatter_bytes);
        // (Round 3, NOLZSS_SORT_TILE=8192: tiles of 8192 pairs on 512 threads -- bin runs of a full 128-byte line.  The
        // kernel needs 134 VGPRs and two such workgroups per CU allow 128: 14 registers spilled (72 in the text
        // pass); u32 passes 3857 -> 3017 GB/s, text pass 1811 -> 1314, histograms + scans 10.8 -> 9.0 ms per step,
        // step 118.7 -> 129.3 ms, profiles/r03_ab_tile8k.txt.  4096 stays.)
        // (Round 2 tried 512 threads with 8 keys each -- 75 instead of 139 VGPRs, 24 instead of 12 wavefronts
        // per CU -- and separate LDS buffers for keys and values: the u32 passes stayed at 3.9 TB/s at 2^30
        // pairs either way.  The pass is bound by its scattered 64-byte write runs, not by latency hiding.)
        const uint32_t grid = xcd_grid(num_tiles);
        if (sort_knobs().scatter_phases && n >= (size_t(1) << 24) && std::is_same<Src, ArraySrc<KeyT>>::value) {
            unsigned long long *d_ph = arena.alloc<unsigned long long>(12);
            HIP_CHECK(hipMemsetAsync(d_ph, 0, 12 * sizeof(unsigned long long), stream));
            rs_scatter_kernel<KeyT, OutT, Src, ValT, true><<<grid, kThreads, 0, stream>>>(src, keys_out, vals_out, n, shift, hist,
                                                                                          num_tiles, seg, d_ph);
            KERNEL_CHECK();
            unsigned long long h[12];
            HIP_CHECK(hipMemcpyAsync(h, d_ph, sizeof(h), hipMemcpyDeviceToHost, stream));
            HIP_CHECK(hipStreamSynchronize(stream));
            const double wn = h[10] ? (double)h[10] : 1.0;
            fprintf(stderr, "[nolzss] rs_scatter phases (cycles per workgroup, %llu sampled, shift %d, %s): start-up + descriptor + zero %.0f  "
                            "loads issued %.0f  loads arrive %.0f  ranking %.0f  offsets %.0f  stage keys %.0f  store keys %.0f  stage values %.0f  "
                            "store values %.0f  drain %.0f\n",
                    h[10], shift, seg.desc ? "segmented" : "whole array", h[0] / wn, h[1] / wn, h[2] / wn, h[3] / wn, h[4] / wn, h[5] / wn,
                    h[6] / wn, h[7] / wn, h[8] / wn, h[9] / wn);
        } else {
            rs_scatter_kernel<KeyT, OutT, Src, ValT><<<grid, kThreads, 0, stream>>>(src, keys_out, vals_out, n, shift, hist,
                                                                                    num_tiles, seg);
            KERNEL_CHECK();
        }
    }
}

}  // namespace
}  // namespace nolzss
