// radix_sort.hip -- the sorts built on the radix pass of radix_pass.hpp (stable, least significant digit first, 8-bit
// digits, (u64 or u32 key, u32 value) pairs), for gfx950:
//   * radix_sort_pairs, and radix_pass_low16 for the window permutation of text_order.hip;
//   * the round-0 key sorts of the suffix array, whose first pass computes its pairs from the packed text (TextSrc,
//     Text16Src, Text35Src, Text16SegSrc, RecordTextSrc): radix_sort_initial_keys, radix_sort_dna_keys, radix_sort_dna_keys16 (and
//     its fused-record A/B variant, rs_scatter_rec_kernel), radix_sort_record_keys;
//   * radix_sort_segments_u32.
// The bucketed sorts run SEGMENTED passes -- tiles that never straddle the buckets of an earlier most-significant-digit
// pass, or of the caller (radix_sort.hpp, SegView; seg_view_of makes it) -- which is how plain DNA is sorted on 8-byte
// records; sub-buckets small enough are finished in LDS (local_sort.hpp).  The knobs, also of text_order.hip: SortKnobs.
// One translation unit: two key sorts share rs_hist_kernel<uint64_t, TextSrc<2>>, everything else the u32 array kernels.
#include "radix_sort.hpp"

#include "local_sort.hpp"
#include "radix_pass.hpp"

#include <cstdlib>

namespace nolzss {

SortKnobs::SortKnobs() {
    auto set = [](const char *name) { return getenv(name) != nullptr; };
    auto i64 = [](const char *name, long long dflt) { return getenv(name) ? atoll(getenv(name)) : dflt; };
    trace = set("NOLZSS_TRACE");
    scatter_phases = set("NOLZSS_SCATTER_PHASES");
    no_local_sort = set("NOLZSS_NO_LOCAL_SORT");
    local_sort_min_set = set("NOLZSS_LOCAL_SORT_MIN");
    local_sort_min = (size_t)i64("NOLZSS_LOCAL_SORT_MIN", 0);
    no_local_regroup = set("NOLZSS_NO_LOCAL_REGROUP");
    no_key35 = set("NOLZSS_NO_KEY35");
    local_regroup_min = (size_t)i64("NOLZSS_LOCAL_REGROUP_MIN", 3ll << 28);
    test_local_order_fails = set("NOLZSS_TEST_LOCAL_ORDER_FAILS");
    test_local_lookback_fails = set("NOLZSS_TEST_LOCAL_LOOKBACK_FAILS");
    rec_bucket_min = (uint64_t)i64("NOLZSS_REC_BUCKET_MIN", 1ll << 16);
    text_order_hist = set("NOLZSS_TEXT_ORDER_HIST");
    const char *esc = getenv("NOLZSS_TEXT_ORDER_ESC");
    text_order_esc = esc ? (long long)strtoul(esc, nullptr, 0) : -1;
    no_code16 = set("NOLZSS_NO_CODE16");
    const long long c16 = i64("NOLZSS_CODE16_MAX", 0xffff);
    code16_max = (uint32_t)(c16 < 1 ? 1 : (c16 > 0xffff ? 0xffff : c16));
}

const SortKnobs &sort_knobs() {
    static const SortKnobs k;
    return k;
}

namespace {

template <int BITS> struct TextSrc {
    using Raw = SymWords;
    static constexpr bool kFromText = true;
    const uint64_t *__restrict__ words;
    TermTable terms;
    bool segmented;
    bool digit_from_text = true;  // MSD histogram digit straight from the packed text (no terminators in the text)
    __device__ __forceinline__ Raw load(size_t idx, const TileExtent &) const { return sym_words<BITS>(words, idx); }
    __device__ __forceinline__ uint64_t key_of(const Raw &raw, size_t idx, const TileExtent &) const {
        return initial_key_of<BITS>(sym_word_of<BITS>(raw, idx), terms, segmented, (uint32_t)idx);
    }
    __device__ __forceinline__ uint32_t val(size_t idx) const { return (uint32_t)idx; }
    // histogram passes only need the digit; the top 8 bits of a plain key are the first 8 / BITS
    // symbols, straight from the packed text (no length tag, no terminator search)
    __device__ __forceinline__ uint32_t hist_digit_of(const Raw &raw, size_t idx, int shift, const TileExtent &ext) const {
        constexpr int kKeyBits = KeyLayout<BITS>::kSyms * BITS + KeyLayout<BITS>::kTagBits;
        if (!segmented && digit_from_text && shift == kKeyBits - kRadixBits)
            return digit_of(sym_word_of<BITS>(raw, idx) >> (64 - kKeyBits), shift);
        return digit_of(key_of(raw, idx, ext), shift);
    }
    // the most significant digits of 16 CONSECUTIVE suffixes are 8-bit windows of one 64-bit piece of a
    // 2-bit text: a histogram thread can take 16 neighbours with two loads instead of 16 strided
    // elements with 32
    __device__ __forceinline__ bool digits_from_window(int shift) const {
        constexpr int kKeyBits = KeyLayout<BITS>::kSyms * BITS + KeyLayout<BITS>::kTagBits;
        return BITS == 2 && !segmented && digit_from_text && shift == kKeyBits - kRadixBits;
    }
    __device__ __forceinline__ uint64_t window(size_t idx) const { return sym_word<BITS>(words, idx); }
    // digit of the j-th of the 16 suffixes that start in the window fetched for element idx0
    __device__ __forceinline__ uint32_t window_digit(uint64_t w, int j, size_t) const {
        return (uint32_t)((w >> (64 - kRadixBits - 2 * j)) & (uint64_t)(kBins - 1));
    }
};
// Plain one-segment 2-bit DNA with the 16-base key of text.hpp (kP16Syms): the most-significant-digit pass.  The
// 40-bit value it hands to the kernels is [32 key bits][8-bit tag]: the digit of this pass (shift 32) is the first
// four bases, and the low 32 bits -- what the pass stores -- are [24 key bits][tag].  Element e of the pass is
// suffix n - 1 - e for e < 16 and suffix e - 16 behind them: the suffixes that end inside the key window come
// first, shortest first, and the stable passes leave them in front of the longer suffixes that tie with their
// zero-padded keys (the packed text is zero behind its end: no masking).
struct Text16Src {
    using Raw = SymWords;
    static constexpr bool kFromText = true;
    const uint64_t *__restrict__ words;
    uint32_t n;  // >= 32
    __device__ __forceinline__ uint32_t suffix_of(size_t idx) const {
        return idx < 16 ? n - 1u - (uint32_t)idx : (uint32_t)idx - 16u;
    }
    __device__ __forceinline__ Raw load(size_t idx, const TileExtent &) const { return sym_words<2>(words, suffix_of(idx)); }
    __device__ __forceinline__ uint64_t key_of(const Raw &raw, size_t idx, const TileExtent &) const {
        const uint32_t s = suffix_of(idx);
        const uint32_t lim = n - s;
        const uint32_t tag = lim < (uint32_t)kP16Syms ? lim : (uint32_t)kP16Syms;
        return ((sym_word_of<2>(raw, s) >> 32) << kP16TagBits) | tag;
    }
    __device__ __forceinline__ uint32_t val(size_t idx) const { return suffix_of(idx); }
    __device__ __forceinline__ uint32_t hist_digit_of(const Raw &raw, size_t idx, int, const TileExtent &) const {
        return (uint32_t)(sym_word_of<2>(raw, suffix_of(idx)) >> (64 - kRadixBits));
    }
    // (tiles start at multiples of 16 elements: only the very first window of the list holds the rotated suffixes;
    // it is the window of suffix n - 16, read backwards)
    __device__ __forceinline__ bool digits_from_window(int) const { return true; }
    __device__ __forceinline__ uint64_t window(size_t idx0) const { return sym_word<2>(words, idx0 == 0 ? (uint64_t)n - 16u : idx0 - 16u); }
    __device__ __forceinline__ uint32_t window_digit(uint64_t w, int j, size_t idx0) const {
        const int jj = idx0 == 0 ? 15 - j : j;
        return (uint32_t)((w >> (64 - kRadixBits - 2 * jj)) & (uint64_t)(kBins - 1));
    }
};
// The same pass with the 35-bit key of text.hpp (kP35Syms): the value handed to the kernels is [35 key bits][5-bit tag],
// its digit (shift 32) the first four bases as before, the stored low 32 bits [27 key bits][tag].  The elements and their
// order are Text16Src's: the suffixes that are short here (tag < 17) are the 16 it takes first.
struct Text35Src : Text16Src {
    __device__ __forceinline__ uint64_t key_of(const Raw &raw, size_t idx, const TileExtent &) const {
        const uint32_t s = suffix_of(idx);
        const uint32_t lim = n - s;
        const uint32_t tag = lim < (uint32_t)kP35Syms ? lim : (uint32_t)kP35Syms;
        return ((sym_word_of<2>(raw, s) >> (64 - kP35KeyBits)) << kP35TagBits) | tag;
    }
};
// The same pass for a SEGMENTED text with a short terminator table (at most kTermFew entries: a prepared reverse-
// complement string T $ rc(T) $ has three).  Every terminator in front of the end has 16 suffixes that end inside the key
// window (0 .. 15 symbols: the terminator's own suffix is the one of 0 symbols), the end of the text 15 (1 .. 15) unless the
// text ends with a terminator.  They come first, ordered by (symbols, terminator) -- the order text.hpp gives suffixes that
// agree up to the nearer terminator -- and the others follow in text order, the removed stretches skipped.  Symbols behind
// the terminator of a suffix belong to the next segment and are masked out of its key.  (Segments of at least 16 symbols:
// key16_applicable.)
struct Text16SegSrc {
    using Raw = SymWords;
    static constexpr bool kFromText = true;
    const uint64_t *__restrict__ words;
    uint32_t n;
    uint32_t treal;       // terminators in front of the end of the text
    uint32_t end_shorts;  // 15 or 0
    uint32_t nshort;      // 16 * treal + end_shorts
    uint32_t pos[kTermFew];  // pos[treal] = n
    __device__ __forceinline__ uint32_t suffix_of(size_t idx) const {
        if (idx < nshort) {
            const uint32_t c0 = treal, c1 = treal + (end_shorts ? 1u : 0u);
            uint32_t L = 0, j = (uint32_t)idx;
            if (idx >= c0) {
                L = 1u + ((uint32_t)idx - c0) / c1;
                j = ((uint32_t)idx - c0) % c1;
            }
            const uint32_t pj = j == 0 ? pos[0] : (j == 1 ? pos[1] : (j == 2 ? pos[2] : pos[3]));
            return pj - L;
        }
        uint32_t p = (uint32_t)idx - nshort;
#pragma unroll
        for (uint32_t k = 0; k + 1 < kTermFew; ++k)
            if (k < treal && p + 15u >= pos[k]) p += 16u;
        return p;
    }
    // symbols in front of the next terminator of suffix s
    __device__ __forceinline__ uint32_t limit_of(uint32_t s) const {
        uint32_t next = n;
#pragma unroll
        for (int k = (int)kTermFew - 2; k >= 0; --k)
            if ((uint32_t)k < treal && pos[k] >= s) next = pos[k];
        return next - s;
    }
    __device__ __forceinline__ uint32_t masked(const Raw &raw, uint32_t s, uint32_t &tag) const {
        const uint32_t lim = limit_of(s);
        tag = lim < (uint32_t)kP16Syms ? lim : (uint32_t)kP16Syms;
        uint32_t sym = (uint32_t)(sym_word_of<2>(raw, s) >> 32);
        if (tag < (uint32_t)kP16Syms) sym = tag == 0 ? 0u : (sym & ~((1u << (2 * ((uint32_t)kP16Syms - tag))) - 1u));
        return sym;
    }
    __device__ __forceinline__ Raw load(size_t idx, const TileExtent &) const { return sym_words<2>(words, suffix_of(idx)); }
    __device__ __forceinline__ uint64_t key_of(const Raw &raw, size_t idx, const TileExtent &) const {
        uint32_t tag;
        const uint32_t sym = masked(raw, suffix_of(idx), tag);
        return ((uint64_t)sym << kP16TagBits) | tag;
    }
    __device__ __forceinline__ uint32_t val(size_t idx) const { return suffix_of(idx); }
    __device__ __forceinline__ uint32_t hist_digit_of(const Raw &raw, size_t idx, int, const TileExtent &) const {
        uint32_t tag;
        return masked(raw, suffix_of(idx), tag) >> (32 - kRadixBits);
    }
    __device__ __forceinline__ bool digits_from_window(int) const { return false; }
    __device__ __forceinline__ uint64_t window(size_t) const { return 0; }
};
// Independent records, one BUCKET per record (radix_sort_record_keys): the pairs of a tile are the suffixes at
// the tile's own text positions, the key [kRecSyms bases][4-bit length tag] of a suffix needs the end of its
// record -- the terminator of the tile's bucket, one scalar load per tile instead of a table search per suffix.
struct RecordTextSrc {
    using Raw = SymWords;
    static constexpr bool kFromText = true;
    const uint64_t *__restrict__ words;
    const uint32_t *__restrict__ term_pos;  // terminator of record k (the separator behind it; n for the last one)
    __device__ __forceinline__ Raw load(size_t idx, const TileExtent &) const { return sym_words<2>(words, idx); }
    __device__ __forceinline__ uint32_t key_of(const Raw &raw, size_t idx, const TileExtent &ext) const {
        const uint64_t w = sym_word_of<2>(raw, idx);
        const uint32_t lim = term_pos[ext.bucket] - (uint32_t)idx;
        const uint32_t tag = lim < (uint32_t)kRecSyms ? lim : (uint32_t)kRecSyms;
        uint32_t sym = (uint32_t)(w >> (64 - kRecSyms * 2));
        if (tag < (uint32_t)kRecSyms) sym &= ~((1u << (2 * (kRecSyms - (int)tag))) - 1u);
        return (sym << kRecTagBits) | tag;
    }
    __device__ __forceinline__ uint32_t val(size_t idx) const { return (uint32_t)idx; }
    __device__ __forceinline__ uint32_t hist_digit_of(const Raw &raw, size_t idx, int shift, const TileExtent &ext) const {
        return digit_of(key_of(raw, idx, ext), shift);
    }
    __device__ __forceinline__ bool digits_from_window(int) const { return false; }
    __device__ __forceinline__ uint64_t window(size_t) const { return 0; }
};

// ---- fused records (round 4, A/B) ------------------------------------------------------------------------
// The same pass on pairs that travel as ONE 64-bit word [key : 32 | value : 32]: one staging buffer of 8-byte
// records, one store loop, bin runs of 16 x 8 = 128 bytes on average where the split form writes two streams of
// 64-byte runs.  The price is paid by the histogram kernel of the pass, which reads the records (8 B per pair)
// where the split form reads the keys alone (4 B).  kSplitOut: the last pass of a sort hands the halves to
// separate arrays (the suffix array and the key words the regroup kernel reads).
struct RecArraySrc {
    using Raw = uint64_t;
    static constexpr bool kDigitInRecord = true;
    const uint64_t *__restrict__ recs;
    __device__ __forceinline__ Raw load(size_t idx, const TileExtent &) const { return recs[idx]; }
    __device__ __forceinline__ uint64_t rec_of(Raw raw, size_t, const TileExtent &, uint32_t &) const { return raw; }
};
// the most-significant-digit pass of the 16-base key sort (Text16Src), writing records: [stored key word | suffix];
// its digit -- the first four bases -- is not part of the record
struct TextRec16Src {
    using Raw = SymWords;
    static constexpr bool kDigitInRecord = false;
    Text16Src t;
    __device__ __forceinline__ Raw load(size_t idx, const TileExtent &ext) const { return t.load(idx, ext); }
    __device__ __forceinline__ uint64_t rec_of(const Raw &raw, size_t idx, const TileExtent &ext, uint32_t &digit) const {
        const uint64_t k = t.key_of(raw, idx, ext);  // [32 key bits][8-bit tag]
        digit = (uint32_t)(k >> 32);
        return (k << 32) | t.suffix_of(idx);
    }
};

template <typename Src, bool kSplitOut>
__global__ __launch_bounds__(kThreads) void rs_scatter_rec_kernel(Src src, uint64_t *__restrict__ rec_out,
                                                                  uint32_t *__restrict__ keys_out,
                                                                  uint32_t *__restrict__ vals_out, size_t n, int shift,
                                                                  const uint32_t *__restrict__ tile_base,
                                                                  uint32_t num_tiles, SegView seg) {
    static_assert(kKeysPerThread == 16, "digits of a thread pack into four registers");
    const uint32_t tile = xcd_tile(blockIdx.x, num_tiles);
    if (tile == 0xffffffffu) return;
    const TileExtent ext = tile_extent(tile, n, num_tiles, seg);
    __shared__ __align__(16) uint64_t s_rec[kTile];
    __shared__ uint32_t s_whist[kWaves * kBins];
    __shared__ uint32_t s_glob[kBins];
    __shared__ uint32_t s_scan[kWaves];
    __shared__ uint8_t s_dig[Src::kDigitInRecord ? 4 : kTile];

    const int tid = threadIdx.x;
    const int w = tid >> 6;
    const int lane = tid & 63;
    for (int i = tid; i < kWaves * kBins; i += kThreads) s_whist[i] = 0;
    __syncthreads();

    const size_t base = ext.first;
    uint64_t rec[kKeysPerThread];
    uint32_t lrank[kKeysPerThread];
    uint32_t dpk[kKeysPerThread / 4] = {0, 0, 0, 0};  // (digits that are not part of the record, four per register)
    auto digit_at = [&](int row) -> uint32_t {
        if constexpr (Src::kDigitInRecord)
            return digit_of(rec[row], 32 + shift);
        else
            return (dpk[row >> 2] >> (8 * (row & 3))) & 255u;
    };
    constexpr int kBatch = sizeof(typename Src::Raw) > sizeof(uint64_t) ? 8 : kKeysPerThread;
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
            uint32_t d = 0;
            const uint64_t x = src.rec_of(raw[r], base + (valid ? local : 0u), ext, d);
            rec[r0 + r] = valid ? x : 0ull;
            if constexpr (!Src::kDigitInRecord) dpk[(r0 + r) >> 2] |= (valid ? d : 0u) << (8 * ((r0 + r) & 3));
        }
    }
    // ranking inside the wavefront, exactly as in rs_scatter_kernel
    uint32_t *wcount = s_whist + w * kBins;
#pragma unroll
    for (int row = 0; row < kKeysPerThread; ++row) {
        const bool valid = (uint32_t)w * kWaveSpan + (uint32_t)row * 64 + lane < ext.count;
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
#pragma unroll
    for (int row = 0; row < kKeysPerThread; ++row) {
        const uint32_t d = digit_at(row);
        lrank[row] += s_whist[w * kBins + d];
    }
#pragma unroll
    for (int row = 0; row < kKeysPerThread; ++row) {
        if ((uint32_t)w * kWaveSpan + (uint32_t)row * 64 + lane < ext.count) {
            s_rec[lrank[row]] = rec[row];
            if constexpr (!Src::kDigitInRecord) s_dig[lrank[row]] = (uint8_t)digit_at(row);
        }
    }
    __syncthreads();
    const uint32_t count = ext.count;
#pragma unroll
    for (int j = 0; j < kKeysPerThread; ++j) {
        const uint32_t p = (uint32_t)j * kThreads + tid;
        if (p < count) {
            const uint64_t x = s_rec[p];
            uint32_t d;
            if constexpr (Src::kDigitInRecord)
                d = digit_of(x, 32 + shift);
            else
                d = s_dig[p];
            const uint32_t g = s_glob[d] + p;
            if constexpr (kSplitOut) {
                keys_out[g] = (uint32_t)(x >> 32);
                vals_out[g] = (uint32_t)x;
            } else {
                rec_out[g] = x;
            }
        }
    }
}

template <typename Src, bool kSplitOut, typename HistSrc>
void radix_pass_rec(Src src, HistSrc hsrc, int hist_shift, uint64_t *rec_out, uint32_t *keys_out, uint32_t *vals_out,
                    size_t n, int shift, uint32_t *hist, uint32_t num_tiles, double hist_bytes, double scatter_bytes,
                    Arena &arena, hipStream_t stream, Profiler *prof, const SegView &seg = SegView{}) {
    hist_and_scan<uint64_t>(hsrc, n, hist_shift, hist, num_tiles, hist_bytes, arena, stream, prof, seg);
    ProfScope ps(prof, Src::kDigitInRecord ? "rs_scatter.rec" : "rs_scatter.text", stream, scatter_bytes);
    rs_scatter_rec_kernel<Src, kSplitOut><<<xcd_grid(num_tiles), kThreads, 0, stream>>>(src, rec_out, keys_out, vals_out, n, shift, hist,
                                                                                     num_tiles, seg);
    KERNEL_CHECK();
}

template <typename KeyT>
int radix_sort_impl(KeyT *keys[2], uint32_t *vals[2], size_t n, const int *shifts, int npasses, Arena &arena,
                    hipStream_t stream, Profiler *prof, int first_pass = 0) {
    if (n == 0 || npasses == 0) return 0;
    if (sizeof(KeyT) == 8)
        for (int p = 0; p < npasses; ++p)
            if ((shifts[p] & 31) + kRadixBits > 32) throw HipError("radix sort: a digit may not straddle the key halves");
    const size_t m = arena.mark();
    const uint32_t num_tiles = (uint32_t)div_up(n, kTile);
    uint32_t *hist = arena.alloc<uint32_t>((size_t)kBins * num_tiles);
    int cur = first_pass & 1;
    for (int p = first_pass; p < npasses; ++p) {
        // algorithmic bytes of one scatter launch: every (key, value) pair read once and
        // written once = 2 * (sizeof(key) + 4) bytes per pair
        radix_pass<KeyT, KeyT>(ArraySrc<KeyT>{keys[cur], vals[cur]}, keys[cur ^ 1], vals[cur ^ 1], n, shifts[p], hist,
                         num_tiles, (double)sizeof(KeyT) * (double)n, 2.0 * (sizeof(KeyT) + 4.0) * (double)n, arena,
                         stream, prof);
        cur ^= 1;
    }
    arena.rewind(m);
    return cur;
}

}  // namespace

int radix_sort_pairs(uint64_t *keys[2], uint32_t *vals[2], size_t n, const int *shifts, int npasses,
                     Arena &arena, hipStream_t stream, Profiler *prof) {
    return radix_sort_impl<uint64_t>(keys, vals, n, shifts, npasses, arena, stream, prof);
}

int radix_sort_pairs(uint32_t *keys[2], uint32_t *vals[2], size_t n, const int *shifts, int npasses,
                     Arena &arena, hipStream_t stream, Profiler *prof) {
    return radix_sort_impl<uint32_t>(keys, vals, n, shifts, npasses, arena, stream, prof);
}

void radix_pass_low16(const uint32_t *keys, const uint32_t *vals, uint16_t *keys16_out, uint32_t *vals_out, size_t n, int shift,
                      Arena &arena, hipStream_t stream, Profiler *prof) {
    const size_t m = arena.mark();
    const uint32_t num_tiles = (uint32_t)div_up(n, kTile);
    uint32_t *hist = arena.alloc<uint32_t>((size_t)kBins * num_tiles);
    radix_pass<uint32_t, uint16_t>(ArraySrc<uint32_t>{keys, vals}, keys16_out, vals_out, n, shift, hist, num_tiles,
                                   4.0 * (double)n, 14.0 * (double)n, arena, stream, prof);
    arena.rewind(m);
}

namespace {
// bucket starts of the partition the MSD pass has just made: the scanned table holds, for bin d
// and tile 0, the first output position of the bin
__global__ void bucket_starts_kernel(const uint32_t *__restrict__ scanned, uint32_t num_tiles, uint32_t n,
                                     uint32_t *__restrict__ bstart) {
    const uint32_t d = threadIdx.x;
    bstart[d] = scanned[(size_t)d * num_tiles];
    if (d == 0) bstart[kBins] = n;
}

// one descriptor per tile of the bucketed view (radix_sort.hpp)
__global__ __launch_bounds__(kThreads) void seg_desc_kernel(const uint32_t *__restrict__ bstart,
                                                            const uint32_t *__restrict__ tile0,
                                                            const uint32_t *__restrict__ prev_ne,
                                                            const uint32_t *__restrict__ next_ne, uint32_t num_tiles,
                                                            uint32_t *__restrict__ desc, uint32_t num_buckets) {
    const uint32_t tile = blockIdx.x * blockDim.x + threadIdx.x;
    if (tile >= num_tiles) return;
    uint32_t lo = 0, hi = num_buckets;  // largest b with tile0[b] <= tile (the non-empty one among equals)
    while (lo + 1 < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (tile0[mid] <= tile)
            lo = mid;
        else
            hi = mid;
    }
    const uint32_t t0 = tile0[lo], local = tile - t0;
    const uint32_t first = bstart[lo] + local * (uint32_t)kTile, end = bstart[lo + 1];
    uint32_t *d = desc + (size_t)tile * kSegDescWords;
    d[0] = first;
    d[1] = end - first < (uint32_t)kTile ? end - first : (uint32_t)kTile;
    d[2] = lo;
    d[3] = t0 * (uint32_t)kBins + local;
    d[4] = tile0[lo + 1] - t0;
    d[5] = bstart[lo];
    d[6] = end;
    d[7] = prev_ne[lo];
    d[8] = next_ne[lo];
    d[9] = d[10] = d[11] = 0;
}

// The bucketed view of nb buckets [h_start[k], h_start[k + 1]) that follow each other without gaps: tile counts,
// nearest non-empty bucket below / above, the device tables and the tile descriptors.  d_tab (device, 4 * (nb + 1)
// words) receives [bucket starts | first tiles | previous | next non-empty bucket], nb + 1 words each -- the starts
// only if they are not there yet; seg_mem holds kSegDescWords words per tile (nullptr: taken from the arena, once
// the number of tiles is known).  Waits for its copies: the host tables are locals.
SegView seg_view_of(const uint32_t *h_start, uint32_t nb, uint32_t *d_tab, bool starts_on_device, uint32_t *seg_mem, Arena &arena,
                    hipStream_t stream) {
    const size_t w = (size_t)nb + 1;
    std::vector<uint32_t> tab(4 * w);
    uint32_t *t_start = tab.data(), *t_tile0 = t_start + w, *t_prev = t_tile0 + w, *t_next = t_prev + w;
    std::copy(h_start, h_start + w, t_start);
    t_tile0[0] = 0;
    for (uint32_t k = 0; k < nb; ++k) t_tile0[k + 1] = t_tile0[k] + (uint32_t)div_up((size_t)(t_start[k + 1] - t_start[k]), kTile);
    uint32_t last = 0xffffffffu;
    for (uint32_t k = 0; k < nb; ++k) {
        t_prev[k] = last;
        if (t_start[k + 1] > t_start[k]) last = k;
    }
    last = 0xffffffffu;
    for (uint32_t k = nb; k-- > 0;) {
        t_next[k] = last;
        if (t_start[k + 1] > t_start[k]) last = k;
    }
    t_prev[nb] = t_next[nb] = 0;
    const size_t skip = starts_on_device ? w : 0;
    HIP_CHECK(hipMemcpyAsync(d_tab + skip, tab.data() + skip, (tab.size() - skip) * sizeof(uint32_t), hipMemcpyHostToDevice, stream));
    HIP_CHECK(hipStreamSynchronize(stream));  // tab is a local vector
    SegView seg;
    seg.num_tiles = t_tile0[nb];
    if (!seg_mem) seg_mem = arena.alloc<uint32_t>((size_t)kSegDescWords * seg.num_tiles + 4);
    seg_desc_kernel<<<(unsigned)div_up(seg.num_tiles, kThreads), kThreads, 0, stream>>>(d_tab, d_tab + w, d_tab + 2 * w, d_tab + 3 * w,
                                                                                   seg.num_tiles, seg_mem, nb);
    KERNEL_CHECK();
    seg.desc = seg_mem;
    return seg;
}

// The same for the 256 buckets a most-significant-digit pass has just made: their starts are read back from the
// scanned table of the pass.  tabs: 4 * 257 words, [0, 257) the bucket starts and [257, 514) the first tiles
// afterwards (local_sort_sub_buckets takes both).
SegView seg_view_of_msd_pass(const uint32_t *scanned, uint32_t tiles0, size_t n, uint32_t *tabs, uint32_t *seg_mem, Arena &arena,
                             hipStream_t stream) {
    bucket_starts_kernel<<<1, kBins, 0, stream>>>(scanned, tiles0, (uint32_t)n, tabs);
    KERNEL_CHECK();
    uint32_t h_start[kBins + 1];
    HIP_CHECK(hipMemcpyAsync(h_start, tabs, sizeof(h_start), hipMemcpyDeviceToHost, stream));
    HIP_CHECK(hipStreamSynchronize(stream));
    return seg_view_of(h_start, (uint32_t)kBins, tabs, true, seg_mem, arena, stream);
}

// npasses segmented passes over the (u32 key, u32 value) pairs of a bucketed view, least significant digit first from
// shift0 up, out of buffer pair cur; returns the pair that holds the result
int segmented_lsd_passes(uint32_t *keys[2], uint32_t *vals[2], int cur, size_t n, int shift0, int npasses, uint32_t *hist,
                         const SegView &seg, Arena &arena, hipStream_t stream, Profiler *prof) {
    for (int p = 0; p < npasses; ++p, cur ^= 1)
        radix_pass<uint32_t, uint32_t>(ArraySrc<uint32_t>{keys[cur], vals[cur]}, keys[cur ^ 1], vals[cur ^ 1], n, shift0 + 8 * p, hist,
                                       seg.num_tiles, 4.0 * (double)n, 16.0 * (double)n, arena, stream, prof, seg);
    return cur;
}

}  // namespace

void radix_sort_dna_keys(const PackedText &text, uint32_t *keys32[2], uint32_t *vals[2], uint32_t *seg_mem,
                         SegView &seg_out, Arena &arena, hipStream_t stream, Profiler *prof) {
    const size_t n = text.n;
    if (text.bits != 2) throw HipError("radix_sort_dna_keys: 2-bit texts only");
    const size_t m = arena.mark();
    const uint32_t tiles0 = (uint32_t)div_up(n, kTile);
    uint32_t *hist = arena.alloc<uint32_t>((size_t)kBins * ((size_t)tiles0 + kBins));
    uint32_t *tabs = arena.alloc<uint32_t>(4 * 257);
    const double text_bytes = (double)n * 2 / 8.0;
    // most significant digit first: key bits 32..39 = the first four bases
    // (the plain key layout for segmented texts too; their histogram digits need the masked key)
    radix_pass<uint64_t, uint32_t>(TextSrc<2>{text.words, text.terms, false, !text.segmented}, keys32[1], vals[1], n, 32, hist, tiles0,
                                   text_bytes, text_bytes + 8.0 * (double)n, arena, stream, prof);
    seg_out = seg_view_of_msd_pass(hist, tiles0, n, tabs, seg_mem, arena, stream);
    // every bucket by the low 32 key bits, least significant digit first
    segmented_lsd_passes(keys32, vals, 1, n, 0, 4, hist, seg_out, arena, stream, prof);
    arena.rewind(m);  // (the sorted pairs are in keys32[1] / vals[1] again)
}

bool key16_applicable(const PackedText &text) {
    if (text.bits != 2 || text.terms.seq_shift != 0) return false;
    if (!text.segmented) return text.terms.count == 1 && text.n >= 32;
    // a short terminator table whose segments all hold at least 16 symbols (the text may end with a terminator)
    const uint32_t cnt = text.terms.nfew;
    if (cnt < 2 || cnt > kTermFew || text.n < 64) return false;
    uint32_t start = 0;
    for (uint32_t k = 0; k < cnt; ++k) {
        const uint32_t p = text.terms.few[k];
        const bool last = k + 1 == cnt;
        if (p < start) return false;
        const uint32_t len = p - start;
        if (!(len >= 16 || (last && len == 0))) return false;
        start = p + 1;
    }
    return text.terms.few[cnt - 1] == text.n;
}

namespace {
// does radix_sort_dna_keys16 finish the sub-buckets of this text in LDS?
bool local_sort_applies(size_t n) {
    const SortKnobs &knobs = sort_knobs();
    return !knobs.no_local_sort && !local_sort_off.load() && n >= knobs.local_min(SortKnobs::kLocalSortMinText) &&
           n <= (size_t)kBins * kBins * kLocalCap / 16 * 15;
}
}  // namespace

bool key35_applicable(const PackedText &text) {
    return !sort_knobs().no_key35 && key16_applicable(text) && !text.segmented && local_sort_applies(text.n);
}

namespace {
Text16SegSrc make_text16_seg(const PackedText &text) {
    Text16SegSrc src{};
    src.words = text.words;
    src.n = text.n;
    const uint32_t cnt = text.terms.nfew;
    src.treal = cnt - 1;
    for (uint32_t k = 0; k < kTermFew; ++k) src.pos[k] = k < cnt ? text.terms.few[k] : text.n;
    // (the text ends with a terminator: the last segment is empty and the end of the text has no suffixes of its own)
    src.end_shorts = text.terms.few[cnt - 2] + 1 == text.n ? 0u : 15u;
    src.nshort = 16u * src.treal + src.end_shorts;
    return src;
}
}  // namespace

void radix_sort_dna_keys16(const PackedText &text, uint32_t *keys32[2], uint32_t *vals[2], uint32_t *seg_mem,
                           SegView &seg_out, Arena &arena, hipStream_t stream, Profiler *prof, Round0Regroup *regroup, bool key35) {
    if (regroup) regroup->done = false;
    const size_t n = text.n;
    if (!key16_applicable(text)) throw HipError("radix_sort_dna_keys16: plain 2-bit texts, or segmented ones with a short terminator table");
    const size_t m = arena.mark();
    const uint32_t tiles0 = (uint32_t)div_up(n, kTile);
    uint32_t *hist = arena.alloc<uint32_t>((size_t)kBins * ((size_t)tiles0 + kBins));
    uint32_t *tabs = arena.alloc<uint32_t>(4 * 257);
    const uint32_t *bstart = tabs, *tile0 = tabs + 257;  // (filled by seg_view_of_msd_pass)
    const double text_bytes = (double)n * 2 / 8.0;
    // Two ways from here (both end in keys32[0] / vals[0]): three bucket-segmented passes, or ONE and the sub-buckets it
    // makes sorted in LDS (local_sort_kernel) -- for texts whose 65 536 sub-buckets are large enough to pay for a
    // workgroup each and small enough to fit one (NOLZSS_NO_LOCAL_SORT, NOLZSS_LOCAL_SORT_MIN = smallest such text).
    // (the 35-bit key exists on the second way only, and the caller's plan has chosen it: key35_applicable)
    if (key35 && text.segmented) throw HipError("radix_sort_dna_keys16: the 35-bit key is for plain texts");
    const bool local = key35 || local_sort_applies(n);
    const int msd_to = local ? 0 : 1;
    // most significant digit first: the first four bases (bits 32..39 of [32 key bits][8-bit tag])
    if (text.segmented)
        radix_pass<uint64_t, uint32_t>(make_text16_seg(text), keys32[msd_to], vals[msd_to], n, 32, hist, tiles0, text_bytes,
                                       text_bytes + 8.0 * (double)n, arena, stream, prof);
    else if (key35)
        radix_pass<uint64_t, uint32_t>(Text35Src{{text.words, (uint32_t)n}}, keys32[msd_to], vals[msd_to], n, 32, hist, tiles0, text_bytes,
                                       text_bytes + 8.0 * (double)n, arena, stream, prof);
    else
        radix_pass<uint64_t, uint32_t>(Text16Src{text.words, (uint32_t)n}, keys32[msd_to], vals[msd_to], n, 32, hist, tiles0, text_bytes,
                                       text_bytes + 8.0 * (double)n, arena, stream, prof);
    seg_out = seg_view_of_msd_pass(hist, tiles0, n, tabs, seg_mem, arena, stream);
    if (local) {
        // the digit below the bucket's (four more bases: the top byte of the stored word in both layouts) first, then
        // every sub-bucket by the 16 or 19 bits between it and the tag
        segmented_lsd_passes(keys32, vals, 0, n, 24, 1, hist, seg_out, arena, stream, prof);
        local_sort_sub_buckets(keys32[1], vals[1], keys32[0], vals[0], hist, tile0, bstart, (uint32_t)kBins, key35 ? kP35TagBits : kP16TagBits, 2, n,
                               arena, stream, prof, regroup, key35);
        arena.rewind(m);
        return;
    }
    // every bucket by the 24 key bits above the tag byte, least significant digit first: THREE passes
    segmented_lsd_passes(keys32, vals, 1, n, kP16TagBits, 3, hist, seg_out, arena, stream, prof);
    arena.rewind(m);  // (the sorted pairs are in keys32[0] / vals[0])
}

void radix_sort_dna_keys16_fused(const PackedText &text, uint64_t *rec[2], uint32_t *sa_out, uint32_t *seg_mem,
                                 SegView &seg_out, Arena &arena, hipStream_t stream, Profiler *prof) {
    const size_t n = text.n;
    if (text.bits != 2 || text.segmented || text.terms.count != 1 || n < 32) throw HipError("radix_sort_dna_keys16_fused: plain 2-bit texts only");
    const size_t m = arena.mark();
    const uint32_t tiles0 = (uint32_t)div_up(n, kTile);
    uint32_t *hist = arena.alloc<uint32_t>((size_t)kBins * ((size_t)tiles0 + kBins));
    uint32_t *tabs = arena.alloc<uint32_t>(4 * 257);
    const double text_bytes = (double)n * 2 / 8.0;
    const Text16Src tsrc{text.words, (uint32_t)n};
    radix_pass_rec<TextRec16Src, false>(TextRec16Src{tsrc}, tsrc, 32, rec[1], nullptr, nullptr, n, 0, hist, tiles0, text_bytes,
                                        text_bytes + 8.0 * (double)n, arena, stream, prof);
    seg_out = seg_view_of_msd_pass(hist, tiles0, n, tabs, seg_mem, arena, stream);
    // three segmented passes over the 24 key bits above the tag byte; the last one splits the records into the key
    // words (left in the buffer the pass does not read: rec[1], as 32-bit words) and the suffix array
    int cur = 1;
    for (int p = 0; p < 3; ++p) {
        const ArraySrc<uint64_t> hsrc{rec[cur], nullptr};
        const int shift = kP16TagBits + 8 * p;
        if (p < 2)
            radix_pass_rec<RecArraySrc, false>(RecArraySrc{rec[cur]}, hsrc, 32 + shift, rec[cur ^ 1], nullptr, nullptr, n, shift,
                                               hist, seg_out.num_tiles, 8.0 * (double)n, 16.0 * (double)n, arena, stream, prof, seg_out);
        else
            radix_pass_rec<RecArraySrc, true>(RecArraySrc{rec[cur]}, hsrc, 32 + shift, nullptr, reinterpret_cast<uint32_t *>(rec[cur ^ 1]),
                                              sa_out, n, shift, hist, seg_out.num_tiles, 8.0 * (double)n, 16.0 * (double)n, arena,
                                              stream, prof, seg_out);
        cur ^= 1;
    }
    arena.rewind(m);  // (the key words are in rec[0], as 32-bit words; the suffixes in sa_out)
}

void radix_sort_record_keys(const PackedText &text, const std::vector<uint32_t> &h_terms, uint32_t *keys32[2],
                            uint32_t *vals[2], uint32_t *seg_mem, SegView &seg_out, Arena &arena, hipStream_t stream,
                            Profiler *prof) {
    const size_t n = text.n;
    const uint32_t nb = (uint32_t)h_terms.size();  // records = buckets; h_terms[k] = terminator of record k
    if (text.bits != 2 || nb == 0 || h_terms.back() != n) throw HipError("radix_sort_record_keys: bad record table");
    const size_t m = arena.mark();
    // bucket k = the text positions of record k and of the separator behind it: already "partitioned"
    std::vector<uint32_t> h_start((size_t)nb + 1);
    h_start[0] = 0;
    for (uint32_t k = 0; k + 1 < nb; ++k) h_start[k + 1] = h_terms[k] + 1;
    h_start[nb] = (uint32_t)n;
    uint32_t *d_tab = arena.alloc<uint32_t>(4 * ((size_t)nb + 1));  // (bucket starts, first tiles: seg_view_of)
    seg_out = seg_view_of(h_start.data(), nb, d_tab, false, seg_mem, arena, stream);
    uint32_t *hist = arena.alloc<uint32_t>((size_t)kBins * seg_out.num_tiles);
    const double text_bytes = (double)n * 2 / 8.0;
    // Long records (a megabase and more on average): the pass from the text takes the MOST significant digit, and the
    // 256 sub-buckets it makes of every record -- 16 Ki pairs of a 4-megabase record -- are sorted by the other three in
    // LDS (local_sort_kernel): one pass over HBM and one read + write instead of four passes.
    const SortKnobs &knobs = sort_knobs();
    if (!knobs.no_local_sort && !local_sort_off.load() && n / nb >= knobs.local_min(SortKnobs::kLocalSortMinRecord)) {
        radix_pass<uint32_t, uint32_t>(RecordTextSrc{text.words, text.terms.pos}, keys32[1], vals[1], n, 24, hist,
                                       seg_out.num_tiles, text_bytes, text_bytes + 8.0 * (double)n, arena, stream, prof, seg_out);
        local_sort_sub_buckets(keys32[1], vals[1], keys32[0], vals[0], hist, d_tab + (nb + 1), d_tab, nb, 0, 3, n, arena, stream, prof);
        arena.rewind(m);
        return;
    }
    // least significant digit first inside every record; the first pass makes its pairs from the text
    radix_pass<uint32_t, uint32_t>(RecordTextSrc{text.words, text.terms.pos}, keys32[1], vals[1], n, 0, hist,
                                   seg_out.num_tiles, text_bytes, text_bytes + 8.0 * (double)n, arena, stream, prof, seg_out);
    segmented_lsd_passes(keys32, vals, 1, n, 8, 3, hist, seg_out, arena, stream, prof);
    arena.rewind(m);  // (the sorted pairs are in keys32[0] / vals[0])
}

void debug_local_sort(uint32_t *keys[2], uint32_t *vals[2], size_t n, const uint32_t *h_start, uint32_t nb, int shift0, int npass,
                      bool key35, Round0Regroup *rg, LocalSortReport &report, Arena &arena, hipStream_t stream) {
    if (n == 0 || nb == 0 || h_start[0] != 0 || h_start[nb] != n) throw HipError("debug_local_sort: bad bucket table");
    if (rg) rg->done = false;
    struct Restore {  // (on every way out)
        bool was = local_sort_off.load();
        ~Restore() { local_sort_off.store(was); }
    } restore;
    const size_t m = arena.mark();
    uint32_t *d_tab = arena.alloc<uint32_t>(4 * ((size_t)nb + 1));  // (bucket starts, first tiles: seg_view_of)
    const SegView seg = seg_view_of(h_start, nb, d_tab, false, nullptr, arena, stream);
    uint32_t *hist = arena.alloc<uint32_t>((size_t)kBins * seg.num_tiles);
    // the digit below the bucket's first (keys[0] -> keys[1]), then every sub-bucket by the digits from shift0 up
    segmented_lsd_passes(keys, vals, 0, n, 24, 1, hist, seg, arena, stream, nullptr);
    local_sort_sub_buckets(keys[1], vals[1], keys[0], vals[0], hist, d_tab + (nb + 1), d_tab, nb, shift0, npass, n, arena, stream, nullptr,
                           rg, key35, &report);
    HIP_CHECK(hipStreamSynchronize(stream));
    arena.rewind(m);
}

int radix_sort_segments_u32(uint32_t *keys[2], uint32_t *vals[2], size_t n, const std::vector<uint32_t> &h_start, int npasses,
                            Arena &arena, hipStream_t stream, Profiler *prof) {
    const uint32_t nb = (uint32_t)h_start.size() - 1;  // segments [h_start[k], h_start[k + 1])
    if (n == 0 || npasses == 0) return 0;
    if (nb == 0 || h_start[0] != 0 || h_start[nb] != n) throw HipError("radix_sort_segments_u32: bad segment table");
    const size_t m = arena.mark();
    uint32_t *d_tab = arena.alloc<uint32_t>(4 * ((size_t)nb + 1));
    const SegView seg = seg_view_of(h_start.data(), nb, d_tab, false, nullptr, arena, stream);
    uint32_t *hist = arena.alloc<uint32_t>((size_t)kBins * seg.num_tiles);
    const int cur = segmented_lsd_passes(keys, vals, 0, n, 0, npasses, hist, seg, arena, stream, prof);
    arena.rewind(m);
    return cur;
}

int radix_sort_initial_keys(const PackedText &text, uint64_t *keys[2], uint32_t *vals[2], const int *shifts,
                            int npasses, Arena &arena, hipStream_t stream, Profiler *prof) {
    const size_t n = text.n;
    if (n == 0 || npasses == 0) return 0;
    {
        // first pass: pairs computed from the packed text, written to buffer 1.  Algorithmic bytes:
        // the text window once per kernel (bits / 8 per symbol) and, for the scatter, the sorted
        // pairs written once.
        const size_t m = arena.mark();
        const uint32_t num_tiles = (uint32_t)div_up(n, kTile);
        uint32_t *hist = arena.alloc<uint32_t>((size_t)kBins * num_tiles);
        const double text_bytes = (double)n * text.bits / 8.0;
        const double out_bytes = text_bytes + 12.0 * (double)n;
        switch (text.bits) {
        case 2:
            radix_pass<uint64_t, uint64_t>(TextSrc<2>{text.words, text.terms, text.segmented}, keys[1], vals[1], n, shifts[0], hist,
                                 num_tiles, text_bytes, out_bytes, arena, stream, prof);
            break;
        case 4:
            radix_pass<uint64_t, uint64_t>(TextSrc<4>{text.words, text.terms, text.segmented}, keys[1], vals[1], n, shifts[0], hist,
                                 num_tiles, text_bytes, out_bytes, arena, stream, prof);
            break;
        default:
            radix_pass<uint64_t, uint64_t>(TextSrc<8>{text.words, text.terms, text.segmented}, keys[1], vals[1], n, shifts[0], hist,
                                 num_tiles, text_bytes, out_bytes, arena, stream, prof);
            break;
        }
        arena.rewind(m);
    }
    return radix_sort_impl<uint64_t>(keys, vals, n, shifts, npasses, arena, stream, prof, 1);
}

}  // namespace nolzss
