// rlz_repeats.hip -- the maximal repeats of the reference itself, both strands, on the relative-LZ index (DESIGN.md 5,
// "Relative-LZ index: maximal repeats"; the entry points: rlz_index_repeats_api.hip, nolzss_rlz_index_repeat_count /
// _repeats).
//
// The occurrences of a string w on both strands are the suffixes of X that start with w inside one segment: one interval
// of the suffix array.  The right extension of an occurrence is the symbol of X behind it and its left extension the
// symbol of X in front of it -- the mirrored block complements and swaps the two sides of a reverse-strand occurrence
// exactly as the definition does --, and a terminator of X is an end mark.  So w is right-maximal with two occurrences
// iff its interval is an LCP interval [lo, hi] of value |w| (lcp[lo] < |w|, lcp[lo + 1 .. hi] >= |w| with the minimum
// attained, lcp[hi + 1] < |w|), and left-maximal iff the symbols in front of two neighbouring members differ somewhere
// in (lo, hi] or one of them is a terminator.  Every LCP interval has one representative: the leftmost rank r in
// (lo, hi] with lcp[r] = |w|.  One lane per rank decides whether it is one, and the rules of the reported set -- the
// counts, the mirror pair, the palindrome at one locus -- are range queries on the pyramids the index keeps anyway.
//
// No kernel here spins, communicates between workgroups or uses an atomic; every loop is bounded by a data size.
#include "rlz_index.hpp"

#include "nearest.hpp"
#include "radix_sort.hpp"
#include "scan.hpp"

namespace nolzss {
namespace {

constexpr int kThreads = 256;
constexpr uint32_t kEndMark = 4;  // the left context of a suffix that starts its segment: no base

// The symbol in front of suffix a of X as a 2-bit code, kEndMark at position 0 and behind a terminator.  Loop: the
// terminator search, at most 32 steps.
__device__ __forceinline__ uint32_t left_code(const PackedText &text, uint32_t a) {
    a = a < text.n ? a : text.n - 1;  // (a position by construction: no entry can lead a load out of the text)
    if (a == 0) return kEndMark;
    const uint32_t p = a - 1;
    uint32_t k;
    if (term_limit(text.terms, p, k) == 0) return kEndMark;  // p is a terminator itself
    const uint64_t bit = 2ull * p;
    return (uint32_t)(text.words[bit >> 6] >> (62 - (int)(bit & 63))) & 3u;
}

// One lane per rank r <= n.  diff[r] = 0 iff r > 0 and the suffixes at ranks r - 1 and r have the same base in front of
// them, else 1; diff[n] = 0, so that the exclusive scan E of the n + 1 entries gives the inclusive one: D[r] = E[r + 1].
// Every lane looks up the code of its own rank and reads its left neighbour's from LDS; lane 0 looks up two.
__global__ __launch_bounds__(kThreads) void rlz_repeat_left_kernel(RlzIndexView ix, uint32_t *__restrict__ diff) {
    __shared__ uint32_t code[kThreads + 1];
    const uint32_t n = ix.text.n;
    const uint64_t gid = (uint64_t)blockIdx.x * kThreads + threadIdx.x;  // (the grid covers n + 1: the first lane's is <= n)
    uint32_t c = kEndMark;
    if (gid < n) c = left_code(ix.text, ix.sa[gid]);
    code[threadIdx.x + 1] = c;
    if (threadIdx.x == 0) code[0] = gid ? left_code(ix.text, ix.sa[gid - 1]) : kEndMark;
    __syncthreads();
    if (gid > n) return;
    const uint32_t prev = code[threadIdx.x];
    diff[gid] = (gid == n || (c < kEndMark && c == prev)) ? 0u : 1u;
}

struct RepeatInterval {
    uint32_t lo, count, length, position, palindrome;
};

// Is rank r (1 <= r < n) the representative of a reported repeat?  E: the exclusive scan of diff, n + 1 entries.  Loops:
// the three pyramid descents and the two range queries, a bounded number of 16-entry blocks per level each.
__device__ __forceinline__ bool repeat_interval(const RlzIndexView &ix, const uint32_t *__restrict__ E, uint32_t r,
                                                uint32_t min_len, uint32_t min_count, RepeatInterval &out) {
    const uint32_t n = ix.text.n;
    const uint32_t l = ix.lcp[r];
    if (l < min_len) return false;  // (min_len >= 1)
    uint32_t lo, hi;
    lcp_interval(ix.Plcp, r, l, lo, hi);
    hi = hi < n ? hi : n - 1;  // (lcp[|X|] = 0 ends every interval inside the suffix array)
    if (lo >= r || hi < r) return false;  // (lcp[r] = l is not below l: never)
    // the leftmost rank of (lo, hi] whose LCP is l: none between lo and r may be <= l
    if (pyr_nearest_left<false>(ix.Plcp, r - 1, l + 1) != (int64_t)lo) return false;
    const uint32_t count = hi - lo + 1;
    if (count < min_count) return false;
    if (E[hi + 1] == E[lo + 1]) return false;  // D[hi] - D[lo] = 0: one base in front of every member
    uint32_t position = pyr_range<false>(ix.Pmin, lo, hi), palindrome = 0;
    if (ix.with_rc) {
        if (position > ix.B) return false;  // no forward member: the mirror image of this interval reports the repeat
        const uint32_t pmax = pyr_range<true>(ix.Pmax, lo, hi);
        if (pmax > ix.B) {  // the leftmost forward occurrence of rc(w) is the reverse-strand occurrence at pmax
            const uint64_t mirror = 2ull * ix.B - pmax - l + 1ull;
            if ((uint64_t)position > mirror) return false;
            if ((uint64_t)position == mirror) {  // w == rc(w): every locus is listed on both strands
                if (count < 4) return false;
                palindrome = 1;
            }
        }
    }
    out.lo = lo;
    out.count = count;
    out.length = l;
    out.position = position;
    out.palindrome = palindrome;
    return true;
}

// One lane per rank r < n: one coalesced store of the flag, whatever the lane decided.
__global__ __launch_bounds__(kThreads) void rlz_repeat_flags_kernel(RlzIndexView ix, const uint32_t *__restrict__ E,
                                                                    uint32_t min_len, uint32_t min_count,
                                                                    uint32_t *__restrict__ flag) {
    const uint64_t gid = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (gid >= ix.text.n) return;
    const uint32_t r = (uint32_t)gid;
    RepeatInterval iv;
    flag[r] = (r >= 1 && repeat_interval(ix, E, r, min_len, min_count, iv)) ? 1u : 0u;
}

// One lane per rank: a flagged rank goes to its slot of the list, slot[r] = the flags in front of it, as the pair
// (key, rank) with key = (position << 32) | length.  The slot is clamped to the list of S entries.
__global__ __launch_bounds__(kThreads) void rlz_repeat_scatter_kernel(RlzIndexView ix, const uint32_t *__restrict__ E,
                                                                      uint32_t min_len, uint32_t min_count,
                                                                      const uint32_t *__restrict__ flag,
                                                                      const uint32_t *__restrict__ slot, uint32_t S,
                                                                      uint64_t *__restrict__ keys, uint32_t *__restrict__ vals) {
    const uint64_t gid = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (gid >= ix.text.n) return;
    const uint32_t r = (uint32_t)gid;
    if (!flag[r]) return;
    RepeatInterval iv;
    if (!repeat_interval(ix, E, r, min_len, min_count, iv)) return;  // (flagged by the same rule: never)
    uint32_t s = slot[r];
    s = s < S ? s : S - 1;
    keys[s] = ((uint64_t)iv.position << 32) | iv.length;
    vals[s] = r;
}

// One lane per repeat j < S in sorted order: the interval of its representative once more, for what the records and the
// hits read of it.  rep[j] = count if its hits are reported (<= cap), else 0.
__global__ __launch_bounds__(kThreads) void rlz_repeat_interval_kernel(RlzIndexView ix, const uint32_t *__restrict__ E,
                                                                       uint32_t min_len, uint32_t min_count, uint32_t cap,
                                                                       const uint32_t *__restrict__ ranks, uint32_t S,
                                                                       uint32_t *__restrict__ first, uint32_t *__restrict__ cnt,
                                                                       uint32_t *__restrict__ rep, uint8_t *__restrict__ pal) {
    const uint64_t gid = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (gid >= S) return;
    uint32_t r = ranks[gid];
    r = r < ix.text.n ? r : ix.text.n - 1;  // (a rank by construction)
    RepeatInterval iv{0, 0, 0, 0, 0};
    if (r >= 1) repeat_interval(ix, E, r, min_len, min_count, iv);  // (a representative by construction)
    first[gid] = iv.lo;
    cnt[gid] = iv.count;
    rep[gid] = iv.count <= cap ? iv.count : 0u;
    pal[gid] = (uint8_t)iv.palindrome;
}

// One lane per record of a chunk.  Loop: the terminator search, at most 32 steps.
__global__ __launch_bounds__(kThreads) void rlz_repeat_records_kernel(TermTable xterms, const uint64_t *__restrict__ keys,
                                                                      const uint32_t *__restrict__ cnt,
                                                                      const uint8_t *__restrict__ pal, uint32_t count,
                                                                      RepeatRec *__restrict__ out) {
    const uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= count) return;
    const uint64_t key = keys[i];
    const uint32_t position = (uint32_t)(key >> 32);
    uint32_t k;
    term_limit(xterms, position, k);  // forward: the next terminator's index is the record
    RepeatRec rec;
    rec.position = position;
    rec.length = key & 0xffffffffull;
    rec.count = cnt[i];
    rec.record = k;
    rec.palindrome = pal[i];
    out[i] = rec;
}

// One lane per hit slot t < T, as rlz_index_hits_kernel: repeat j is the last one whose offset is <= t (an upper-bound
// search over the S offsets, at most 32 steps; repeats without reported hits share the offset of their successor and are
// never the last), and its length is the m of the reverse-strand coordinate.  key = (j << 33) | (position << 1) | is_rc,
// value = the record.
__global__ __launch_bounds__(kThreads) void rlz_repeat_hits_kernel(RlzIndexView ix, uint32_t records,
                                                                   const uint64_t *__restrict__ rkeys, uint32_t S,
                                                                   const uint32_t *__restrict__ off,
                                                                   const uint32_t *__restrict__ first, uint32_t T,
                                                                   uint64_t *__restrict__ keys, uint32_t *__restrict__ vals) {
    const uint64_t gid = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (gid >= T) return;
    const uint32_t t = (uint32_t)gid;
    uint32_t lo = 0, hi = S;  // the first repeat whose offset is > t lies in [lo, hi]; off[0] = 0 <= t
    for (int step = 0; step < 32 && lo < hi; ++step) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (off[mid] <= t) lo = mid + 1;
        else hi = mid;
    }
    const uint32_t j = lo ? lo - 1u : 0u;
    const uint32_t m = (uint32_t)(rkeys[j] & 0xffffffffull);
    uint32_t r = first[j] + (t - off[j]);
    r = r < ix.text.n ? r : ix.text.n - 1;  // (a rank by construction: no slot can lead a load out of the suffix array)
    const uint32_t a = ix.sa[r];
    const bool is_rc = a > ix.B;
    uint32_t k;
    term_limit(ix.text.terms, a, k);
    // forward: the next terminator's index is the record; the mirror lays the records out last to first
    const uint32_t record = is_rc ? 2u * records - 1u - k : k;
    const uint64_t position = is_rc ? 2ull * ix.B - a - m + 1ull : (uint64_t)a;
    keys[t] = ((uint64_t)j << 33) | (position << 1) | (is_rc ? 1ull : 0ull);
    vals[t] = record;
}

int bits_of(uint64_t v) {  // the number of bits that hold v
    int b = 0;
    while (v >> b) ++b;
    return b;
}

}  // namespace

void rlz_repeat_flags(Context &ctx, const RlzIndexView &ix, uint32_t min_len, uint32_t min_count, uint32_t *d_left,
                      uint32_t *d_flag, uint32_t *d_slot, uint32_t *d_total) {
    const uint32_t n = ix.text.n;
    if (n == 0) return;
    hipStream_t s = ctx.stream;
    {
        ProfScope ps(ctx.profiler(), "rlz_repeat_left", s, 8.0 * (double)n);
        rlz_repeat_left_kernel<<<(unsigned)div_up((size_t)n + 1, kThreads), kThreads, 0, s>>>(ix, d_left);
        KERNEL_CHECK();
    }
    {
        ProfScope ps(ctx.profiler(), "rlz_repeat_scans", s, 8.0 * (double)n);
        scan_exclusive_add_u32(d_left, d_left, (size_t)n + 1, nullptr, ctx.arena, s);
    }
    {
        ProfScope ps(ctx.profiler(), "rlz_repeat_flags", s, 8.0 * (double)n);
        rlz_repeat_flags_kernel<<<(unsigned)div_up((size_t)n, kThreads), kThreads, 0, s>>>(ix, d_left, min_len, min_count, d_flag);
        KERNEL_CHECK();
    }
    ProfScope ps(ctx.profiler(), "rlz_repeat_scans", s, 8.0 * (double)n);
    scan_exclusive_add_u32(d_flag, d_slot, n, d_total, ctx.arena, s);
}

// The digits of key = (position << 32) | length that can differ: the length in bits [0, bits of B), the position in bits
// [32, 32 + bits of B); no digit straddles the key halves.
int rlz_repeat_sort_shifts(uint64_t B, int *shifts) {
    const int bits = bits_of(B);  // (<= 32)
    int npasses = 0;
    for (int b = 0; b < bits; b += kRadixBits) shifts[npasses++] = b;
    for (int b = 32; b < 32 + bits; b += kRadixBits) shifts[npasses++] = b;
    return npasses;
}

RepeatList rlz_repeat_list(Context &ctx, const RlzIndexView &ix, uint32_t min_len, uint32_t min_count, uint32_t cap,
                           const uint32_t *d_left, const uint32_t *d_flag, const uint32_t *d_slot, uint32_t S) {
    RepeatList out;
    if (S == 0) return out;
    hipStream_t s = ctx.stream;
    const uint32_t n = ix.text.n;
    uint64_t *keys[2] = {ctx.arena.alloc<uint64_t>(S), ctx.arena.alloc<uint64_t>(S)};
    uint32_t *vals[2] = {ctx.arena.alloc<uint32_t>(S), ctx.arena.alloc<uint32_t>(S)};
    uint32_t *first = ctx.arena.alloc<uint32_t>(S), *cnt = ctx.arena.alloc<uint32_t>(S), *rep = ctx.arena.alloc<uint32_t>(S);
    uint8_t *pal = ctx.arena.alloc<uint8_t>(S);
    int at;
    {
        ProfScope ps(ctx.profiler(), "rlz_repeat_sort", s, 8.0 * (double)n + 12.0 * (double)S);
        rlz_repeat_scatter_kernel<<<(unsigned)div_up((size_t)n, kThreads), kThreads, 0, s>>>(ix, d_left, min_len, min_count, d_flag,
                                                                                             d_slot, S, keys[0], vals[0]);
        KERNEL_CHECK();
        int shifts[kLocateMaxPasses];
        const int npasses = rlz_repeat_sort_shifts(ix.B, shifts);
        at = radix_sort_pairs(keys, vals, S, shifts, npasses, ctx.arena, s, ctx.profiler());
    }
    ProfScope ps(ctx.profiler(), "rlz_repeat_intervals", s, 17.0 * (double)S);
    rlz_repeat_interval_kernel<<<(unsigned)div_up((size_t)S, kThreads), kThreads, 0, s>>>(ix, d_left, min_len, min_count, cap,
                                                                                          vals[at], S, first, cnt, rep, pal);
    KERNEL_CHECK();
    out.keys = keys[at];
    out.first = first;
    out.count = cnt;
    out.rep = rep;
    out.pal = pal;
    out.S = S;
    return out;
}

void rlz_repeat_records(Context &ctx, const RlzIndexView &ix, const RepeatList &list, size_t first, uint32_t count,
                        RepeatRec *d_out) {
    if (count == 0) return;
    ProfScope ps(ctx.profiler(), "rlz_repeat_records", ctx.stream, 45.0 * (double)count);
    rlz_repeat_records_kernel<<<(unsigned)div_up((size_t)count, kThreads), kThreads, 0, ctx.stream>>>(
        ix.text.terms, list.keys + first, list.count + first, list.pal + first, count, d_out);
    KERNEL_CHECK();
}

LocateSorted rlz_repeat_hits(Context &ctx, const RlzIndexView &ix, uint32_t records, const RepeatList &list, uint32_t T) {
    LocateSorted out;
    if (T == 0 || list.S == 0) return out;
    hipStream_t s = ctx.stream;
    uint32_t *d_off = ctx.arena.alloc<uint32_t>(list.S);
    uint64_t *keys[2] = {ctx.arena.alloc<uint64_t>(T), ctx.arena.alloc<uint64_t>(T)};
    uint32_t *vals[2] = {ctx.arena.alloc<uint32_t>(T), ctx.arena.alloc<uint32_t>(T)};
    rlz_index_hit_offsets(ctx, list.rep, list.S, d_off);
    {
        ProfScope ps(ctx.profiler(), "rlz_repeat_hits", s, 16.0 * (double)T);
        rlz_repeat_hits_kernel<<<(unsigned)div_up((size_t)T, kThreads), kThreads, 0, s>>>(ix, records, list.keys, list.S, d_off,
                                                                                          list.first, T, keys[0], vals[0]);
        KERNEL_CHECK();
    }
    int shifts[kLocateMaxPasses];
    const int npasses = rlz_locate_sort_shifts(ix.B, list.S, shifts);
    ProfScope ps(ctx.profiler(), "rlz_repeat_hit_sort", s, 24.0 * (double)T * npasses);
    const int at = radix_sort_pairs(keys, vals, T, shifts, npasses, ctx.arena, s, ctx.profiler());
    out.keys = keys[at];
    out.vals = vals[at];
    return out;
}

}  // namespace nolzss
