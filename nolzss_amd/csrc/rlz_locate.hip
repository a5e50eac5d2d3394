// rlz_locate.hip -- pattern count and locate queries on the relative-LZ index ("Relative-LZ index: pattern
// count and locate"; the entry points: rlz_index_api.hip, nolzss_rlz_index_count / _locate).
//
// A pattern P of m bases is placed among the suffixes of X by the bisection of the match (rlz_index.hip), in the same
// order: the pattern's end is the smallest terminator, so P sorts in front of every suffix it is a prefix of and the
// insertion rank q is the lower end of P's suffix-array interval.  P occurs iff its common prefix with rank q is all of
// P -- the left neighbour is smaller than P and can never carry it --, and the occurrences are then exactly I(m) around
// q.  A suffix below B is a forward occurrence, one above B lies in the mirrored block: a reverse-strand occurrence at
// the forward coordinate 2 B - a - m + 1.
//
// No kernel here spins, communicates between workgroups or uses an atomic; every loop is bounded by a data size.
#include "rlz_index.hpp"

#include "nearest.hpp"
#include "radix_sort.hpp"
#include "scan.hpp"

namespace nolzss {
namespace {

constexpr int kThreads = 256;

// pattern j of the batch P1 s P2 s .. Pq s: its first position and its length from the terminator table (pos[j] = the
// separator behind pattern j; q + 1 entries)
__device__ __forceinline__ uint32_t pattern_start(const uint32_t *__restrict__ tpos, uint32_t j, uint32_t &m) {
    const uint32_t p = j ? tpos[j - 1] + 1u : 0u;
    m = tpos[j] - p;
    return p;
}

// One lane per PATTERN.  cnt[j] = occurrences on both strands, lo[j] = the first rank of the interval (0 without an
// occurrence), rep[j] = cnt[j] if it is reported (<= cap), else 0.  Loops: the bisection, at most 32 steps; the
// comparisons, m / 32 + kCrossWords words each; the two pyramid descents of lcp_interval, one block per level.
__global__ __launch_bounds__(kThreads) void rlz_index_pattern_kernel(RlzIndexView ix, const uint64_t *__restrict__ tw,
                                                                     const uint32_t *__restrict__ tpos, uint32_t q,
                                                                     uint32_t cap, uint32_t *__restrict__ out_lo,
                                                                     uint32_t *__restrict__ out_cnt,
                                                                     uint32_t *__restrict__ out_rep) {
    const uint64_t gid = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (gid >= q) return;
    const uint32_t j = (uint32_t)gid;
    const uint64_t *__restrict__ xw = ix.text.words;
    const uint32_t *__restrict__ sa = ix.sa;
    uint32_t m;
    const uint32_t p = pattern_start(tpos, j, m);
    uint32_t first = 0, count = 0;
    if (m) {
        const uint32_t nx = ix.text.n;
        uint32_t lo = 0, hi = nx;  // the insertion rank lies in [lo, hi]
        if (m >= ix.P) {
            const uint32_t w = (uint32_t)(sym_word<2>(tw, p) >> (64 - 2 * ix.P));
            lo = ix.table[w];
            hi = ix.table[w + 1];
            hi = hi < nx ? hi : nx;  // (ranks by construction: no entry can lead a load out of the suffix array)
            lo = lo < hi ? lo : hi;
        }
        // Manber-Myers, as rlz_index_search_kernel: rank lo - 1 is smaller and rank hi not smaller than the pattern
        uint32_t llo = 0, lhi = 0;
        bool khi = false;
        for (int step = 0; step < 32 && lo < hi; ++step) {  // hi - lo halves: at most 32 steps
            const uint32_t mid = lo + (hi - lo) / 2;
            uint32_t l;
            if (cross_suffix_less(xw, ix.text.terms, sa[mid], tw, p, m, llo < lhi ? llo : lhi, l)) {
                lo = mid + 1;
                llo = l;
            } else {
                hi = mid;
                lhi = l;
                khi = true;
            }
        }
        // the right neighbour of the insertion rank lo; one that was never a mid is compared once
        uint32_t lr = 0;
        if (lo < nx) {
            if (khi) lr = lhi;
            else cross_suffix_less(xw, ix.text.terms, sa[lo], tw, p, m, 0u, lr);
        }
        if (lr == m) {
            uint32_t ilo, ihi;
            lcp_interval(ix.Plcp, lo, m, ilo, ihi);
            ihi = ihi < nx ? ihi : nx - 1;  // (lcp[|X|] = 0 ends every interval inside the suffix array)
            first = ilo;
            count = ihi >= ilo ? ihi - ilo + 1u : 0u;
        }
    }
    out_lo[j] = first;
    out_cnt[j] = count;
    out_rep[j] = count <= cap ? count : 0u;
}

// One lane per hit slot t < T: the load is balanced however skewed the counts are.  Pattern j is the last one whose
// offset is <= t (an upper-bound search over the q offsets, at most 32 steps; patterns without reported hits share the
// offset of their successor and are never the last).  key = (j << 33) | (position << 1) | is_rc, value = the record.
__global__ __launch_bounds__(kThreads) void rlz_index_hits_kernel(RlzIndexView ix, uint32_t records,
                                                                  const uint32_t *__restrict__ tpos, uint32_t q,
                                                                  const uint32_t *__restrict__ off,
                                                                  const uint32_t *__restrict__ first, uint32_t T,
                                                                  uint64_t *__restrict__ keys, uint32_t *__restrict__ vals) {
    const uint64_t gid = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (gid >= T) return;
    const uint32_t t = (uint32_t)gid;
    uint32_t lo = 0, hi = q;  // the first pattern whose offset is > t lies in [lo, hi]; off[0] = 0 <= t
    for (int step = 0; step < 32 && lo < hi; ++step) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (off[mid] <= t) lo = mid + 1;
        else hi = mid;
    }
    const uint32_t j = lo ? lo - 1u : 0u;
    uint32_t m;
    pattern_start(tpos, j, m);
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

__global__ __launch_bounds__(kThreads) void rlz_index_hit_records_kernel(const uint64_t *__restrict__ keys,
                                                                         const uint32_t *__restrict__ vals, uint32_t count,
                                                                         LocateHit *__restrict__ out) {
    const uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= count) return;
    const uint64_t key = keys[i];
    LocateHit h;
    h.position = (key >> 1) & 0xffffffffull;
    h.record = vals[i];
    h.is_rc = (uint32_t)(key & 1ull);
    out[i] = h;
}

int bits_of(uint64_t v) {  // the number of bits that hold v
    int b = 0;
    while (v >> b) ++b;
    return b;
}

}  // namespace

void rlz_index_patterns(Context &ctx, const RlzIndexView &ix, const PackedText &batch, uint32_t q, uint32_t cap,
                        uint32_t *d_lo, uint32_t *d_cnt, uint32_t *d_rep) {
    if (q == 0) return;
    ProfScope ps(ctx.profiler(), "rlz_index_pattern", ctx.stream);
    rlz_index_pattern_kernel<<<(unsigned)div_up((size_t)q, kThreads), kThreads, 0, ctx.stream>>>(
        ix, batch.words, batch.terms.pos, q, cap, d_lo, d_cnt, d_rep);
    KERNEL_CHECK();
}

void rlz_index_hit_offsets(Context &ctx, const uint32_t *d_rep, uint32_t q, uint32_t *d_off) {
    if (q == 0) return;
    ProfScope ps(ctx.profiler(), "rlz_locate_offsets", ctx.stream, 8.0 * (double)q);
    scan_exclusive_add_u32(d_rep, d_off, q, nullptr, ctx.arena, ctx.stream);
}

// The digits of key = (j << 33) | (position << 1) | is_rc that can differ: (position, strand) in bits [0, 1 + bits of B),
// the pattern in bits [33, 33 + bits of q - 1).  A digit of the 64-bit sort may not straddle the key halves, so the low
// half is sorted by the digits at 0, 8, 16, 24 and the high half by those at 32, 40, 48, 56 -- the one at 32 holds the
// top position bit and the low seven bits of the pattern --, each as far up as a bit can be set.
int rlz_locate_sort_shifts(uint64_t B, uint64_t q, int *shifts) {
    const int low = 1 + bits_of(B), high = q ? bits_of(q - 1) : 0;  // (low <= 33, high <= 31)
    const int top = high ? 33 + high : low;
    int npasses = 0;
    for (int b = 0; b < (low < 32 ? low : 32); b += kRadixBits) shifts[npasses++] = b;
    for (int b = 32; b < top; b += kRadixBits) shifts[npasses++] = b;
    return npasses;
}

LocateSorted rlz_index_hits(Context &ctx, const RlzIndexView &ix, uint32_t records, const PackedText &batch, uint32_t q,
                            const uint32_t *d_off, const uint32_t *d_lo, uint32_t T) {
    LocateSorted out;
    if (T == 0) return out;
    hipStream_t s = ctx.stream;
    uint64_t *keys[2] = {ctx.arena.alloc<uint64_t>(T), ctx.arena.alloc<uint64_t>(T)};
    uint32_t *vals[2] = {ctx.arena.alloc<uint32_t>(T), ctx.arena.alloc<uint32_t>(T)};
    {
        ProfScope ps(ctx.profiler(), "rlz_index_hits", s, 16.0 * (double)T);
        rlz_index_hits_kernel<<<(unsigned)div_up((size_t)T, kThreads), kThreads, 0, s>>>(ix, records, batch.terms.pos, q, d_off,
                                                                                         d_lo, T, keys[0], vals[0]);
        KERNEL_CHECK();
    }
    int shifts[kLocateMaxPasses];
    const int npasses = rlz_locate_sort_shifts(ix.B, q, shifts);
    ProfScope ps(ctx.profiler(), "rlz_locate_sort", s, 24.0 * (double)T * npasses);
    const int at = radix_sort_pairs(keys, vals, T, shifts, npasses, ctx.arena, s, ctx.profiler());
    out.keys = keys[at];
    out.vals = vals[at];
    return out;
}

void rlz_index_hit_records(Context &ctx, const LocateSorted &sorted, size_t first, uint32_t count, LocateHit *d_out) {
    if (count == 0) return;
    ProfScope ps(ctx.profiler(), "rlz_index_hit_records", ctx.stream, 28.0 * (double)count);
    rlz_index_hit_records_kernel<<<(unsigned)div_up((size_t)count, kThreads), kThreads, 0, ctx.stream>>>(
        sorted.keys + first, sorted.vals + first, count, d_out);
    KERNEL_CHECK();
}

}  // namespace nolzss
