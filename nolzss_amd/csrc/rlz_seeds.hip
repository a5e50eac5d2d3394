// rlz_seeds.hip -- maximal exact match seeds of a target batch on the relative-LZ index ("Relative-LZ index:
// maximal match seeds"; the entry point: rlz_index_api.hip, nolzss_rlz_index_seeds).
//
// rlz_index_search leaves ms[p] = len[p], the longest match of the target suffix at p, and a rank that attains it.  A
// match that occurs still occurs without its first base, so ms[p + 1] >= ms[p] - 1, and the matches [p, p + ms[p]) that no
// other match of the target contains are those with ms[p - 1] <= ms[p]: a longer left neighbour would reach as far or
// further.  A separator has ms = 0, so the first position of a target needs no rule of its own.  Every occurrence of a
// seed of L bases, on either strand, lies in the LCP interval I(L) around its rank: the interval is expanded and sorted as
// the hits of a pattern are (rlz_locate.hip), without a second bisection.
//
// No kernel here spins, communicates between workgroups or uses an atomic; every loop is bounded by a data size.
#include "rlz_index.hpp"

#include "nearest.hpp"
#include "radix_sort.hpp"
#include "scan.hpp"

namespace nolzss {
namespace {

constexpr int kThreads = 256;

// One lane per batch position: two coalesced loads of len.  No loop.
__global__ __launch_bounds__(kThreads) void rlz_seed_flags_kernel(const uint32_t *__restrict__ len, uint32_t n,
                                                                  uint32_t min_len, uint32_t *__restrict__ flag) {
    const uint64_t gid = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (gid >= n) return;
    const uint32_t p = (uint32_t)gid;
    const uint32_t l = len[p], left = p ? len[p - 1] : 0u;
    flag[p] = (l >= min_len && left <= l) ? 1u : 0u;  // (min_len >= 1: a position without a match is never a seed)
}

// One lane per batch position: a flagged position goes to its slot of the seed list, slot[p] = the flags in front of it,
// so the list ascends by position.  The slot is clamped to the list, which holds one entry per position.  No loop.
__global__ __launch_bounds__(kThreads) void rlz_seed_scatter_kernel(const uint32_t *__restrict__ flag,
                                                                    const uint32_t *__restrict__ slot, uint32_t n,
                                                                    uint32_t *__restrict__ seeds) {
    const uint64_t gid = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (gid >= n) return;
    const uint32_t p = (uint32_t)gid;
    if (!flag[p]) return;
    const uint32_t s = slot[p];
    seeds[s < n ? s : n - 1] = p;
}

// One lane per SEED j of [j0, j0 + count).  first[j] = the first rank of I(L) around the seed's rank, rep[j] = its
// occurrences on both strands if they are reported (<= cap), else 0; with `out`, the record of seed j goes to out[j - j0].
// Loops: the two pyramid descents of lcp_interval, one block per level; the terminator search, at most 32 steps.
__global__ __launch_bounds__(kThreads) void rlz_seed_interval_kernel(RlzIndexView ix, TermTable tterms, uint32_t n,
                                                                     const uint32_t *__restrict__ seeds, uint32_t j0,
                                                                     uint32_t count, uint32_t cap,
                                                                     const uint32_t *__restrict__ len,
                                                                     const uint32_t *__restrict__ rank,
                                                                     uint32_t *__restrict__ out_first,
                                                                     uint32_t *__restrict__ out_rep,
                                                                     SeedRec *__restrict__ out) {
    const uint64_t gid = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (gid >= count) return;
    const uint32_t j = j0 + (uint32_t)gid;
    uint32_t p = seeds[j];
    p = p < n ? p : n - 1;  // (a position by construction: no entry can lead a load out of the batch)
    const uint32_t nx = ix.text.n;
    const uint32_t L = len[p];
    uint32_t r = rank[p];
    r = r < nx ? r : nx - 1;  // (a rank by construction)
    uint32_t first = 0, occ = 0;
    if (L) {  // (a seed by construction)
        uint32_t ilo, ihi;
        lcp_interval(ix.Plcp, r, L, ilo, ihi);
        ihi = ihi < nx ? ihi : nx - 1;  // (lcp[|X|] = 0 ends every interval inside the suffix array)
        first = ilo;
        occ = ihi >= ilo ? ihi - ilo + 1u : 0u;
    }
    out_first[j] = first;
    out_rep[j] = occ <= cap ? occ : 0u;
    if (!out) return;
    uint32_t t;
    term_limit(tterms, p, t);  // the next terminator's index is the target
    t = t < tterms.count ? t : tterms.count - 1;
    SeedRec s;
    s.target = t;
    s.start = p - (t ? tterms.pos[t - 1] + 1u : 0u);
    s.length = L;
    s.count = occ;
    out[gid] = s;
}

// One lane per hit slot t < T, as rlz_index_hits_kernel: seed j is the last one whose offset is <= t (an upper-bound
// search over the S offsets, at most 32 steps; seeds without reported hits share the offset of their successor and are
// never the last), and its length is the m of the reverse-strand coordinate.  key = (j << 33) | (position << 1) | is_rc,
// value = the record.
__global__ __launch_bounds__(kThreads) void rlz_seed_hits_kernel(RlzIndexView ix, uint32_t records, uint32_t n,
                                                                 const uint32_t *__restrict__ seeds,
                                                                 const uint32_t *__restrict__ len, uint32_t S,
                                                                 const uint32_t *__restrict__ off,
                                                                 const uint32_t *__restrict__ first, uint32_t T,
                                                                 uint64_t *__restrict__ keys, uint32_t *__restrict__ vals) {
    const uint64_t gid = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (gid >= T) return;
    const uint32_t t = (uint32_t)gid;
    uint32_t lo = 0, hi = S;  // the first seed whose offset is > t lies in [lo, hi]; off[0] = 0 <= t
    for (int step = 0; step < 32 && lo < hi; ++step) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (off[mid] <= t) lo = mid + 1;
        else hi = mid;
    }
    const uint32_t j = lo ? lo - 1u : 0u;
    uint32_t p = seeds[j];
    p = p < n ? p : n - 1;  // (a position by construction)
    const uint32_t m = len[p];
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

}  // namespace

void rlz_index_seed_list(Context &ctx, const uint32_t *d_len, uint32_t n, uint32_t min_len, uint32_t *d_flag,
                         uint32_t *d_slot, uint32_t *d_seeds, uint32_t *d_total) {
    if (n == 0) return;
    hipStream_t s = ctx.stream;
    const unsigned blocks = (unsigned)div_up((size_t)n, kThreads);
    ProfScope ps(ctx.profiler(), "rlz_seed_flags", s, 24.0 * (double)n);
    rlz_seed_flags_kernel<<<blocks, kThreads, 0, s>>>(d_len, n, min_len ? min_len : 1u, d_flag);
    KERNEL_CHECK();
    scan_exclusive_add_u32(d_flag, d_slot, n, d_total, ctx.arena, s);
    rlz_seed_scatter_kernel<<<blocks, kThreads, 0, s>>>(d_flag, d_slot, n, d_seeds);
    KERNEL_CHECK();
}

void rlz_index_seed_intervals(Context &ctx, const RlzIndexView &ix, const PackedText &batch, const uint32_t *d_seeds,
                              uint32_t first, uint32_t count, uint32_t cap, const uint32_t *d_len, const uint32_t *d_rank,
                              uint32_t *d_first, uint32_t *d_rep, SeedRec *d_out) {
    if (count == 0) return;
    ProfScope ps(ctx.profiler(), "rlz_seed_intervals", ctx.stream, (d_out ? 52.0 : 20.0) * (double)count);
    rlz_seed_interval_kernel<<<(unsigned)div_up((size_t)count, kThreads), kThreads, 0, ctx.stream>>>(
        ix, batch.terms, batch.n, d_seeds, first, count, cap, d_len, d_rank, d_first, d_rep, d_out);
    KERNEL_CHECK();
}

LocateSorted rlz_index_seed_hits(Context &ctx, const RlzIndexView &ix, uint32_t records, uint32_t n, const uint32_t *d_seeds,
                                 const uint32_t *d_len, uint32_t S, const uint32_t *d_rep, const uint32_t *d_first,
                                 uint32_t T) {
    LocateSorted out;
    if (T == 0 || S == 0) return out;
    hipStream_t s = ctx.stream;
    uint32_t *d_off = ctx.arena.alloc<uint32_t>(S);
    uint64_t *keys[2] = {ctx.arena.alloc<uint64_t>(T), ctx.arena.alloc<uint64_t>(T)};
    uint32_t *vals[2] = {ctx.arena.alloc<uint32_t>(T), ctx.arena.alloc<uint32_t>(T)};
    {
        ProfScope ps(ctx.profiler(), "rlz_seed_hits", s, 8.0 * (double)S + 16.0 * (double)T);
        scan_exclusive_add_u32(d_rep, d_off, S, nullptr, ctx.arena, s);
        rlz_seed_hits_kernel<<<(unsigned)div_up((size_t)T, kThreads), kThreads, 0, s>>>(ix, records, n, d_seeds, d_len, S,
                                                                                        d_off, d_first, T, keys[0], vals[0]);
        KERNEL_CHECK();
    }
    int shifts[kLocateMaxPasses];
    const int npasses = rlz_locate_sort_shifts(ix.B, S, shifts);
    ProfScope ps(ctx.profiler(), "rlz_seed_sort", s, 24.0 * (double)T * npasses);
    const int at = radix_sort_pairs(keys, vals, T, shifts, npasses, ctx.arena, s, ctx.profiler());
    out.keys = keys[at];
    out.vals = vals[at];
    return out;
}

}  // namespace nolzss
