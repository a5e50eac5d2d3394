// rlz_index.hip -- relative-LZ index: the prefix table over the suffix array of the index text, the search of a target
// batch in it, and the factor records from the ranks the search found ("Relative-LZ index: targets matched
// against a resident reference").
//
// A target suffix T[p..) is placed among the suffixes of X by bisection over the suffix array: the order is the one of
// text.hpp with the target's end as the smallest terminator.  The longest match of T[p..) in X is the larger of its
// common prefixes with the two neighbours of the insertion rank, and every occurrence of that match on either strand
// lies in the LCP interval I(L) around the neighbour: min SA over it below B is the leftmost forward occurrence (forward
// wins ties without a second search, since I(L) holds a block suffix exactly when Lf = L), otherwise max SA is the
// rightmost mirrored one, i.e. the leftmost reverse-complement occurrence in forward coordinates.
//
// No kernel here spins, communicates between workgroups or uses an atomic; every loop is bounded by a data size.
#include "rlz_index.hpp"

#include "nearest.hpp"

namespace nolzss {
namespace {

constexpr int kThreads = 256;
constexpr uint32_t kLenMask = 0x7fffffffu;

__device__ __forceinline__ uint32_t padded_key(const PackedText &text, uint32_t a, uint32_t P) {
    uint32_t k;
    const uint32_t lim = term_limit(text.terms, a, k);
    uint64_t w = sym_word<2>(text.words, a) >> (64 - 2 * P);
    if (lim < P) w &= ~((1ull << (2 * (P - lim))) - 1ull);  // bases behind the terminator belong to the next segment
    return (uint32_t)w;
}

// One lane per rank r <= n: the padded keys do not decrease with the rank (a suffix that meets its terminator inside
// the P bases is a prefix of the longer ones that continue its padded key with A's and sorts in front of them), so rank
// r is the answer for every key in (key[r - 1], key[r]]; rank n stands for the key 4^P behind the last one.  The
// 4^P + 1 entries are written once each.
__global__ __launch_bounds__(kThreads) void rlz_index_table_kernel(PackedText text, const uint32_t *__restrict__ sa,
                                                                   uint32_t P, uint32_t *__restrict__ table) {
    const uint64_t r = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (r > text.n) return;
    const uint32_t last = r < text.n ? padded_key(text, sa[r], P) : 1u << (2 * P);
    const uint32_t first = r > 0 ? padded_key(text, sa[r - 1], P) + 1u : 0u;
    for (uint32_t w = first; w <= last; ++w) table[w] = (uint32_t)r;
}

// The hot path: one lane per position of the batch.
__global__ __launch_bounds__(kThreads) void rlz_index_search_kernel(RlzIndexView ix, const uint64_t *__restrict__ tw,
                                                                    TermTable tterms, uint32_t n,
                                                                    uint32_t *__restrict__ out_len,
                                                                    uint32_t *__restrict__ out_rank) {
    const uint64_t gid = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (gid >= n) return;
    const uint32_t p = (uint32_t)gid;
    const uint64_t *__restrict__ xw = ix.text.words;
    const uint32_t *__restrict__ sa = ix.sa;
    uint32_t tk;
    const uint32_t rem = term_limit(tterms, p, tk);  // bases before the target's end; 0 at a separator
    uint32_t len = 0, rank = 0;
    if (rem) {
        const uint32_t nx = ix.text.n;
        uint32_t lo = 0, hi = nx;  // the insertion rank lies in [lo, hi]
        if (rem >= ix.P) {
            const uint32_t w = (uint32_t)(sym_word<2>(tw, p) >> (64 - 2 * ix.P));
            lo = ix.table[w];
            hi = ix.table[w + 1];
            hi = hi < nx ? hi : nx;  // (ranks by construction: no entry can lead a load out of the suffix array)
            lo = lo < hi ? lo : hi;
        }
        // Manber-Myers: rank lo - 1 is smaller and rank hi greater than the target suffix, with common prefixes llo and
        // lhi once they have been a mid; every suffix between them then shares min(llo, lhi) symbols with it
        uint32_t llo = 0, lhi = 0;
        bool klo = false, khi = false;
        for (int step = 0; step < 32 && lo < hi; ++step) {  // hi - lo halves: at most 32 steps
            const uint32_t mid = lo + (hi - lo) / 2;
            const uint32_t a = sa[mid];
            uint32_t l;
            if (cross_suffix_less(xw, ix.text.terms, a, tw, p, rem, llo < lhi ? llo : lhi, l)) {
                lo = mid + 1;
                llo = l;
                klo = true;
            } else {
                hi = mid;
                lhi = l;
                khi = true;
            }
        }
        // the two neighbours of the insertion rank lo; one that was never a mid (an empty bucket, a bucket's edge) is
        // compared once
        uint32_t ll = 0, lr = 0;
        if (lo > 0) {
            if (klo) ll = llo;
            else cross_suffix_less(xw, ix.text.terms, sa[lo - 1], tw, p, rem, 0u, ll);
        }
        if (lo < nx) {
            if (khi) lr = lhi;
            else cross_suffix_less(xw, ix.text.terms, sa[lo], tw, p, rem, 0u, lr);
        }
        len = ll >= lr ? ll : lr;
        rank = len ? (ll >= lr ? lo - 1 : lo) : 0u;
    }
    out_len[p] = len;
    out_rank[p] = rank;
}

// strand and reference of a match of L >= 1 symbols whose occurrences are I(L) around rank r
__device__ __forceinline__ void index_reference(const RlzIndexView &ix, uint32_t L, uint32_t r, bool &is_rc,
                                                uint64_t &ref) {
    uint32_t lo, hi;
    lcp_interval(ix.Plcp, r, L, lo, hi);
    const uint32_t mn = pyr_range<false>(ix.Pmin, lo, hi);
    is_rc = ix.with_rc && mn >= ix.B;
    if (!is_rc) {
        ref = mn;
    } else {
        const uint32_t mx = pyr_range<true>(ix.Pmax, lo, hi);
        // 2 rcN = B - 1 + E = 2 B: the forward coordinate of the last matched base, as factor_kernel (chain.hip)
        ref = (1ull << 63) | (2ull * ix.B - mx - L + 1);
    }
}

// kAll = false: one record per factor start.  kAll = true: the same look-ups at every position, only the strand kept.
template <bool kAll>
__global__ __launch_bounds__(kThreads) void rlz_index_record_kernel(RlzIndexView ix, const uint32_t *__restrict__ fpos,
                                                                    uint32_t z, uint32_t *len,
                                                                    const uint32_t *__restrict__ rank,
                                                                    IndexRec *__restrict__ out) {
    const uint64_t k = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (k >= z) return;
    const uint32_t p = kAll ? (uint32_t)k : fpos[k];
    const uint32_t L = len[p] & kLenMask;
    bool is_rc = false;
    uint64_t ref = 0;
    if (L) index_reference(ix, L, rank[p], is_rc, ref);
    if (kAll) {
        if (is_rc) len[p] = L | 0x80000000u;
        return;
    }
    IndexRec f;
    f.start = (uint64_t)ix.B + 1u + p;
    f.length = L ? L : 1u;
    f.ref = L ? ref : f.start;
    out[k] = f;
}

size_t padded(size_t bytes) { return (bytes + 255) & ~size_t(255); }
// (finish_packing, text_pack.hip: the packed words and their zero pad words)
size_t packed_words(uint32_t n) { return div_up((size_t)n * 2, 64) + 8; }
size_t coarse_entries(uint32_t n) { return (size_t)(n >> kTermBlockShift) + 3; }

}  // namespace

RlzIndexView rlz_index_build(Context &ctx, const uint8_t *d_X, uint32_t n, uint32_t B, bool with_rc, uint32_t P) {
    Arena &arena = ctx.arena;
    hipStream_t s = ctx.stream;
    RlzIndexView v;
    v.text = pack_text(ctx, d_X, n);
    if (!v.text.segmented || v.text.bits != 2) throw HipError("rlz index: the index text did not pack segmented at 2 bits");
    uint32_t *sa = arena.alloc<uint32_t>(n);
    uint32_t *lcp = arena.alloc<uint32_t>((size_t)n + 1);
    {
        const size_t mark = arena.mark();
        uint32_t *isa = arena.alloc<uint32_t>(n);  // (the construction needs it; a match does not)
        build_suffix_array(ctx, v.text, sa, isa, lcp);
        arena.rewind(mark);
    }
    v.sa = sa;
    v.lcp = lcp;
    v.Plcp = build_lcp_pyramid(ctx, v.text, sa, lcp);
    {
        ProfScope ps(ctx.profiler(), "pyramids", s);
        v.Pmin = build_pyramid(sa, n, false, arena, s);
        v.Pmax = with_rc ? build_pyramid(sa, n, true, arena, s) : v.Pmin;
    }
    const size_t entries = ((size_t)1 << (2 * P)) + 1;
    uint32_t *table = arena.alloc<uint32_t>(entries);
    {
        ProfScope ps(ctx.profiler(), "rlz_index_table", s, 4.0 * (double)entries + 8.0 * (double)n);
        rlz_index_table_kernel<<<(unsigned)div_up((size_t)n + 1, kThreads), kThreads, 0, s>>>(v.text, sa, P, table);
        KERNEL_CHECK();
    }
    v.table = table;
    v.P = P;
    v.B = B;
    v.with_rc = with_rc;
    return v;
}

namespace {

// the arrays of a view in the order they are laid out; walk() calls f(pointer slot, bytes) for each
template <typename F> void walk(RlzIndexView &v, F &&f) {
    const uint32_t n = v.text.n;
    f(reinterpret_cast<const void **>(&v.text.words), packed_words(n) * sizeof(uint64_t));
    f(reinterpret_cast<const void **>(&v.text.terms.pos), (size_t)v.text.terms.count * sizeof(uint32_t));
    if (v.text.terms.coarse) f(reinterpret_cast<const void **>(&v.text.terms.coarse), coarse_entries(n) * sizeof(uint32_t));
    f(reinterpret_cast<const void **>(&v.sa), (size_t)n * sizeof(uint32_t));
    f(reinterpret_cast<const void **>(&v.lcp), ((size_t)n + 1) * sizeof(uint32_t));
    Pyramid *pyr[3] = {&v.Plcp, &v.Pmin, &v.Pmax};
    for (int k = 0; k < (v.with_rc ? 3 : 2); ++k)
        for (int l = 1; l < pyr[k]->nlev; ++l)
            f(reinterpret_cast<const void **>(&pyr[k]->lvl[l]), (size_t)pyr[k]->len[l] * sizeof(uint32_t));
    f(reinterpret_cast<const void **>(&v.table), (((size_t)1 << (2 * v.P)) + 1) * sizeof(uint32_t));
}

}  // namespace

size_t rlz_index_footprint(const RlzIndexView &v) {
    RlzIndexView w = v;
    size_t total = 0;
    walk(w, [&](const void **, size_t bytes) { total += padded(bytes); });
    return total;
}

RlzIndexView rlz_index_copy_into(Context &ctx, const RlzIndexView &v, void *d_base) {
    RlzIndexView w = v;
    size_t at = 0;
    HIP_CHECK(hipMemsetAsync(d_base, 0, rlz_index_footprint(v), ctx.stream));  // (the padding is read, never used)
    walk(w, [&](const void **slot, size_t bytes) {
        void *dst = static_cast<char *>(d_base) + at;
        HIP_CHECK(hipMemcpyAsync(dst, *slot, bytes, hipMemcpyDeviceToDevice, ctx.stream));
        *slot = dst;
        at += padded(bytes);
    });
    // level 0 of each pyramid is its base array
    w.Plcp.lvl[0] = w.lcp;
    w.Pmin.lvl[0] = w.sa;
    if (w.with_rc) w.Pmax.lvl[0] = w.sa;
    else w.Pmax = w.Pmin;
    return w;
}

void rlz_index_search(Context &ctx, const RlzIndexView &ix, const PackedText &batch, uint32_t *d_len, uint32_t *d_rank) {
    const uint32_t n = batch.n;
    if (n == 0) return;
    // per position: its text window, a table pair, one SA entry and one window of X per bisection step (the extensions
    // come on top and depend on the data: the bytes are not stated)
    ProfScope ps(ctx.profiler(), "rlz_index_search", ctx.stream);
    rlz_index_search_kernel<<<(unsigned)div_up((size_t)n, kThreads), kThreads, 0, ctx.stream>>>(ix, batch.words, batch.terms,
                                                                                                 n, d_len, d_rank);
    KERNEL_CHECK();
}

void rlz_index_records(Context &ctx, const RlzIndexView &ix, const uint32_t *d_fpos, uint32_t z, const uint32_t *d_len,
                       const uint32_t *d_rank, IndexRec *d_out) {
    if (z == 0) return;
    ProfScope ps(ctx.profiler(), "rlz_index_records", ctx.stream, 36.0 * (double)z);
    rlz_index_record_kernel<false><<<(unsigned)div_up((size_t)z, kThreads), kThreads, 0, ctx.stream>>>(
        ix, d_fpos, z, const_cast<uint32_t *>(d_len), d_rank, d_out);
    KERNEL_CHECK();
}

void rlz_index_strands(Context &ctx, const RlzIndexView &ix, uint32_t n, uint32_t *d_len, const uint32_t *d_rank) {
    if (n == 0 || !ix.with_rc) return;
    ProfScope ps(ctx.profiler(), "rlz_index_strands", ctx.stream, 12.0 * (double)n);
    rlz_index_record_kernel<true><<<(unsigned)div_up((size_t)n, kThreads), kThreads, 0, ctx.stream>>>(ix, nullptr, n, d_len,
                                                                                                      d_rank, nullptr);
    KERNEL_CHECK();
}

}  // namespace nolzss
