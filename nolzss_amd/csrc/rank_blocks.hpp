// rank_blocks.hpp -- SA and LCP of 16 consecutive ranks in ONE 128-byte line, and the interval search of the factor
// records over such lines (chain.hip: factor_block_kernel; written by lpf_tile_kernel, lpnf.hip).
//
// A factor record needs the interval I(L) = [lo, hi] of ranks around r = ISA[i] whose suffixes share L symbols --
// lo = the nearest entry at or below r with lcp < L, hi + 1 = the nearest entry above r with lcp < L -- and the minimum
// of SA over it.  With lcp[] and sa[] in two arrays even the shortest interval costs two to three lines around one
// rank; here the interval of nearly every factor lies in the one to three lines around r, read whole and decided in
// registers.  The search itself is plain C++ over caller-supplied loads, so that a host program can run it against
// the entry-by-entry loops (tests/host/rank_blocks_test.cpp).
#pragma once
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define NOLZSS_RB_FN __host__ __device__ __forceinline__
#else
#define NOLZSS_RB_FN inline
#endif

namespace nolzss {

constexpr int kRankBlockShift = 4;
constexpr uint32_t kRankBlock = 1u << kRankBlockShift;

// Block b holds the ranks 16 b .. 16 b + 15 with the indexing of the arrays it copies (lcp[0] = 0; lcp[n] = 0 is the
// entry that stops the upward scan).  Behind the last entry: lcp = 0, sa = 0xffffffff (neutral for the minimum).
// The array is 128-byte aligned: one block is one line.
struct RankBlock {
    uint32_t sa[kRankBlock];
    uint32_t lcp[kRankBlock];
};
static_assert(sizeof(RankBlock) == 128, "one block is one 128-byte line");

// ceil((n + 1) / 16): the block that holds lcp[n] included
inline size_t rank_block_count(size_t n) { return (n + kRankBlock) >> kRankBlockShift; }

// bit j set iff lcp[j] < L (entry j stops a scan for L)
NOLZSS_RB_FN uint32_t rb_stop_mask(const RankBlock &B, uint32_t L) {
    uint32_t m = 0;
#pragma unroll
    for (int j = 0; j < (int)kRankBlock; ++j) m |= (B.lcp[j] < L ? 1u : 0u) << j;
    return m;
}
// min of sa[j] over the entries whose bit is set (no dynamic index: the block stays in registers)
NOLZSS_RB_FN uint32_t rb_min_sa(const RankBlock &B, uint32_t entries) {
    uint32_t mn = 0xffffffffu;
#pragma unroll
    for (int j = 0; j < (int)kRankBlock; ++j) {
        const uint32_t v = ((entries >> j) & 1u) ? B.sa[j] : 0xffffffffu;
        mn = v < mn ? v : mn;
    }
    return mn;
}
NOLZSS_RB_FN uint32_t rb_top_bit(uint32_t m) { return 31u - (uint32_t)__builtin_clz(m); }     // m != 0
NOLZSS_RB_FN uint32_t rb_bottom_bit(uint32_t m) { return (uint32_t)__builtin_ctz(m); }        // m != 0
NOLZSS_RB_FN uint32_t rb_min(uint32_t a, uint32_t b) { return a < b ? a : b; }

// The interval of a factor of length L >= 1 at rank r, and min SA over it, in three steps: the block of r, then the
// neighbouring block on each side on which the block of r holds no stop, then -- only if the neighbour holds none
// either -- the rest from where the blocks end:
//   far_left(q, L)   -> the largest rank <= q with lcp < L        (q >= 15; exists: lcp[0] = 0)
//   far_right(q, L)  -> the smallest rank >= q with lcp < L       (q <= n; exists: lcp[n] = 0)
//   range_min(a, b)  -> min sa[a .. b], a <= b
// lo, hi and the minimum are those of the entry-by-entry scans.  (Block 0 stops every downward scan at lcp[0] and the
// last block every upward one at lcp[n] or at the padding: a neighbour that is asked for exists.)
struct RankInterval {
    uint32_t lo, hi, mn;
    bool need_left, need_right;  // the block of r has no stop at or below r / above r
};
NOLZSS_RB_FN RankInterval rb_centre(const RankBlock &C, uint32_t r, uint32_t L) {
    const uint32_t b = r >> kRankBlockShift, j = r & (kRankBlock - 1u);
    const uint32_t stop = rb_stop_mask(C, L);
    const uint32_t upto_r = (2u << j) - 1u;
    const uint32_t below = stop & upto_r, above = stop & ~upto_r;      // stops at or below r / above r
    const uint32_t lj = below ? rb_top_bit(below) : 0u;                // first entry of the interval in this block
    const uint32_t hj = above ? rb_bottom_bit(above) - 1u : kRankBlock - 1u;  // last one (above has no bit <= j)
    RankInterval S;
    S.lo = (b << kRankBlockShift) + lj;
    S.hi = (b << kRankBlockShift) + hj;
    S.mn = rb_min_sa(C, ((2u << hj) - 1u) & ~((1u << lj) - 1u));
    S.need_left = below == 0u;
    S.need_right = above == 0u;
    return S;
}
// Lb = block bl = (r >> 4) - 1, for an interval with need_left
template <typename FarLeft, typename RangeMin>
NOLZSS_RB_FN void rb_left(RankInterval &S, const RankBlock &Lb, uint32_t bl, uint32_t L, FarLeft far_left, RangeMin range_min) {
    const uint32_t s = rb_stop_mask(Lb, L);
    const uint32_t q = s ? rb_top_bit(s) : 0u;
    S.mn = rb_min(S.mn, rb_min_sa(Lb, 0xffffu & ~((1u << q) - 1u)));
    S.lo = (bl << kRankBlockShift) + q;
    if (!s) {
        const uint32_t edge = (bl << kRankBlockShift) - 1u;  // (bl >= 1: block 0 has a stop)
        S.lo = far_left(edge, L);
        S.mn = rb_min(S.mn, range_min(S.lo, edge));
    }
}
// Rb = block br = (r >> 4) + 1, for an interval with need_right
template <typename FarRight, typename RangeMin>
NOLZSS_RB_FN void rb_right(RankInterval &S, const RankBlock &Rb, uint32_t br, uint32_t L, FarRight far_right, RangeMin range_min) {
    const uint32_t s = rb_stop_mask(Rb, L);
    const uint32_t q = s ? rb_bottom_bit(s) : kRankBlock;  // entries 0 .. q - 1 of the neighbour belong
    S.mn = rb_min(S.mn, rb_min_sa(Rb, (1u << q) - 1u));
    S.hi = (br << kRankBlockShift) + q - 1u;
    if (!s) {
        const uint32_t edge = (br + 1u) << kRankBlockShift;
        S.hi = far_right(edge, L) - 1u;
        if (S.hi >= edge) S.mn = rb_min(S.mn, range_min(edge, S.hi));
    }
}
// The three steps for one rank, load(b) -> RankBlock b (the host test's form; the kernel loads the blocks of a whole
// wavefront between the steps).
template <typename Load, typename FarLeft, typename FarRight, typename RangeMin>
NOLZSS_RB_FN RankInterval rank_block_interval(uint32_t r, uint32_t L, Load load, FarLeft far_left, FarRight far_right,
                                              RangeMin range_min) {
    const uint32_t b = r >> kRankBlockShift;
    RankInterval S = rb_centre(load(b), r, L);
    if (S.need_left) rb_left(S, load(b - 1u), b - 1u, L, far_left, range_min);
    if (S.need_right) rb_right(S, load(b + 1u), b + 1u, L, far_right, range_min);
    return S;
}

}  // namespace nolzss
