// rlz.hip -- relative Lempel-Ziv: every target factorized against the reference block and nothing else
// ("Relative LZ against a reference block").
//
// The prepared string is  Rblk s T1 s .. Tk s [pad] rc-block s  (rlz_api.hip).  A suffix is FLAGGED for the forward
// strand when it starts inside Rblk (position < B) and for the reverse-complement strand when it starts inside the
// mirrored block (position >= E).  The longest match of the suffix of rank r with any flagged suffix is the range
// minimum of lcp[] towards the NEAREST flagged rank above or below (range minima only shrink as the range grows), so
//
//   up[r]   = min lcp[j + 1 .. r],  j = nearest flagged rank below r   (0 without one)
//   down[r] = min lcp[r + 1 .. j],  j = nearest flagged rank above r   (0 without one)
//   L[r]    = max(up[r], down[r])   per strand,  code = Lf >= Lr ? Lf : Lr | 1 << 31
//
// Both are scans of one monoid over the pairs (sa[r], lcp[r]).  An element is (hf, val): hf = a flagged rank has been
// passed, val = the minimum LCP since the last one (over everything when hf = 0); x followed by y is
// y.hf ? y : (x.hf, min(x.val, y.val)).  Ascending the element of rank r is (flag[r], flag[r] ? inf : lcp[r]) and
// up[r] = min(prefix before r applied to "nothing seen", lcp[r]); descending it is (flag[r], lcp[r]) and down[r] = the
// prefix before r.  The scans have the reduce-then-scan shape of scan.hip -- tile aggregates, a scan of the aggregates,
// apply -- with both directions and both strands served by one read of the tile: 8 + 8 bytes read and 4 written per
// rank.  There is no search and no fallback: a source inside Rblk can never run into a target position.
#include "pipeline.hpp"
#include "text_order.hpp"

namespace nolzss {
namespace {

constexpr int kThreads = 256;
constexpr int kItems = 4;  // consecutive ranks per lane: one 16-byte load per array
constexpr int kRows = 4;
constexpr int kTile = kThreads * kItems * kRows;  // 4096
constexpr int kCarryThreads = 1024;
constexpr uint32_t kInf = 0xffffffffu;

struct Seg {
    uint32_t hf, val;
};
// NS strands side by side: forward only, or forward and reverse complement
template <int NS> struct St {
    Seg s[NS];
};

__device__ __forceinline__ Seg seg_then(Seg x, Seg y) { return y.hf ? y : Seg{x.hf, x.val < y.val ? x.val : y.val}; }
template <int NS> __device__ __forceinline__ St<NS> st_identity() {
    St<NS> r;
#pragma unroll
    for (int k = 0; k < NS; ++k) r.s[k] = Seg{0u, kInf};
    return r;
}
template <int NS> __device__ __forceinline__ St<NS> st_then(const St<NS> &x, const St<NS> &y) {
    St<NS> r;
#pragma unroll
    for (int k = 0; k < NS; ++k) r.s[k] = seg_then(x.s[k], y.s[k]);
    return r;
}
template <int NS> __device__ __forceinline__ St<NS> st_unpack(uint4 v) {
    St<NS> r;
    r.s[0] = Seg{v.x, v.y};
    if (NS > 1) r.s[NS - 1] = Seg{v.z, v.w};
    return r;
}
template <int NS> __device__ __forceinline__ uint4 st_pack(const St<NS> &v) {
    return make_uint4(v.s[0].hf, v.s[0].val, NS > 1 ? v.s[NS - 1].hf : 0u, NS > 1 ? v.s[NS - 1].val : kInf);
}

// strand k of a suffix start: 0 = inside the reference block, 1 = inside the mirrored block
__device__ __forceinline__ bool flagged(int k, uint32_t pos, uint32_t B, uint32_t E) { return k == 0 ? pos < B : pos >= E; }

// the element of one rank: ascending (kBack = false) a flagged rank starts a new minimum behind itself, descending its
// own lcp entry already belongs to the ranks below
template <int NS, bool kBack>
__device__ __forceinline__ St<NS> element(uint32_t pos, uint32_t l, uint32_t B, uint32_t E) {
    St<NS> r;
#pragma unroll
    for (int k = 0; k < NS; ++k) {
        const bool f = flagged(k, pos, B, E);
        r.s[k] = Seg{f ? 1u : 0u, (f && !kBack) ? kInf : l};
    }
    return r;
}

// Inclusive scan across the wavefront in processing order (kBack: from lane 63 down).  The hf halves come from one
// ballot; the val halves are a segmented minimum by doubling that stops at the nearest lane with hf set.
template <bool kBack> __device__ __forceinline__ Seg wave_scan(Seg v) {
    const int lane = lane_id();
    const uint64_t flags = __ballot(v.hf != 0u);
    const uint64_t mine = kBack ? (flags & ~((1ull << lane) - 1ull)) : (flags & ((2ull << lane) - 1ull));
    const int start = mine ? (kBack ? __ffsll((long long)mine) - 1 : 63 - __clzll((long long)mine)) : (kBack ? 63 : 0);
    uint32_t x = v.val;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t o = kBack ? __shfl_down(x, d, 64) : __shfl_up(x, d, 64);
        const bool in = kBack ? lane + d <= start : lane - d >= start;
        if (in && o < x) x = o;
    }
    return Seg{mine ? 1u : 0u, x};
}

// Exclusive scan of one element per thread across NW wavefronts in processing order; lds holds NS * NW entries.
// Every thread must call it (two barriers).  total = all threads.
template <int NS, int NW, bool kBack>
__device__ __forceinline__ St<NS> block_scan(const St<NS> &v, Seg *lds, St<NS> &total) {
    const int lane = lane_id(), w = threadIdx.x >> 6;
    St<NS> inc;
#pragma unroll
    for (int k = 0; k < NS; ++k) inc.s[k] = wave_scan<kBack>(v.s[k]);
    if (lane == (kBack ? 0 : 63)) {
#pragma unroll
        for (int k = 0; k < NS; ++k) lds[k * NW + w] = inc.s[k];
    }
    __syncthreads();
    St<NS> prefix = st_identity<NS>(), tot = st_identity<NS>();
#pragma unroll
    for (int j = 0; j < NW; ++j) {
        const int q = kBack ? NW - 1 - j : j;
        St<NS> a;
#pragma unroll
        for (int k = 0; k < NS; ++k) a.s[k] = lds[k * NW + q];
        if (kBack ? q > w : q < w) prefix = st_then<NS>(prefix, a);
        tot = st_then<NS>(tot, a);
    }
    __syncthreads();
    St<NS> exc;
#pragma unroll
    for (int k = 0; k < NS; ++k) {
        exc.s[k].hf = kBack ? __shfl_down(inc.s[k].hf, 1, 64) : __shfl_up(inc.s[k].hf, 1, 64);
        exc.s[k].val = kBack ? __shfl_down(inc.s[k].val, 1, 64) : __shfl_up(inc.s[k].val, 1, 64);
        if (lane == (kBack ? 63 : 0)) exc.s[k] = Seg{0u, kInf};
    }
    total = tot;
    return st_then<NS>(prefix, exc);
}

// The tile of a workgroup in registers: row `row` of lane t holds the ranks base + (row * 256 + t) * 4 .. + 3.  Ranks
// at or beyond m are the identity of both directions: position B is in neither block, their lcp is inf.
struct TileRegs {
    uint32_t pos[kRows][kItems], l[kRows][kItems];
};
__device__ __forceinline__ void load_tile(const uint32_t *__restrict__ sa, const uint32_t *__restrict__ lcp, uint32_t m,
                                          uint32_t B, size_t base, TileRegs &t) {
#pragma unroll
    for (int row = 0; row < kRows; ++row) {
        const size_t idx = base + ((size_t)row * kThreads + threadIdx.x) * kItems;
        if (idx + kItems <= m) {  // (the arrays come from the arena, 256-byte aligned, and idx is a multiple of 4)
            const uint4 a = *reinterpret_cast<const uint4 *>(sa + idx);
            const uint4 b = *reinterpret_cast<const uint4 *>(lcp + idx);
            t.pos[row][0] = a.x, t.pos[row][1] = a.y, t.pos[row][2] = a.z, t.pos[row][3] = a.w;
            t.l[row][0] = b.x, t.l[row][1] = b.y, t.l[row][2] = b.z, t.l[row][3] = b.w;
        } else {
#pragma unroll
            for (int e = 0; e < kItems; ++e) {
                const bool in = idx + e < m;
                t.pos[row][e] = in ? sa[idx + e] : B;
                t.l[row][e] = in ? lcp[idx + e] : kInf;
            }
        }
    }
}

// agg[tile] = the ascending aggregate of the tile, agg[nb + tile] = the descending one
template <int NS>
__global__ __launch_bounds__(kThreads) void rlz_reduce_kernel(const uint32_t *__restrict__ sa,
                                                              const uint32_t *__restrict__ lcp, uint32_t m, uint32_t B,
                                                              uint32_t E, uint4 *__restrict__ agg, uint32_t nb) {
    constexpr int NW = kThreads / 64;
    __shared__ Seg lds[2][NS][kRows][NW];
    TileRegs t;
    load_tile(sa, lcp, m, B, (size_t)blockIdx.x * kTile, t);
    const int lane = lane_id(), w = threadIdx.x >> 6;
#pragma unroll
    for (int row = 0; row < kRows; ++row) {
        St<NS> up = st_identity<NS>(), down = st_identity<NS>();
#pragma unroll
        for (int e = 0; e < kItems; ++e) {
            up = st_then<NS>(up, element<NS, false>(t.pos[row][e], t.l[row][e], B, E));
            down = st_then<NS>(down, element<NS, true>(t.pos[row][kItems - 1 - e], t.l[row][kItems - 1 - e], B, E));
        }
#pragma unroll
        for (int k = 0; k < NS; ++k) {
            const Seg u = wave_scan<false>(up.s[k]), d = wave_scan<true>(down.s[k]);
            if (lane == 63) lds[0][k][row][w] = u;
            if (lane == 0) lds[1][k][row][w] = d;
        }
    }
    __syncthreads();
    if (threadIdx.x < 2) {
        const bool back = threadIdx.x == 1;
        St<NS> acc = st_identity<NS>();
        for (int j = 0; j < kRows * NW; ++j) {
            const int q = back ? kRows * NW - 1 - j : j;
            St<NS> a;
#pragma unroll
            for (int k = 0; k < NS; ++k) a.s[k] = lds[back ? 1 : 0][k][q / NW][q % NW];
            acc = st_then<NS>(acc, a);
        }
        agg[(back ? nb : 0u) + blockIdx.x] = st_pack<NS>(acc);
    }
}

// Exclusive scan of the tile aggregates, workgroup 0 ascending, workgroup 1 descending: every thread takes a contiguous
// run of tiles (in processing order), the runs are scanned across the workgroup, and a second walk writes the carries.
template <int NS>
__global__ __launch_bounds__(kCarryThreads) void rlz_carry_kernel(const uint4 *__restrict__ agg, uint4 *__restrict__ carry,
                                                                  uint32_t nb) {
    constexpr int NW = kCarryThreads / 64;
    __shared__ Seg lds[NS * NW];
    const bool back = blockIdx.x == 1;
    const uint4 *in = agg + (back ? nb : 0u);
    uint4 *out = carry + (back ? nb : 0u);
    const uint32_t per = (nb + kCarryThreads - 1) / kCarryThreads;
    const uint32_t lo = threadIdx.x * per < nb ? threadIdx.x * per : nb, hi = lo + per < nb ? lo + per : nb;
    St<NS> loc = st_identity<NS>();
    for (uint32_t i = lo; i < hi; ++i) loc = st_then<NS>(loc, st_unpack<NS>(in[back ? nb - 1u - i : i]));
    St<NS> total;
    St<NS> run = block_scan<NS, NW, false>(loc, lds, total);
    for (uint32_t i = lo; i < hi; ++i) {
        const uint32_t q = back ? nb - 1u - i : i;
        out[q] = st_pack<NS>(run);
        run = st_then<NS>(run, st_unpack<NS>(in[q]));
    }
}

template <int NS>
__global__ __launch_bounds__(kThreads) void rlz_apply_kernel(const uint32_t *__restrict__ sa,
                                                             const uint32_t *__restrict__ lcp, uint32_t m, uint32_t B,
                                                             uint32_t E, const uint4 *__restrict__ carry, uint32_t nb,
                                                             uint32_t *__restrict__ code) {
    constexpr int NW = kThreads / 64;
    __shared__ Seg lds[NS * NW];
    const size_t base = (size_t)blockIdx.x * kTile;
    TileRegs t;
    load_tile(sa, lcp, m, B, base, t);
    uint32_t up[NS][kRows][kItems];
    St<NS> run = st_unpack<NS>(carry[blockIdx.x]);
#pragma unroll
    for (int row = 0; row < kRows; ++row) {
        St<NS> loc = st_identity<NS>();
#pragma unroll
        for (int e = 0; e < kItems; ++e) loc = st_then<NS>(loc, element<NS, false>(t.pos[row][e], t.l[row][e], B, E));
        St<NS> total;
        St<NS> pre = st_then<NS>(run, block_scan<NS, NW, false>(loc, lds, total));
#pragma unroll
        for (int e = 0; e < kItems; ++e) {
            const uint32_t l = t.l[row][e];
#pragma unroll
            for (int k = 0; k < NS; ++k) {
                const uint32_t before = pre.s[k].hf ? pre.s[k].val : 0u;
                up[k][row][e] = before < l ? before : l;
            }
            pre = st_then<NS>(pre, element<NS, false>(t.pos[row][e], l, B, E));
        }
        run = st_then<NS>(run, total);
    }
    run = st_unpack<NS>(carry[nb + blockIdx.x]);
#pragma unroll
    for (int row = kRows - 1; row >= 0; --row) {
        St<NS> loc = st_identity<NS>();
#pragma unroll
        for (int e = kItems - 1; e >= 0; --e) loc = st_then<NS>(loc, element<NS, true>(t.pos[row][e], t.l[row][e], B, E));
        St<NS> total;
        St<NS> pre = st_then<NS>(run, block_scan<NS, NW, true>(loc, lds, total));
        uint32_t out[kItems];
#pragma unroll
        for (int e = kItems - 1; e >= 0; --e) {
            uint32_t len[NS];
#pragma unroll
            for (int k = 0; k < NS; ++k) {
                const uint32_t down = pre.s[k].hf ? pre.s[k].val : 0u;
                len[k] = down > up[k][row][e] ? down : up[k][row][e];
            }
            // forward wins ties; bit 31 = reverse complement
            out[e] = (NS == 1 || len[0] >= len[NS - 1]) ? len[0] : (len[NS - 1] | 0x80000000u);
            pre = st_then<NS>(pre, element<NS, true>(t.pos[row][e], t.l[row][e], B, E));
        }
        const size_t idx = base + ((size_t)row * kThreads + threadIdx.x) * kItems;
        if (idx + kItems <= m) {
            *reinterpret_cast<uint4 *>(code + idx) = make_uint4(out[0], out[1], out[2], out[3]);
        } else {
#pragma unroll
            for (int e = 0; e < kItems; ++e)
                if (idx + e < m) code[idx + e] = out[e];
        }
        run = st_then<NS>(run, total);
    }
}

template <int NS>
void launch_candidates(const uint32_t *sa, const uint32_t *lcp, uint32_t m, uint32_t B, uint32_t E, uint4 *agg, uint4 *carry,
                       uint32_t nb, uint32_t *by_rank, hipStream_t s) {
    rlz_reduce_kernel<NS><<<nb, kThreads, 0, s>>>(sa, lcp, m, B, E, agg, nb);
    KERNEL_CHECK();
    rlz_carry_kernel<NS><<<2, kCarryThreads, 0, s>>>(agg, carry, nb);
    KERNEL_CHECK();
    rlz_apply_kernel<NS><<<nb, kThreads, 0, s>>>(sa, lcp, m, B, E, carry, nb, by_rank);
    KERNEL_CHECK();
}

// counts[j] = factor starts inside [lo[j], hi[j]) of the ascending list fpos
__global__ __launch_bounds__(kThreads) void rlz_count_kernel(const uint32_t *__restrict__ fpos, uint32_t z,
                                                             const uint32_t *__restrict__ bounds, uint32_t k,
                                                             uint32_t *__restrict__ counts) {
    const uint32_t j = blockIdx.x * kThreads + threadIdx.x;
    if (j >= k) return;
    uint32_t at[2];
    for (int side = 0; side < 2; ++side) {
        const uint32_t x = bounds[2 * j + side];
        uint32_t lo = 0, hi = z;
        while (lo < hi) {
            const uint32_t mid = lo + (hi - lo) / 2;
            if (fpos[mid] < x) lo = mid + 1;
            else hi = mid;
        }
        at[side] = lo;
    }
    counts[j] = at[1] - at[0];
}

}  // namespace

void rlz_candidates(Context &ctx, const uint32_t *sa, const uint32_t *lcp, uint32_t m, uint32_t B, uint32_t E, bool with_rc,
                    uint32_t *by_rank) {
    if (m == 0) return;
    Arena &arena = ctx.arena;
    hipStream_t s = ctx.stream;
    const size_t mark = arena.mark();
    const uint32_t nb = (uint32_t)div_up(m, kTile);
    uint4 *agg = arena.alloc<uint4>(2 * (size_t)nb), *carry = arena.alloc<uint4>(2 * (size_t)nb);
    {
        // two reads of (sa, lcp), one write of the codes; the aggregates are written, scanned and read once each
        ProfScope ps(ctx.profiler(), "rlz_candidates", s, 20.0 * (double)m + 128.0 * (double)nb);
        if (with_rc) launch_candidates<2>(sa, lcp, m, B, E, agg, carry, nb, by_rank, s);
        else launch_candidates<1>(sa, lcp, m, B, E, agg, carry, nb, by_rank, s);
    }
    arena.rewind(mark);
}

void rlz_count_per_target(Context &ctx, const uint32_t *d_fpos, uint32_t z, const uint32_t *d_bounds, uint32_t k,
                          uint32_t *d_counts) {
    if (k == 0) return;
    rlz_count_kernel<<<(unsigned)div_up(k, kThreads), kThreads, 0, ctx.stream>>>(d_fpos, z, d_bounds, k, d_counts);
    KERNEL_CHECK();
}

void run_rlz_pipeline(Context &ctx, const uint8_t *d_S, const RlzLayout &lay, ChainRequest &rq, uint32_t *h_codes) {
    Arena &arena = ctx.arena;
    hipStream_t s = ctx.stream;
    const PackedText text = pack_text(ctx, d_S, lay.total);  // segmented at 2 bits, as the multi-FASTA strings
    const uint32_t m = text.n;
    uint32_t *sa = arena.alloc<uint32_t>(m);
    uint32_t *isa = arena.alloc<uint32_t>(m);
    uint32_t *lcp = arena.alloc<uint32_t>((size_t)m + 1);
    build_suffix_array(ctx, text, sa, isa, lcp);
    const Pyramid Plcp = build_lcp_pyramid(ctx, text, sa, lcp);
    Pyramid Pmin, Pmax;
    {
        ProfScope ps(ctx.profiler(), "pyramids", s);
        Pmin = build_pyramid(sa, m, false, arena, s);
        Pmax = lay.with_rc ? build_pyramid(sa, m, true, arena, s) : Pmin;
    }
    // code[] spans all of S so that rank order -> text order is a permutation; only target positions mean anything
    uint32_t *code = arena.alloc<uint32_t>(m);
    {
        const size_t mark = arena.mark();
        uint32_t *by_rank = arena.alloc<uint32_t>(m);
        uint32_t *scratch_idx = arena.alloc<uint32_t>(m), *scratch_val = arena.alloc<uint32_t>(m);
        rlz_candidates(ctx, sa, lcp, m, lay.block_length, lay.with_rc ? lay.rc_block_start : kInf, lay.with_rc, by_rank);
        {
            ProfScope ps(ctx.profiler(), "rlz_text_order", s, 12.0 * (double)m);
            uint32_t *idx[2] = {sa, scratch_idx};
            uint32_t *val[2] = {by_rank, scratch_val};
            bucketed_scatter(idx, val, m, code, m, arena, s, ctx.profiler(), true, /*keep_val=*/false);
        }
        arena.rewind(mark);
    }
    if (h_codes && lay.chain_end) {
        HIP_CHECK(hipMemcpyAsync(h_codes, code, (size_t)lay.chain_end * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipStreamSynchronize(s));
    }
    // min SA over I(L) lies in Rblk (the block comes first), max SA in the mirrored block (it comes last), and
    // 2 rcN - max SA - L + 1 with 2 rcN = B - 1 + E is the leftmost forward coordinate
    RecordLookup lookup{sa, isa, lcp, Pmin, Plcp};
    if (lay.with_rc) {
        lookup.Pmax = &Pmax;
        lookup.rcN = lay.rcN;
    }
    chain_outputs(ctx, mark_chain(ctx, lay.chain_end, lay.block_length + 1u, LstarCodes::of(code)), lookup, lay.with_rc, rq);
}

}  // namespace nolzss
