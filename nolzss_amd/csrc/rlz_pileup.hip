// rlz_pileup.hip -- pileup counts and variant sites of the alignments on the relative-LZ index (DESIGN.md 5,
// "Relative-LZ index: pileup"; the entry points: rlz_pileup_api.hip, nolzss_rlz_pileup_*; the rules:
// include/nolzss_hip.h).
//
// The accumulation runs behind rlz_align_ops on what that left in the arena: the alignment records, op_offsets, the ops
// and the packed batch.  Two exclusive scans over the ops give every op the target bases and the block bases consumed in
// front of it; minus the values at its alignment's first op they are its place inside the alignment.  An op finds its
// alignment by bisecting op_offsets.  Almost every column of real data is a `=` column, and every block base under a
// reverse-strand alignment counts for REV: both are kept as DIFFERENCE entries in wrapping u32 -- +1 at the first
// position of a run, -1 just past its last -- two atomics per `=` op and two per reverse-strand alignment, whatever
// their length.  X, D, I and BREAK are bounded by the edit distance and the number of alignments: one atomic per column
// (X, D) or per op (I) or per alignment end (BREAK) on dense counters.  A read resolves the difference entries by one
// scan each (the handle keeps a dirty flag) and composes the eight channels: the `=` depth of a position is credited to
// the channel of the block's own base.  Every I op also appends one event -- position, length, the first 64 bases -- to the
// handle's insertion log (the allele table and the consensus over it: rlz_consensus.hip), and on request D and I ops are
// counted at their leftmost block position ("Relative-LZ index: consensus"): a shift is a bounded walk over
// the block by the op's own lane, and the `=` columns it moves are difference entries again.
//
// No kernel here spins or communicates between workgroups; every loop bound is a field clamped on load to the arrays it
// indexes, and no position outside [r_start, r_end) of an op's alignment is written (the -1 of a difference entry
// falls at r_end <= B, which is why the arrays hold B + 1 entries).
#include "rlz_pileup_device.hpp"

#include "scan.hpp"

namespace nolzss {
namespace {

constexpr int kThreads = 256;
constexpr size_t kAlign = 256;  // bytes: every array of a view starts on such a boundary

// The alignment of op i: the largest c with op_offsets[c] <= i.  Loop: at most 32 halvings.
__device__ __forceinline__ uint32_t alignment_of_op(const uint64_t *__restrict__ op_offsets, uint32_t C, uint32_t i) {
    uint32_t lo = 0, hi = C;  // op_offsets[lo] <= i < op_offsets[hi]
    while (hi - lo > 1) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (op_offsets[mid] <= i)
            lo = mid;
        else
            hi = mid;
    }
    return lo;
}

// What the kernels take of an alignment record, clamped on load: kept is false for an alignment that is skipped
// (primary_only) or whose coordinates leave the block, its target or the batch (none by construction).
struct Geometry {
    bool kept;
    uint32_t r_start, r_end;  // 0 <= r_start < r_end <= B
    uint32_t t_at, t_span;    // the batch position of t_start, and t_end - t_start
    bool rc, clip_front, clip_back;  // clip_*: the target has bases in front of / behind the aligned part, in q
};
__device__ __forceinline__ Geometry geometry_of(const AlignRec &r, const TermTable &tt, uint32_t qn, uint32_t B,
                                                bool primary_only) {
    Geometry g;
    g.kept = false;
    g.r_start = g.r_end = g.t_at = g.t_span = 0;
    g.rc = r.is_rc != 0;
    g.clip_front = g.clip_back = false;
    if (tt.count < 2 || r.target >= (uint64_t)(tt.count - 1)) return g;
    const uint32_t k = (uint32_t)r.target;
    const uint32_t tfirst = k ? tt.pos[k - 1] + 1u : 0u, tend = tt.pos[k];
    if (tend < tfirst || tend > qn) return g;
    const uint64_t tlen = tend - tfirst;
    if (!(r.r_start < r.r_end && r.r_end <= (uint64_t)B && r.t_start <= r.t_end && r.t_end <= tlen)) return g;
    if (primary_only && !r.primary) return g;
    g.kept = true;
    g.r_start = (uint32_t)r.r_start;
    g.r_end = (uint32_t)r.r_end;
    g.t_at = tfirst + (uint32_t)r.t_start;
    g.t_span = (uint32_t)(r.t_end - r.t_start);
    g.clip_front = r.t_start > 0;
    g.clip_back = r.t_end < tlen;
    return g;
}

// One lane per op: the target bases and the block bases it consumes.  No loop.
__global__ __launch_bounds__(kThreads) void rlz_pileup_sizes_kernel(const uint32_t *__restrict__ ops, uint32_t nops,
                                                                    uint32_t *__restrict__ tq, uint32_t *__restrict__ rq) {
    const uint64_t gid = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (gid >= nops) return;
    const uint32_t op = ops[gid], code = op & 0xfu, len = op >> 4;
    tq[gid] = code == kAlignD ? 0u : len;
    rq[gid] = code == kAlignI ? 0u : len;
}

// One lane per alignment: the REV span of a reverse-strand alignment as a difference entry, BREAK at either end, and
// the kept alignments with their ops and columns summed per wavefront -- one atomic per wavefront and total.  No loop.
__global__ __launch_bounds__(kThreads) void rlz_pileup_alignments_kernel(const AlignRec *__restrict__ recs, uint32_t C,
                                                                         TermTable tt, uint32_t qn, PileupView v,
                                                                         bool primary_only,
                                                                         unsigned long long *__restrict__ stats) {
    const uint64_t gid = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    unsigned long long kept = 0, nops = 0, cols = 0;
    if (gid < C) {
        const AlignRec r = recs[gid];
        const Geometry g = geometry_of(r, tt, qn, v.B, primary_only);
        if (g.kept) {
            kept = 1;
            nops = r.num_ops;
            cols = r.columns;
            if (g.rc) {
                atomicAdd(v.diff_rev + g.r_start, 1u);
                atomicAdd(v.diff_rev + g.r_end, 0xffffffffu);
            }
            // in forward-block orientation the walk of a reverse-strand alignment begins at the target's end
            const bool at_start = g.rc ? g.clip_back : g.clip_front, at_end = g.rc ? g.clip_front : g.clip_back;
            if (at_start) atomicAdd(v.brk + g.r_start, 1u);
            if (at_end) atomicAdd(v.brk + (g.r_end - 1u), 1u);
        }
    }
#pragma unroll
    for (int o = 32; o; o >>= 1) {
        kept += __shfl_xor(kept, o, 64);
        nops += __shfl_xor(nops, o, 64);
        cols += __shfl_xor(cols, o, 64);
    }
    if ((threadIdx.x & 63u) == 0 && kept) {
        atomicAdd(stats, kept);
        atomicAdd(stats + 1, nops);
        atomicAdd(stats + 2, cols);
    }
}

// The length of the `=` op in front of op i in forward-block orientation -- op i - 1 on the forward strand, op i + 1 on
// the reverse strand, inside the alignment's ops [o0, o_end) --, 0 if there is none or it has another code.  No loop.
__device__ __forceinline__ uint32_t eq_run_before(const uint32_t *__restrict__ ops, uint32_t i, uint32_t o0, uint32_t o_end,
                                                  bool rc) {
    if (rc ? i + 1u >= o_end : i <= o0) return 0u;
    const uint32_t op = ops[rc ? i + 1u : i - 1u];
    return (op & 0xfu) == kAlignEq ? op >> 4 : 0u;
}

// The shift of a deletion of n >= 1 block bases at [r, r + n): the largest s <= L with X[r - j] == X[r + n - j] for all
// 1 <= j <= s.  The caller has made sure that L <= r and L <= kPileupMaxShift.  Loop: at most L steps.
__device__ __forceinline__ uint32_t deletion_shift(const uint64_t *__restrict__ xwords, uint32_t r, uint32_t n, uint32_t L) {
    uint32_t s = 0;
    while (s < L) {
        const uint32_t a = r - s - 1u, b = a + n;
        if (base_of(xwords[a >> 5], a) != base_of(xwords[b >> 5], b)) break;
        ++s;
    }
    return s;
}

// One lane per op i < nops.  T and R: the target and block bases its alignment consumes in front of it.  Its block
// positions are r_start + R + j on the forward strand and r_end - 1 - (R + j) on the reverse strand, j < n, where n is
// the op's length clamped to what is left of [r_start, r_end) -- and, for X and I, of the aligned part of the target.
// With kPileupNormalize a D or an I op behind an `=` op moves left by its shift s (at most kPileupMaxShift, and never
// in front of r_start); the `=` op in front of a D gives up its last s positions, which the D op counts behind the gap.
// Every I op appends one event to the log, clamped to its capacity.
// Loops: the bisection; the n columns of an X or a D op; a shift (at most kPileupMaxShift steps); the kPileupInsBases
// bases of an event.
__global__ __launch_bounds__(kThreads) void rlz_pileup_ops_kernel(const AlignRec *__restrict__ recs,
                                                                  const uint64_t *__restrict__ op_offsets, uint32_t C,
                                                                  const uint32_t *__restrict__ ops, uint32_t nops,
                                                                  const uint32_t *__restrict__ tpre,
                                                                  const uint32_t *__restrict__ rpre,
                                                                  const uint64_t *__restrict__ qwords, TermTable tt,
                                                                  uint32_t qn, PileupView v, bool primary_only,
                                                                  const uint64_t *__restrict__ xwords, PileupLog log,
                                                                  unsigned long long *__restrict__ logged) {
    const uint64_t gid = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (gid >= nops) return;
    const uint32_t i = (uint32_t)gid;
    const uint32_t c = alignment_of_op(op_offsets, C, i);
    const uint64_t o64 = op_offsets[c];
    if (o64 > i) return;  // (an op of no alignment: none by construction)
    const uint32_t o0 = (uint32_t)o64;
    const uint64_t e64 = op_offsets[c + 1u];
    const uint32_t o_end = e64 < (uint64_t)nops ? (uint32_t)e64 : nops;
    const Geometry g = geometry_of(recs[c], tt, qn, v.B, primary_only);
    if (!g.kept) return;
    const uint32_t T = tpre[i] - tpre[o0], R = rpre[i] - rpre[o0];
    const uint32_t span = g.r_end - g.r_start;
    const uint32_t op = ops[i], code = op & 0xfu;
    const bool normalize = (log.flags & kPileupNormalize) != 0;
    uint32_t n = op >> 4;
    if (code == kAlignI) {  // once per op, at the base in front of the walk: clamp(r - s - 1, r_start, r_end - 1)
        const uint32_t Rc = R < span ? R : span;
        const uint32_t r = g.rc ? g.r_end - Rc : g.r_start + Rc;
        // the op's ni target bases, W in forward-block orientation: W[j] is the batch position below, complemented on
        // the reverse strand (t_at + T + ni <= the target's end <= qn)
        const uint32_t ni = T < g.t_span ? (n < g.t_span - T ? n : g.t_span - T) : 0u;
        auto wbase = [&](uint32_t j) {
            const uint32_t tp = g.rc ? g.t_at + T + (ni - 1u - j) : g.t_at + T + j;
            const uint32_t b = base_of(qwords[tp >> 5], tp);
            return g.rc ? 3u - b : b;
        };
        uint32_t s = 0;
        if (normalize && ni) {
            uint32_t L = eq_run_before(ops, i, o0, o_end, g.rc);
            L = L < kPileupMaxShift ? L : kPileupMaxShift;
            L = L < r - g.r_start ? L : r - g.r_start;
            while (s < L) {  // each step rotates the inserted string by one: X[r - j] against W[(ni - j) mod ni]
                const uint32_t j = s + 1u, a = r - j;
                if (base_of(xwords[a >> 5], a) != wbase((ni - j % ni) % ni)) break;
                ++s;
            }
        }
        const uint32_t rs = r - s;
        uint32_t at = rs > g.r_start ? rs - 1u : g.r_start;
        at = at < g.r_end - 1u ? at : g.r_end - 1u;
        atomicAdd(v.ins + at, 1u);
        const uint64_t slot = log.base + atomicAdd(logged, 1ull);
        if (slot >= log.capacity) return;  // (none by construction: the capacity was secured for the counted events)
        PileupEvent ev;
        ev.position = at;
        ev.length = n;
        ev.bases[0] = ev.bases[1] = 0;
        const uint32_t m = ni < kPileupInsBases ? ni : kPileupInsBases, back = ni ? ni - s % ni : 0u;
        for (uint32_t j = 0; j < m; ++j)  // W'[j] = W[(j - s) mod ni]
            ev.bases[j >> 5] |= (uint64_t)wbase((j + back) % ni) << (62u - 2u * (j & 31u));
        log.events[slot] = ev;
        return;
    }
    if (code != kAlignEq && code != kAlignX && code != kAlignD) return;
    if (R >= span) return;
    n = n < span - R ? n : span - R;
    if (code == kAlignX) {
        if (T >= g.t_span) return;
        n = n < g.t_span - T ? n : g.t_span - T;
    }
    if (n == 0) return;
    const uint32_t lo = g.rc ? g.r_end - R - n : g.r_start + R;  // the op's positions are [lo, lo + n)
    if (code == kAlignEq) {
        uint32_t keep = n;
        if (normalize && (g.rc ? i > o0 : i + 1u < o_end)) {  // a D op behind it takes the positions it shifts over
            const uint32_t next = ops[g.rc ? i - 1u : i + 1u];
            uint32_t nd = next >> 4;
            nd = nd < g.r_end - (lo + n) ? nd : g.r_end - (lo + n);
            if ((next & 0xfu) == kAlignD && nd)
                keep = n - deletion_shift(xwords, lo + n, nd, n < kPileupMaxShift ? n : kPileupMaxShift);
        }
        if (keep == 0) return;
        atomicAdd(v.diff_eq + lo, 1u);
        atomicAdd(v.diff_eq + (lo + keep), 0xffffffffu);  // (lo + keep <= r_end <= B: the arrays hold B + 1 entries)
    } else if (code == kAlignD) {
        uint32_t s = 0;
        if (normalize) {
            uint32_t L = eq_run_before(ops, i, o0, o_end, g.rc);
            L = L < kPileupMaxShift ? L : kPileupMaxShift;
            L = L < lo - g.r_start ? L : lo - g.r_start;
            s = deletion_shift(xwords, lo, n, L);
        }
        for (uint32_t j = 0; j < n; ++j) atomicAdd(v.del + (lo - s + j), 1u);
        if (s) {  // the `=` columns that moved behind the gap: [lo - s + n, lo + n), the block's own base
            atomicAdd(v.diff_eq + (lo - s + n), 1u);
            atomicAdd(v.diff_eq + (lo + n), 0xffffffffu);
        }
    } else {
        const uint32_t t0 = g.t_at + T;  // (t0 + n <= the target's end <= qn)
        uint64_t w = 0;
        uint32_t cur = 0xffffffffu;
        for (uint32_t j = 0; j < n; ++j) {
            const uint32_t tp = t0 + j;
            if ((tp >> 5) != cur) {
                cur = tp >> 5;
                w = qwords[cur];
            }
            const uint32_t b = base_of(w, tp);
            const uint32_t p = g.rc ? g.r_end - 1u - (R + j) : g.r_start + R + j;
            atomicAdd(v.xbase + (4ull * p + (g.rc ? 3u - b : b)), 1u);
        }
    }
}

// One lane per op: the I ops of the kept alignments, summed per wavefront -- one atomic per wavefront.  Loop: the
// bisection.
__global__ __launch_bounds__(kThreads) void rlz_pileup_count_insertions_kernel(const AlignRec *__restrict__ recs,
                                                                               const uint64_t *__restrict__ op_offsets,
                                                                               uint32_t C, const uint32_t *__restrict__ ops,
                                                                               uint32_t nops, TermTable tt, uint32_t qn,
                                                                               uint32_t B, bool primary_only,
                                                                               unsigned long long *__restrict__ total) {
    const uint64_t gid = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    unsigned long long mine = 0;
    if (gid < nops && (ops[gid] & 0xfu) == kAlignI) {
        const uint32_t c = alignment_of_op(op_offsets, C, (uint32_t)gid);
        if (op_offsets[c] <= gid && geometry_of(recs[c], tt, qn, B, primary_only).kept) mine = 1;
    }
#pragma unroll
    for (int o = 32; o; o >>= 1) mine += __shfl_xor(mine, o, 64);
    if ((threadIdx.x & 63u) == 0 && mine) atomicAdd(total, mine);
}

// One lane per position of [start, start + count): its eight words, two 16-byte stores.  Loop: the separator search.
__global__ __launch_bounds__(kThreads) void rlz_pileup_compose_kernel(PileupView v, const uint64_t *__restrict__ xwords,
                                                                      TermTable xt, uint32_t start, uint32_t count,
                                                                      uint32_t *__restrict__ out) {
    const uint64_t gid = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (gid >= count) return;
    const uint32_t p = start + (uint32_t)gid;  // (start + count <= B: the caller's check)
    uint32_t first, ch[kPileupChannels];
    bool separator;
    block_record_of(xt, p, first, separator);
    channels_of(v, xwords, separator, p, ch);
    uint4 *o = reinterpret_cast<uint4 *>(out + 8ull * gid);
    o[0] = make_uint4(ch[0], ch[1], ch[2], ch[3]);
    o[1] = make_uint4(ch[4], ch[5], ch[6], ch[7]);
}

// The alleles a variants query reports at a position with block base b, bit a for allele a: the three other bases and
// DEL against depth = A + C + G + T + DEL, INS against the same depth; the products in 64 bits.
__device__ __forceinline__ uint32_t variant_mask(const uint32_t ch[kPileupChannels], uint32_t b, const PileupRule &rule,
                                                 uint32_t &depth) {
    const uint64_t d64 = (uint64_t)ch[0] + ch[1] + ch[2] + ch[3] + ch[4];  // (below 2^32: at most 2^31 - 1 targets, two each)
    depth = (uint32_t)d64;
    uint32_t mask = 0;
#pragma unroll
    for (uint32_t a = 0; a < 6u; ++a) {
        if (a == b) continue;
        const uint64_t n = ch[a];
        if (n >= rule.min_count && n * rule.den >= rule.num * d64) mask |= 1u << a;
    }
    return mask;
}

// One lane per block position: the records it will write.  Loop: the separator search.
__global__ __launch_bounds__(kThreads) void rlz_pileup_variant_flags_kernel(PileupView v, const uint64_t *__restrict__ xwords,
                                                                            TermTable xt, PileupRule rule,
                                                                            uint32_t *__restrict__ nrec) {
    const uint64_t gid = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (gid >= v.B) return;
    const uint32_t p = (uint32_t)gid;
    uint32_t first, ch[kPileupChannels], depth;
    bool separator;
    block_record_of(xt, p, first, separator);
    const uint32_t b = channels_of(v, xwords, separator, p, ch);
    nrec[p] = separator ? 0u : (uint32_t)__popc(variant_mask(ch, b, rule, depth));
}

// One lane per block position: those of its records that fall into [first, first + count) go to out, in allele order.
// Loops: the separator search; the six alleles.
__global__ __launch_bounds__(kThreads) void rlz_pileup_variant_records_kernel(PileupView v, const uint64_t *__restrict__ xwords,
                                                                              TermTable xt, PileupRule rule,
                                                                              const uint32_t *__restrict__ off, uint64_t first,
                                                                              uint32_t count, PileupVariantRec *__restrict__ out) {
    const uint64_t gid = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (gid >= v.B) return;
    const uint32_t p = (uint32_t)gid;
    uint64_t at = off[p];
    if (at >= first + count) return;  // (the offsets ascend: nothing of this position is wanted)
    uint32_t rec_first, ch[kPileupChannels], depth;
    bool separator;
    const uint32_t record = block_record_of(xt, p, rec_first, separator);
    if (separator) return;
    const uint32_t b = channels_of(v, xwords, separator, p, ch);
    const uint32_t mask = variant_mask(ch, b, rule, depth);
#pragma unroll
    for (uint32_t a = 0; a < 6u; ++a) {
        if (!(mask & (1u << a))) continue;
        if (at >= first && at < first + count) {
            PileupVariantRec r;
            r.position = p;
            r.record_offset = p - rec_first;
            r.record = record;
            r.ref_base = b;
            r.allele = a;
            r.count = ch[a];
            r.depth = depth;
            r.rev = ch[6];
            out[at - first] = r;
        }
        ++at;
    }
}

size_t padded(size_t bytes) { return (bytes + kAlign - 1) / kAlign * kAlign; }

}  // namespace

size_t rlz_pileup_footprint(uint32_t B) { return kPileupArrays * padded(sizeof(uint32_t) * ((size_t)B + 1)); }

PileupView rlz_pileup_view(void *d_base, uint32_t B) {
    const size_t step = padded(sizeof(uint32_t) * ((size_t)B + 1));
    char *at = static_cast<char *>(d_base);
    auto take = [&](size_t arrays) {
        uint32_t *p = reinterpret_cast<uint32_t *>(at);
        at += arrays * step;
        return p;
    };
    PileupView v;
    v.B = B;
    v.diff_eq = take(1);
    v.diff_rev = take(1);
    v.depth_eq = take(1);
    v.depth_rev = take(1);
    v.xbase = take(4);
    v.del = take(1);
    v.ins = take(1);
    v.brk = take(1);
    return v;
}

void rlz_pileup_count_insertions(Context &ctx, const AlignOut &a, const PackedText &batch, uint32_t B, bool primary_only,
                                 unsigned long long *d_count) {
    hipStream_t s = ctx.stream;
    HIP_CHECK(hipMemsetAsync(d_count, 0, sizeof(unsigned long long), s));
    const uint32_t C = a.num_alignments, N = a.num_ops;
    if (C == 0 || N == 0) return;
    ProfScope ps(ctx.profiler(), "rlz_pileup_log_count", s, 4.0 * (double)N);
    rlz_pileup_count_insertions_kernel<<<(unsigned)div_up((size_t)N, kThreads), kThreads, 0, s>>>(
        a.recs, a.op_offsets, C, a.ops, N, batch.terms, batch.n, B, primary_only, d_count);
    KERNEL_CHECK();
}

void rlz_pileup_accumulate(Context &ctx, const PileupView &v, const AlignOut &a, const PackedText &batch,
                           const PackedText &block, bool primary_only, const PileupLog &log, unsigned long long *d_stats) {
    hipStream_t s = ctx.stream;
    HIP_CHECK(hipMemsetAsync(d_stats, 0, kPileupStats * sizeof(unsigned long long), s));
    const uint32_t C = a.num_alignments, N = a.num_ops;
    if (C == 0 || N == 0) return;
    uint32_t *tq = ctx.arena.alloc<uint32_t>(N), *rq = ctx.arena.alloc<uint32_t>(N);
    uint32_t *tpre = ctx.arena.alloc<uint32_t>(N), *rpre = ctx.arena.alloc<uint32_t>(N);
    {
        ProfScope ps(ctx.profiler(), "rlz_pileup_scans", s, 28.0 * (double)N);
        rlz_pileup_sizes_kernel<<<(unsigned)div_up((size_t)N, kThreads), kThreads, 0, s>>>(a.ops, N, tq, rq);
        KERNEL_CHECK();
        scan_exclusive_add_u32(tq, tpre, N, nullptr, ctx.arena, s);
        scan_exclusive_add_u32(rq, rpre, N, nullptr, ctx.arena, s);
    }
    ProfScope ps(ctx.profiler(), "rlz_pileup_accumulate", s, 80.0 * (double)C + 20.0 * (double)N);
    rlz_pileup_alignments_kernel<<<(unsigned)div_up((size_t)C, kThreads), kThreads, 0, s>>>(a.recs, C, batch.terms, batch.n, v,
                                                                                           primary_only, d_stats);
    KERNEL_CHECK();
    rlz_pileup_ops_kernel<<<(unsigned)div_up((size_t)N, kThreads), kThreads, 0, s>>>(a.recs, a.op_offsets, C, a.ops, N, tpre, rpre,
                                                                                    batch.words, batch.terms, batch.n, v,
                                                                                    primary_only, block.words, log, d_stats + 3);
    KERNEL_CHECK();
}

void rlz_pileup_resolve(Context &ctx, const PileupView &v) {
    ProfScope ps(ctx.profiler(), "rlz_pileup_resolve", ctx.stream, 16.0 * ((double)v.B + 1.0));
    scan_exclusive_add_u32(v.diff_eq, v.depth_eq, (size_t)v.B + 1, nullptr, ctx.arena, ctx.stream);
    scan_exclusive_add_u32(v.diff_rev, v.depth_rev, (size_t)v.B + 1, nullptr, ctx.arena, ctx.stream);
}

void rlz_pileup_compose(Context &ctx, const PileupView &v, const PackedText &block, uint32_t start, uint32_t count,
                        uint32_t *d_out) {
    if (count == 0) return;
    ProfScope ps(ctx.profiler(), "rlz_pileup_counts", ctx.stream, 68.0 * (double)count);
    rlz_pileup_compose_kernel<<<(unsigned)div_up((size_t)count, kThreads), kThreads, 0, ctx.stream>>>(v, block.words, block.terms,
                                                                                                     start, count, d_out);
    KERNEL_CHECK();
}

void rlz_pileup_variant_flags(Context &ctx, const PileupView &v, const PackedText &block, const PileupRule &rule, uint32_t *d_n) {
    if (v.B == 0) return;
    ProfScope ps(ctx.profiler(), "rlz_pileup_variant_flags", ctx.stream, 40.0 * (double)v.B);
    rlz_pileup_variant_flags_kernel<<<(unsigned)div_up((size_t)v.B, kThreads), kThreads, 0, ctx.stream>>>(v, block.words, block.terms,
                                                                                                         rule, d_n);
    KERNEL_CHECK();
}

void rlz_pileup_variant_records(Context &ctx, const PileupView &v, const PackedText &block, const PileupRule &rule,
                                const uint32_t *d_off, uint64_t first, uint32_t count, PileupVariantRec *d_out) {
    if (v.B == 0 || count == 0) return;
    ProfScope ps(ctx.profiler(), "rlz_pileup_variant_records", ctx.stream, 40.0 * (double)v.B + 40.0 * (double)count);
    rlz_pileup_variant_records_kernel<<<(unsigned)div_up((size_t)v.B, kThreads), kThreads, 0, ctx.stream>>>(
        v, block.words, block.terms, rule, d_off, first, count, d_out);
    KERNEL_CHECK();
}

}  // namespace nolzss
