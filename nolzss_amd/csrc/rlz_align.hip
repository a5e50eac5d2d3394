// rlz_align.hip -- base-level alignments of the seed chains on the relative-LZ index ("Relative-LZ index:
// base-level alignments"; the entry point: rlz_index_api.hip, nolzss_rlz_index_align; the rules: include/nolzss_hip.h).
//
// A chain of d anchors becomes d + 1 jobs: its left flank, the d - 1 gaps between consecutive anchors, its right flank.
// A job is a banded edit-distance rectangle of nq query bases by ny reference bases whose allowed diagonals, at most 64,
// are the lanes of ONE wavefront: lane l holds D[i][i + lo + l] of the current row i.  The diagonal predecessor is the
// lane's own value of the row before, the upper one that of lane l + 1, and the left one -- the only dependency inside a
// row -- is resolved by a 64-lane prefix minimum of v[l] - l (D[i][j] = l + min over l' <= l of (t[l'] - l'), t the
// minimum of the diagonal and upper candidates), six DPP steps and no LDS.  Every cell leaves a 2-bit direction by the
// tie rule (diagonal, then up, then left): two ballots per row, 16 bytes, written by one lane.  One lane per job walks
// them back; the ops of a chain follow from head flags over the code bytes and two scans.
//
// Both strands are served alike: on the reverse strand y is the coordinate in the mirrored block of X, where the
// alignment reads forward.  A left flank runs on the reversed strings: its texts are read downward.
//
// No kernel here spins, communicates between workgroups or uses an atomic; every loop bound is a job field clamped on
// load to the arrays it indexes.
#include "rlz_index.hpp"

#include "scan.hpp"

namespace nolzss {
namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
static_assert(kAlignLanes == 64, "the diagonals of a job are one wavefront");
constexpr int kInf = 1 << 30;  // an unreachable cell; a real D is below 2^28 + 64 (a target has less than 2^28 bases)

// ---- plan ----------------------------------------------------------------------------------------------------------
// The chain of anchor a: the largest c with offsets[c] <= a.  Loop: at most 32 halvings.
__device__ __forceinline__ uint32_t chain_of_anchor(const uint64_t *__restrict__ offsets, uint32_t C, uint32_t a) {
    uint32_t lo = 0, hi = C;  // offsets[lo] <= a < offsets[hi]
    while (hi - lo > 1) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (offsets[mid] <= a)
            lo = mid;
        else
            hi = mid;
    }
    return lo;
}

// first and end of the segment of a terminator table that holds position p (p below the table's end)
__device__ __forceinline__ void segment_of(const TermTable &t, uint32_t p, uint32_t &first, uint32_t &end) {
    uint32_t k = term_lower_bound(t, p);
    k = k < t.count ? k : t.count - 1;
    end = t.pos[k];
    first = k ? t.pos[k - 1] + 1u : 0u;
}

// One lane per chain anchor a < A.  Anchor i of chain c (anchors [o, o + d)) writes L' and, behind it, job o + c + 1 + i:
// the gap to anchor i + 1, or the right flank when it is the last.  The first anchor writes the left flank, job o + c.
// Loops: the chain search and two terminator searches, at most 32 steps each.
__global__ __launch_bounds__(kThreads) void rlz_align_plan_kernel(const ChainRec *__restrict__ chains,
                                                                  const uint64_t *__restrict__ offsets,
                                                                  const ChainAnchorRec *__restrict__ anchors, uint32_t C,
                                                                  uint32_t A, TermTable tterms, TermTable xterms, uint32_t nx,
                                                                  uint32_t B, uint32_t band, uint64_t max_flank,
                                                                  AlignJob *__restrict__ jobs, uint32_t *__restrict__ alen) {
    const uint64_t gid = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (gid >= A) return;
    const uint32_t a = (uint32_t)gid;
    const uint32_t c = chain_of_anchor(offsets, C, a);
    const uint64_t o64 = offsets[c], e64 = offsets[c + 1];
    const uint32_t o = o64 < A ? (uint32_t)o64 : a;  // (the chain's range lies inside the A anchors by construction)
    const uint32_t e = e64 <= A && e64 > a ? (uint32_t)e64 : a + 1;
    const uint32_t i = a - o, d = e - o;
    const ChainRec ch = chains[c];
    uint32_t k = (uint32_t)ch.target;
    k = k < tterms.count ? k : tterms.count - 1;
    const uint32_t tfirst = k ? tterms.pos[k - 1] + 1u : 0u;
    const uint32_t tlen = tterms.pos[k] - tfirst;
    const ChainAnchorRec an = anchors[a];
    const uint32_t q = (uint32_t)an.t_start, L = (uint32_t)an.length;
    uint64_t y64 = ch.is_rc ? 2ull * B + 1ull - an.position - an.length : an.position;
    const uint32_t y = y64 < nx ? (uint32_t)y64 : nx - 1;  // (a position of X by construction)
    const uint32_t jbase = o + c;
    uint32_t sfirst, send;
    segment_of(xterms, y, sfirst, send);
    if (i == 0) {
        AlignJob j = align_flank_job(kAlignLeft, tfirst + q, q, y, y - sfirst, band, max_flank);
        j.anchor = a;
        jobs[jbase] = j;
    }
    if (i + 1 < d) {
        const ChainAnchorRec nx_an = anchors[a + 1];
        const uint64_t yn = ch.is_rc ? 2ull * B + 1ull - nx_an.position - nx_an.length : nx_an.position;
        const int64_t dq = (int64_t)nx_an.t_start - (int64_t)q, dy = (int64_t)yn - (int64_t)y;
        int64_t keep = L;
        keep = keep < dq ? keep : dq;
        keep = keep < dy ? keep : dy;
        keep = keep > 0 ? keep : 0;  // (dq, dy >= 1 by the chain rules)
        const uint32_t Lp = (uint32_t)keep;
        const uint32_t gq = dq > keep ? (uint32_t)(dq - keep) : 0u, gy = dy > keep ? (uint32_t)(dy - keep) : 0u;
        AlignJob j = align_gap_job(tfirst + q + Lp, gq, y + Lp, gy, band);
        j.anchor = a + 1;
        alen[a] = Lp;
        jobs[jbase + 1u + i] = j;
    } else {
        const uint32_t qe = q + L < tlen ? q + L : tlen, ye = y + L < send ? y + L : send;
        AlignJob j = align_flank_job(kAlignRight, tfirst + qe, tlen - qe, ye, send - ye, band, max_flank);
        alen[a] = L;
        jobs[jbase + 1u + i] = j;
    }
}

// One lane per job: the DP rows it stores, its column slots (the most columns it can have, and one for the anchor behind
// it) and the most columns it and that anchor can have.  No loop.
__global__ __launch_bounds__(kThreads) void rlz_align_sizes_kernel(const AlignJob *__restrict__ jobs, uint32_t J,
                                                                   const uint32_t *__restrict__ alen, uint32_t A,
                                                                   uint32_t *__restrict__ rows, uint32_t *__restrict__ slots,
                                                                   uint32_t *__restrict__ weight) {
    const uint64_t gid = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (gid >= J) return;
    const AlignJob j = jobs[gid];
    const uint32_t cap = j.nq + j.ny;
    rows[gid] = j.dp ? j.nq : 0u;
    slots[gid] = cap + 1u;
    weight[gid] = cap + ((alen && j.anchor < A) ? alen[j.anchor] : 0u);
}

// ---- the recurrence ------------------------------------------------------------------------------------------------
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ int dpp_or(int old, int v) {  // lanes without a source, or outside the row mask, read `old`
    return __builtin_amdgcn_update_dpp(old, v, CTRL, ROW_MASK, 0xf, false);
}
__device__ __forceinline__ int imin(int a, int b) { return a < b ? a : b; }

// Inclusive prefix minimum over the 64 lanes: row_shr 1, 2, 4, 8 inside the rows of 16, then the last lane of row 0 / 2
// into row 1 / 3 (row_bcast:15) and lane 31 into rows 2 and 3 (row_bcast:31).  Values are at most kInf.
__device__ __forceinline__ int wave_prefix_min(int v) {
    v = imin(v, dpp_or<0x111, 0xf>(kInf, v));
    v = imin(v, dpp_or<0x112, 0xf>(kInf, v));
    v = imin(v, dpp_or<0x114, 0xf>(kInf, v));
    v = imin(v, dpp_or<0x118, 0xf>(kInf, v));
    v = imin(v, dpp_or<0x142, 0xa>(kInf, v));
    v = imin(v, dpp_or<0x143, 0xc>(kInf, v));
    return v;
}

__device__ __forceinline__ uint64_t wave_min_u64(uint64_t v) {  // every lane ends with the minimum; 6 steps
#pragma unroll
    for (int o = 32; o; o >>= 1) {
        const uint64_t w = (uint64_t)__shfl_xor((unsigned long long)v, o, 64);
        v = w < v ? w : v;
    }
    return v;
}

__device__ __forceinline__ uint32_t base_of(uint64_t word, uint32_t pos) {  // big-endian 2-bit codes, 32 per word
    return (uint32_t)(word >> (62u - 2u * (pos & 31u))) & 3u;
}

// One WAVEFRONT per job, kWaves per workgroup.  Lane l is diagonal d = lo + l and keeps D[i - 1][i - 1 + d] in `prev`
// (kInf outside the rectangle or the band).  Row i: the query base i - 1 is the same for every lane; lane l needs the
// reference base j - 1 = i - 1 + d, one further per row, so it keeps its current packed word and fetches another only
// when the position crosses a word boundary.  No text is read at a position outside the job's own ranges, which are
// checked against both texts before the first row.  Loops: nq rows; the end cell is a 64-lane minimum.
__global__ __launch_bounds__(kThreads) void rlz_align_dp_kernel(const AlignJob *__restrict__ jobs, uint32_t J,
                                                                const uint32_t *__restrict__ row_off, uint64_t R,
                                                                const uint64_t *__restrict__ qwords, uint32_t qn,
                                                                const uint64_t *__restrict__ xwords, uint32_t xn,
                                                                unsigned long long *__restrict__ dirs,
                                                                uint32_t *__restrict__ cost, uint32_t *__restrict__ endj) {
    const int l = (int)(threadIdx.x & 63u);
    const uint64_t gw = (uint64_t)blockIdx.x * kWaves + (threadIdx.x >> 6);
    if (gw >= J) return;  // (the whole wavefront)
    const uint32_t jn = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)gw);
    const AlignJob job = jobs[jn];
    const uint32_t nq = job.nq, ny = job.ny;
    const bool down = job.kind == kAlignLeft;
    const uint64_t r0 = row_off[jn];
    bool ok = job.dp && nq && ny && job.width >= 1 && job.width <= kAlignLanes && r0 <= R && nq <= R - r0;
    // the bases of the job lie inside the texts: [pos, pos + n) upward, (pos - n, pos] downward
    if (down)
        ok = ok && job.qpos < qn && nq <= job.qpos + 1u && job.ypos < xn && ny <= job.ypos + 1u;
    else
        ok = ok && job.qpos <= qn && nq <= qn - job.qpos && job.ypos <= xn && ny <= xn - job.ypos;
    if (!ok) {  // a job without recurrence: its cost and end column stand in the plan
        if (l == 0) {
            cost[jn] = job.dp ? 0u : job.cost;
            endj[jn] = job.dp ? 0u : job.endj;
        }
        return;
    }
    const int width = (int)job.width, lo = job.lo;
    const int d = lo + l;
    const bool lane_on = l < width;
    int prev = (lane_on && d >= 0 && (int64_t)d <= (int64_t)ny) ? d : kInf;  // D[0][d] = d
    uint64_t qw = 0, rw = 0;
    uint32_t qcur = 0xffffffffu, rcur = 0xffffffffu;
    for (uint32_t i = 1; i <= nq; ++i) {
        const uint32_t qp = down ? job.qpos - (i - 1u) : job.qpos + (i - 1u);
        if ((qp >> 5) != qcur) {
            qcur = qp >> 5;
            qw = qwords[qcur];
        }
        const uint32_t qb = base_of(qw, qp);
        const int64_t j = (int64_t)i + d;
        const bool valid = lane_on && j >= 0 && j <= (int64_t)ny;
        uint32_t rb = 4u;  // (no reference base: column 0 has no diagonal predecessor)
        if (lane_on && j >= 1 && j <= (int64_t)ny) {
            const uint32_t rp = down ? job.ypos - (uint32_t)(j - 1) : job.ypos + (uint32_t)(j - 1);
            if ((rp >> 5) != rcur) {
                rcur = rp >> 5;
                rw = xwords[rcur];
            }
            rb = base_of(rw, rp);
        }
        const int up_prev = dpp_or<0x130, 0xf>(kInf, prev);  // wave_shl:1 -- lane l reads lane l + 1, the last one kInf
        const int diagc = prev + (qb != rb ? 1 : 0);
        const int upc = up_prev + 1;
        const int t = valid ? imin(diagc, upc) : kInf;
        const int incl = wave_prefix_min(t - l);
        const int left_incl = dpp_or<0x138, 0xf>(kInf, incl);  // wave_shr:1 -- lane l reads lane l - 1, lane 0 kInf
        const int leftc = left_incl + l;                       // D[i][j - 1] + 1
        const int D = imin(t, leftc);
        // the first of diagonal, up, left that attains D: 0 `=`, 3 X, 1 up (I), 2 left (D)
        const int code = diagc == D ? (qb != rb ? 3 : 0) : (upc == D ? 1 : 2);
        const unsigned long long b0 = __ballot(valid && (code & 1)), b1 = __ballot(valid && (code & 2));
        if (l == 0) {
            ulonglong2 w;
            w.x = b0;
            w.y = b1;
            *reinterpret_cast<ulonglong2 *>(dirs + 2ull * (r0 + i - 1u)) = w;
        }
        prev = valid ? D : kInf;
    }
    // the end cell: (nq, ny) of a gap; of a flank the valid cell of row nq with the least D, then the least |j - nq|,
    // then the smaller j
    const int64_t j = (int64_t)nq + d;
    bool cand = lane_on && j >= 0 && j <= (int64_t)ny && prev < kInf;
    if (job.kind == kAlignGap) cand = cand && j == (int64_t)ny;
    const uint32_t ad = (uint32_t)(d < 0 ? -d : d) & 0x7fu;
    const uint64_t key = cand ? ((uint64_t)(uint32_t)prev << 16) | ((uint64_t)ad << 8) | (uint32_t)l : ~0ull;
    const uint64_t best = wave_min_u64(key);
    if (l == 0) {
        const bool found = best != ~0ull;
        cost[jn] = found ? (uint32_t)(best >> 16) : 0u;
        const int64_t je = (int64_t)nq + lo + (int64_t)(best & 0xffu);
        endj[jn] = found && je >= 0 && je <= (int64_t)ny ? (uint32_t)je : 0u;
    }
}

// ---- traceback -----------------------------------------------------------------------------------------------------
// One lane per job walks back from (nq, endj): in row 0 only left remains, in column 0 only up, elsewhere the stored
// direction of the cell's lane.  One code byte per column goes into the job's slots [col_off, col_off + nq + ny): back
// to front from their end for a gap and a right flank, front to back for a left flank, whose walk meets the columns in
// ascending q.  Loop: at most nq + ny steps.
__global__ __launch_bounds__(kThreads) void rlz_align_traceback_kernel(const AlignJob *__restrict__ jobs, uint32_t J,
                                                                       const uint32_t *__restrict__ row_off, uint64_t R,
                                                                       const uint32_t *__restrict__ col_off, uint64_t S,
                                                                       const unsigned long long *__restrict__ dirs,
                                                                       const uint32_t *__restrict__ endj,
                                                                       uint8_t *__restrict__ codes,
                                                                       uint32_t *__restrict__ ncols) {
    const uint64_t gid = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (gid >= J) return;
    const AlignJob job = jobs[gid];
    const uint64_t c0 = col_off[gid], r0 = row_off[gid];
    const uint32_t cap = job.nq + job.ny;
    uint32_t n = 0;
    if (c0 <= S && cap <= S - c0) {  // (the job's slots lie inside the S slots by construction)
        const bool stored = job.dp && r0 <= R && job.nq <= R - r0;
        const bool front = job.kind == kAlignLeft;
        uint32_t i = job.nq, j = endj[gid];
        j = j <= job.ny ? j : job.ny;
        while ((i | j) && n < cap) {
            uint32_t dir;
            if (i == 0)
                dir = 2u;
            else if (j == 0)
                dir = 1u;
            else {
                const int64_t l = (int64_t)j - (int64_t)i - job.lo;
                if (!stored || l < 0 || l > 63) break;  // (a cell of the band by construction)
                const unsigned long long *row = dirs + 2ull * (r0 + i - 1u);
                dir = (uint32_t)((row[0] >> l) & 1ull) | ((uint32_t)((row[1] >> l) & 1ull) << 1);
            }
            const uint8_t op = dir == 0u ? kAlignEq : (dir == 3u ? kAlignX : (dir == 1u ? kAlignI : kAlignD));
            codes[front ? c0 + n : c0 + (cap - 1u - n)] = op;
            ++n;
            if (dir != 2u) --i;
            if (dir != 1u) --j;
        }
    }
    ncols[gid] = n;
}

// ---- ops -----------------------------------------------------------------------------------------------------------
// One WAVEFRONT per job over its cap + 1 slots: flag = 1 where a run of equal codes begins, weight = the columns the slot
// stands for (a used column 1, the anchor's slot L', an unused slot 0).  The used columns are the first ncols slots of
// a left flank and the last ncols of the cap slots otherwise; slot cap is the `=` run of the anchor behind the job.  The
// column in front of a job's first used one is the anchor slot of the job before it -- always `=`, a left flank has
// none: there a chain begins.  Loop: the slots of the job, 64 per step.
__global__ __launch_bounds__(kThreads) void rlz_align_heads_kernel(const AlignJob *__restrict__ jobs, uint32_t J,
                                                                   const uint32_t *__restrict__ col_off, uint64_t S,
                                                                   const uint32_t *__restrict__ ncols,
                                                                   const uint32_t *__restrict__ alen, uint32_t A,
                                                                   const uint8_t *__restrict__ codes,
                                                                   uint32_t *__restrict__ flag, uint32_t *__restrict__ weight) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t gw = (uint64_t)blockIdx.x * kWaves + (threadIdx.x >> 6);
    if (gw >= J) return;  // (the whole wavefront)
    const uint32_t jn = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)gw);
    const AlignJob job = jobs[jn];
    const uint64_t c0 = col_off[jn];
    const uint32_t cap = job.nq + job.ny;
    if (c0 > S || (uint64_t)cap + 1u > S - c0) return;  // (the job's slots lie inside the S slots by construction)
    uint32_t n = ncols[jn];
    n = n < cap ? n : cap;
    const bool left = job.kind == kAlignLeft;
    const uint32_t first = left ? 0u : cap - n;  // the used slots: [first, first + n)
    for (uint32_t s = lane; s <= cap; s += 64u) {
        uint32_t fl = 0, w = 0;
        if (s == cap) {  // the anchor's run
            if (job.anchor < A) {
                w = alen[job.anchor];
                const uint32_t before = n ? codes[c0 + first + n - 1u] : (left ? 0u : kAlignEq);
                fl = before != kAlignEq ? 1u : 0u;
            }
        } else if (s >= first && s < first + n) {
            const uint32_t code = codes[c0 + s];
            const uint32_t before = s > first ? codes[c0 + s - 1u] : (left ? 0u : kAlignEq);
            w = 1u;
            fl = before != code ? 1u : 0u;
        }
        flag[c0 + s] = fl;
        weight[c0 + s] = w;
    }
}

// One lane per slot: a head writes the column position its run starts at, and its code, to its op.  No loop.
__global__ __launch_bounds__(kThreads) void rlz_align_runs_kernel(const uint32_t *__restrict__ flag,
                                                                  const uint32_t *__restrict__ slot,
                                                                  const uint32_t *__restrict__ wpos,
                                                                  const uint8_t *__restrict__ codes, uint64_t S, uint32_t nops,
                                                                  uint32_t *__restrict__ op_start, uint32_t *__restrict__ op_code) {
    const uint64_t gid = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (gid >= S || !flag[gid]) return;
    const uint32_t at = slot[gid];
    if (at >= nops) return;  // (a head has its op by construction)
    const uint32_t code = codes[gid];
    op_start[at] = wpos[gid];
    op_code[at] = code ? code : kAlignEq;  // (an anchor's slot holds no byte: its run is `=`)
}

// One lane per op: its length is the distance to the next run's start, or to the end of all columns.  No loop.
__global__ __launch_bounds__(kThreads) void rlz_align_ops_kernel(const uint32_t *__restrict__ op_start,
                                                                 const uint32_t *__restrict__ op_code, uint32_t nops,
                                                                 const uint32_t *__restrict__ d_totals,
                                                                 uint32_t *__restrict__ ops) {
    const uint64_t gid = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (gid >= nops) return;
    const uint32_t next = gid + 1 < nops ? op_start[gid + 1] : d_totals[1];
    const uint32_t len = (next - op_start[gid]) & 0x0fffffffu;  // (below 2^28: a target has less than 2^28 bases)
    ops[gid] = (len << 4) | (op_code[gid] & 0xfu);
}

// One lane per chain: the record.  The chain's slots begin at those of its left flank, job o + c; its ops and columns
// end where the next chain's begin, or at the totals.  Loop: the d + 1 job costs of the chain.
__global__ __launch_bounds__(kThreads) void rlz_align_records_kernel(const ChainRec *__restrict__ chains,
                                                                     const uint64_t *__restrict__ offsets,
                                                                     const ChainAnchorRec *__restrict__ anchors, uint32_t C,
                                                                     uint32_t A, const AlignJob *__restrict__ jobs, uint32_t J,
                                                                     const uint32_t *__restrict__ col_off, uint64_t S,
                                                                     const uint32_t *__restrict__ cost,
                                                                     const uint32_t *__restrict__ endj,
                                                                     const uint32_t *__restrict__ slot,
                                                                     const uint32_t *__restrict__ wpos,
                                                                     const uint32_t *__restrict__ d_totals, uint32_t B,
                                                                     AlignRec *__restrict__ recs, uint64_t *__restrict__ op_offsets) {
    const uint64_t gid = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (gid >= C) return;
    const uint32_t c = (uint32_t)gid;
    const ChainRec ch = chains[c];
    uint64_t o = offsets[c], e = offsets[c + 1];
    e = e <= A ? e : A;  // (anchors by construction)
    o = o < e ? o : (e ? e - 1 : 0);
    const uint32_t d = (uint32_t)(e - o);
    uint64_t jb = o + c, jnext = e + c + 1u;
    jb = jb < J ? jb : J - 1;  // (jobs by construction; J >= 1)
    const uint64_t jl = jb + d < J ? jb + d : J - 1;
    uint64_t s0 = col_off[jb], s1 = jnext < J ? col_off[jnext] : S;
    const uint32_t ops0 = s0 < S ? slot[s0] : d_totals[0], ops1 = s1 < S ? slot[s1] : d_totals[0];
    const uint32_t w0 = s0 < S ? wpos[s0] : d_totals[1], w1 = s1 < S ? wpos[s1] : d_totals[1];
    uint64_t edits = 0;
    for (uint64_t j = jb; j <= jl; ++j) edits += cost[j];
    const ChainAnchorRec a0 = anchors[o < A ? o : A - 1], a1 = anchors[e ? e - 1 : 0];
    const uint64_t y0 = ch.is_rc ? 2ull * B + 1ull - a0.position - a0.length : a0.position;
    const uint64_t y1 = ch.is_rc ? 2ull * B + 1ull - a1.position - a1.length : a1.position;
    const uint64_t y_begin = y0 - endj[jb], y_end = y1 + a1.length + endj[jl];
    AlignRec r;
    r.target = ch.target;
    r.t_start = a0.t_start - jobs[jb].nq;
    r.t_end = a1.t_start + a1.length + jobs[jl].nq;
    r.r_start = ch.is_rc ? 2ull * B + 1ull - y_end : y_begin;
    r.r_end = ch.is_rc ? 2ull * B + 1ull - y_begin : y_end;
    r.score = ch.score;
    r.edit_distance = edits;
    r.columns = w1 - w0;
    r.record = ch.record;
    r.is_rc = ch.is_rc;
    r.num_ops = ops1 - ops0;
    r.primary = ch.primary;
    recs[c] = r;
    op_offsets[c] = ops0;
    if (c == C - 1) op_offsets[C] = ops1;
}

}  // namespace

AlignJobs rlz_align_plan(Context &ctx, const RlzIndexView &ix, const PackedText &batch, const ChainsOut &chains, uint32_t band,
                         uint64_t max_flank) {
    AlignJobs out;
    const uint32_t C = chains.num_chains, A = chains.num_anchors;
    if (C == 0 || A == 0) return out;
    out.J = A + C;  // (A + C <= 2 A < 2^32: a hit total beyond 2^32 - 2^19 has been refused)
    AlignJob *jobs = ctx.arena.alloc<AlignJob>(out.J);
    uint32_t *alen = ctx.arena.alloc<uint32_t>(A);
    ProfScope ps(ctx.profiler(), "rlz_align_plan", ctx.stream, 100.0 * (double)A);
    rlz_align_plan_kernel<<<(unsigned)div_up((size_t)A, kThreads), kThreads, 0, ctx.stream>>>(
        chains.chains, chains.offsets, chains.anchors, C, A, batch.terms, ix.text.terms, ix.text.n, ix.B, band, max_flank, jobs,
        alen);
    KERNEL_CHECK();
    out.A = A;
    out.jobs = jobs;
    out.alen = alen;
    return out;
}

void rlz_align_sizes(Context &ctx, AlignJobs &a) {
    const uint32_t J = a.J;
    if (J == 0) return;
    hipStream_t s = ctx.stream;
    a.rows = ctx.arena.alloc<uint32_t>(J);
    a.slots = ctx.arena.alloc<uint32_t>(J);
    a.weight = ctx.arena.alloc<uint32_t>(J);
    uint64_t *d_sums = ctx.arena.alloc<uint64_t>(3);
    {
        ProfScope ps(ctx.profiler(), "rlz_align_sizes", s, 60.0 * (double)J);
        rlz_align_sizes_kernel<<<(unsigned)div_up((size_t)J, kThreads), kThreads, 0, s>>>(a.jobs, J, a.alen, a.alen ? a.A : 0u, a.rows,
                                                                                         a.slots, a.weight);
        KERNEL_CHECK();
    }
    rlz_index_rep_total(ctx, a.rows, J, d_sums);
    rlz_index_rep_total(ctx, a.slots, J, d_sums + 1);
    rlz_index_rep_total(ctx, a.weight, J, d_sums + 2);
    uint64_t sums[3] = {0, 0, 0};
    HIP_CHECK(hipMemcpyAsync(sums, d_sums, sizeof sums, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));  // (sums is a local)
    a.total_rows = sums[0];
    a.total_slots = sums[1];
    a.total_weight = sums[2];
}

void rlz_align_layout(Context &ctx, AlignJobs &a) {
    const uint32_t J = a.J;
    if (J == 0) return;
    hipStream_t s = ctx.stream;
    a.row_off = ctx.arena.alloc<uint32_t>(J);
    a.col_off = ctx.arena.alloc<uint32_t>(J);
    a.cost = ctx.arena.alloc<uint32_t>(J);
    a.endj = ctx.arena.alloc<uint32_t>(J);
    a.ncols = ctx.arena.alloc<uint32_t>(J);
    a.dirs = ctx.arena.alloc<unsigned long long>(2 * (size_t)a.total_rows + 2);
    a.codes = ctx.arena.alloc<uint8_t>((size_t)a.total_slots);
    ProfScope ps(ctx.profiler(), "rlz_align_offsets", s, 16.0 * (double)J + (double)a.total_slots);
    scan_exclusive_add_u32(a.rows, a.row_off, J, nullptr, ctx.arena, s);
    scan_exclusive_add_u32(a.slots, a.col_off, J, nullptr, ctx.arena, s);
    HIP_CHECK(hipMemsetAsync(a.codes, 0, (size_t)a.total_slots, s));
}

void rlz_align_dp(Context &ctx, const AlignJobs &a, const PackedText &qt, const PackedText &xt) {
    if (a.J == 0) return;
    ProfScope ps(ctx.profiler(), "rlz_align_dp", ctx.stream, 16.0 * (double)a.total_rows + 60.0 * (double)a.J);
    rlz_align_dp_kernel<<<(unsigned)div_up((size_t)a.J, kWaves), kThreads, 0, ctx.stream>>>(
        a.jobs, a.J, a.row_off, a.total_rows, qt.words, qt.n, xt.words, xt.n, a.dirs, a.cost, a.endj);
    KERNEL_CHECK();
}

void rlz_align_traceback(Context &ctx, const AlignJobs &a) {
    if (a.J == 0) return;
    ProfScope ps(ctx.profiler(), "rlz_align_traceback", ctx.stream, 16.0 * (double)a.total_rows + (double)a.total_slots);
    rlz_align_traceback_kernel<<<(unsigned)div_up((size_t)a.J, kThreads), kThreads, 0, ctx.stream>>>(
        a.jobs, a.J, a.row_off, a.total_rows, a.col_off, a.total_slots, a.dirs, a.endj, a.codes, a.ncols);
    KERNEL_CHECK();
}

AlignOut rlz_align_ops(Context &ctx, const AlignJobs &a, const ChainsOut &chains, const ChainRules &rules) {
    AlignOut out;
    const uint32_t C = chains.num_chains, A = chains.num_anchors, J = a.J;
    if (C == 0 || J == 0) return out;
    hipStream_t s = ctx.stream;
    const size_t S = (size_t)a.total_slots;
    uint32_t *flag = ctx.arena.alloc<uint32_t>(S), *weight = ctx.arena.alloc<uint32_t>(S);
    uint32_t *slot = ctx.arena.alloc<uint32_t>(S), *wpos = ctx.arena.alloc<uint32_t>(S);
    uint32_t *d_totals = ctx.arena.alloc<uint32_t>(2);
    {
        ProfScope ps(ctx.profiler(), "rlz_align_heads", s, 9.0 * (double)S + 60.0 * (double)J);
        rlz_align_heads_kernel<<<(unsigned)div_up((size_t)J, kWaves), kThreads, 0, s>>>(a.jobs, J, a.col_off, S, a.ncols, a.alen, A,
                                                                                       a.codes, flag, weight);
        KERNEL_CHECK();
        scan_exclusive_add_u32(flag, slot, S, d_totals, ctx.arena, s);
        scan_exclusive_add_u32(weight, wpos, S, d_totals + 1, ctx.arena, s);
    }
    uint32_t totals[2] = {0, 0};
    HIP_CHECK(hipMemcpyAsync(totals, d_totals, sizeof totals, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));  // (totals is a local)
    const uint32_t nops = totals[0];
    if (nops < C || nops > S || totals[1] > a.total_weight)
        throw HipError("rlz align: fewer ops than chains, more ops than slots, or more columns than planned");
    uint32_t *op_start = ctx.arena.alloc<uint32_t>(nops), *op_code = ctx.arena.alloc<uint32_t>(nops);
    uint32_t *ops = ctx.arena.alloc<uint32_t>(nops);
    AlignRec *recs = ctx.arena.alloc<AlignRec>(C);
    uint64_t *op_offsets = ctx.arena.alloc<uint64_t>((size_t)C + 1);
    {
        ProfScope ps(ctx.profiler(), "rlz_align_ops", s, 9.0 * (double)S + 20.0 * (double)nops);
        rlz_align_runs_kernel<<<(unsigned)div_up(S, (size_t)kThreads), kThreads, 0, s>>>(flag, slot, wpos, a.codes, S, nops,
                                                                                        op_start, op_code);
        KERNEL_CHECK();
        rlz_align_ops_kernel<<<(unsigned)div_up((size_t)nops, kThreads), kThreads, 0, s>>>(op_start, op_code, nops, d_totals, ops);
        KERNEL_CHECK();
    }
    {
        ProfScope ps(ctx.profiler(), "rlz_align_records", s, 200.0 * (double)C + 4.0 * (double)J);
        rlz_align_records_kernel<<<(unsigned)div_up((size_t)C, kThreads), kThreads, 0, s>>>(
            chains.chains, chains.offsets, chains.anchors, C, A, a.jobs, J, a.col_off, S, a.cost, a.endj, slot, wpos, d_totals,
            rules.B, recs, op_offsets);
        KERNEL_CHECK();
    }
    out.num_alignments = C;
    out.num_ops = nops;
    out.recs = recs;
    out.op_offsets = op_offsets;
    out.ops = ops;
    return out;
}

}  // namespace nolzss
