// rlz_seed_chain.hip -- colinear chains of the seeds of every target on the relative-LZ index ("Relative-LZ
// index: colinear seed chains"; the entry point: rlz_index_api.hip, nolzss_rlz_index_seed_chains; the rules:
// include/nolzss_hip.h).
//
// Every reported hit of every seed is an anchor (q, y, L): q the seed's start inside its target, y the coordinate of the
// occurrence in the index text X -- the mirrored block's coordinate on the reverse strand, the value rlz_seed_hits_kernel
// read from the suffix array --, so that a colinear alignment ascends in q and in y on either strand.  The anchors are
// sorted by (target, group, y), group = is_rc * m + record, and a group is walked in that order by ONE wavefront whose 64
// lanes hold the last 64 anchors as a ring: the look-back of the recurrence is the width of the wavefront.
//
// Scores stay below 2^32: along a chain f grows by at most dq per link, so f(i) <= L(first) + q(i) - q(first), and the
// callers admit only q + L < 2^31 (a target of 2^31 bases or more is refused, rlz_index_api.hip; the debug hook checks
// its anchors).  The candidates are compared in signed 64 bits all the same.
//
// No kernel here spins, communicates between workgroups or uses an atomic; every loop is bounded by a data size.
#include "rlz_index.hpp"

#include <algorithm>

#include "radix_sort.hpp"
#include "scan.hpp"

namespace nolzss {
namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
static_assert(kChainLookback == 64, "the ring of the recurrence is one wavefront");

// The reported hits of all seeds summed in 64 bits (a 32-bit scan would wrap where the total has to be refused), in two
// launches: every workgroup sums its stride of rep into out[blockIdx.x], then ONE workgroup sums those (parts = the number
// of workgroups of the first launch, at most kTotalParts).  Loops: count / (256 * workgroups) strided loads per lane; the
// tree over the 256 partial sums, 8 steps.
constexpr unsigned kTotalParts = 256;
template <typename T>
__global__ __launch_bounds__(kThreads) void rlz_chain_total_kernel(const T *__restrict__ in, uint32_t count,
                                                                   uint64_t *__restrict__ out) {
    __shared__ uint64_t part[kThreads];
    uint64_t sum = 0;
    for (uint64_t j = (uint64_t)blockIdx.x * kThreads + threadIdx.x; j < count; j += (uint64_t)gridDim.x * kThreads) sum += in[j];
    part[threadIdx.x] = sum;
    __syncthreads();
    for (int w = kThreads / 2; w; w >>= 1) {
        if ((int)threadIdx.x < w) part[threadIdx.x] += part[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[blockIdx.x] = part[0];
}

// One lane per sorted hit slot t < T of LocateSorted: key = (seed << 33) | (position << 1) | is_rc, value = the record.
// The seed gives q and L: its batch position p = seeds[j], L = len[p], and the next terminator's index is the target.
// out_keys[t] = (target << 40) | (group << 32) | y, out_vals[t] = t, q and L by slot.  Loop: the terminator search, at
// most 32 steps.
__global__ __launch_bounds__(kThreads) void rlz_chain_keys_kernel(TermTable tterms, uint32_t n, uint32_t nx, uint32_t B,
                                                                  uint32_t records, const uint32_t *__restrict__ seeds,
                                                                  const uint32_t *__restrict__ len, uint32_t S,
                                                                  const uint64_t *__restrict__ keys,
                                                                  const uint32_t *__restrict__ vals, uint32_t T,
                                                                  uint64_t *__restrict__ out_keys,
                                                                  uint32_t *__restrict__ out_vals,
                                                                  uint32_t *__restrict__ slot_q,
                                                                  uint32_t *__restrict__ slot_len) {
    const uint64_t gid = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (gid >= T) return;
    const uint32_t t = (uint32_t)gid;
    const uint64_t key = keys[t];
    uint32_t j = (uint32_t)(key >> 33);
    j = j < S ? j : S - 1;  // (a seed by construction: no key can lead a load out of the seed list)
    const uint64_t x = (key >> 1) & 0xffffffffull;
    const uint32_t is_rc = (uint32_t)(key & 1ull);
    uint32_t p = seeds[j];
    p = p < n ? p : n - 1;  // (a position by construction)
    const uint32_t L = len[p];
    uint32_t k;
    term_limit(tterms, p, k);  // the next terminator's index is the target
    k = k < tterms.count ? k : tterms.count - 1;
    const uint32_t q = p - (k ? tterms.pos[k - 1] + 1u : 0u);
    // the reverse strand: the hit kernel reported 2 B - a - L + 1 for the suffix a of the mirrored block; y = a
    uint64_t y = is_rc ? 2ull * B + 1ull - x - L : x;
    y = y < nx ? y : nx - 1;  // (a position of X by construction)
    const uint32_t record = vals[t];
    const uint32_t group = ((is_rc ? records : 0u) + record) & 0xffu;  // (below 2 m <= 250 by construction)
    out_keys[t] = ((uint64_t)(k & 0xffffffu) << 40) | ((uint64_t)group << 32) | y;
    out_vals[t] = t;
    slot_q[t] = q;
    slot_len[t] = L;
}

// One lane per sorted anchor: q and L gathered from their slots.  The slot is clamped to the T slots.  No loop.
__global__ __launch_bounds__(kThreads) void rlz_chain_gather_kernel(const uint32_t *__restrict__ vals, uint32_t T,
                                                                    const uint32_t *__restrict__ slot_q,
                                                                    const uint32_t *__restrict__ slot_len,
                                                                    uint32_t *__restrict__ aq, uint32_t *__restrict__ alen) {
    const uint64_t gid = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (gid >= T) return;
    uint32_t v = vals[gid];
    v = v < T ? v : T - 1;  // (a slot by construction)
    aq[gid] = slot_q[v];
    alen[gid] = slot_len[v];
}

// One lane per anchor: flag[i] = 1 at the first anchor of a (target, group).  Two coalesced loads.  No loop.
__global__ __launch_bounds__(kThreads) void rlz_chain_heads_kernel(const uint64_t *__restrict__ keys, uint32_t n,
                                                                   uint32_t *__restrict__ flag) {
    const uint64_t gid = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (gid >= n) return;
    const uint32_t i = (uint32_t)gid;
    flag[i] = (i == 0 || (keys[i] >> 32) != (keys[i - 1] >> 32)) ? 1u : 0u;
}

// One lane per anchor: a head goes to its slot of the group list, slot[i] = the heads in front of it; the last anchor
// closes the list with n.  gstart holds n + 1 entries and the slots are clamped to them.  No loop.
__global__ __launch_bounds__(kThreads) void rlz_chain_starts_kernel(const uint32_t *__restrict__ flag,
                                                                    const uint32_t *__restrict__ slot, uint32_t n,
                                                                    uint32_t *__restrict__ gstart) {
    const uint64_t gid = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (gid >= n) return;
    const uint32_t i = (uint32_t)gid;
    const uint32_t s = slot[i], fl = flag[i];
    if (fl) gstart[s < n ? s : n] = i;
    if (i == n - 1) {
        const uint32_t G = s + fl;
        gstart[G < n ? G : n] = n;
    }
}

__device__ __forceinline__ uint32_t lane_read(uint32_t v, uint32_t lane) {  // wave-uniform lane: a scalar read
    return (uint32_t)__builtin_amdgcn_readlane((int)v, __builtin_amdgcn_readfirstlane((int)lane));
}

__device__ __forceinline__ uint64_t wave_max_u64(uint64_t v) {  // every lane ends with the maximum; 6 steps
#pragma unroll
    for (int o = 32; o; o >>= 1) {
        const uint64_t w = (uint64_t)__shfl_xor((unsigned long long)v, o, 64);
        v = w > v ? w : v;
    }
    return v;
}

// One WAVEFRONT per group.  Lane l holds the latest anchor of the group whose index is l mod 64, with its f and its depth:
// when anchor i is scored the ring holds exactly i - 64 .. i - 1, the look-back.  Each block of 64 anchors is loaded one
// per lane, the next block before the current one is walked; anchor i is read from lane i mod 64, every lane scores its
// held anchor, and a 64-lane max over (score << 32 | index) gives f(i) and pred(i): of equal scores the largest index,
// the nearest, wins.  A candidate counts only if its score is above L(i), so a packed value is never 0 by accident and
// pred stays empty when L(i) is not beaten.  The end of the group -- the smallest index with maximal f -- and the depth of
// its chain are carried along.  Loops: the blocks of the group, 64 anchors each.
__global__ __launch_bounds__(kThreads) void rlz_chain_recurrence_kernel(const uint64_t *__restrict__ keys,
                                                                        const uint32_t *__restrict__ aq,
                                                                        const uint32_t *__restrict__ alen, uint32_t n,
                                                                        const uint32_t *__restrict__ gstart, uint32_t G,
                                                                        uint32_t max_gap, uint32_t bandwidth,
                                                                        uint64_t min_score, uint32_t *__restrict__ f,
                                                                        uint32_t *__restrict__ pred,
                                                                        uint32_t *__restrict__ gend,
                                                                        uint32_t *__restrict__ gscore,
                                                                        uint32_t *__restrict__ gdepth,
                                                                        uint32_t *__restrict__ kept,
                                                                        uint32_t *__restrict__ kept_depth) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t gw = (uint64_t)blockIdx.x * kWaves + (threadIdx.x >> 6);
    if (gw >= G) return;  // (the whole wavefront)
    const uint32_t g = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)gw);
    uint32_t start = gstart[g], end = gstart[g + 1];
    end = end < n ? end : n;  // (anchors by construction: no entry can lead a load out of the anchor arrays)
    start = start < end ? start : end;
    const uint32_t size = end - start;

    uint32_t hq = 0, hy = 0, hf = 0, hd = 0, hidx = kChainNoPred;  // the ring: this lane's held anchor
    uint32_t nq = 0, ny = 0, nl = 0;
    if (lane < size) {
        nq = aq[start + lane];
        ny = (uint32_t)keys[start + lane];
        nl = alen[start + lane];
    }
    uint32_t best_f = 0, best_i = 0, best_d = 0;
    for (uint32_t base = 0; base < size; base += 64u) {
        const uint32_t cq = nq, cy = ny, cl = nl;
        const uint32_t ahead = base + 64u + lane;
        if (ahead < size) {  // the next block, asked for before this one is walked
            nq = aq[start + ahead];
            ny = (uint32_t)keys[start + ahead];
            nl = alen[start + ahead];
        }
        const uint32_t cnt = size - base < 64u ? size - base : 64u;
        uint32_t out_f = 0, out_p = kChainNoPred;
        for (uint32_t t = 0; t < cnt; ++t) {
            const uint32_t i = base + t;
            const uint32_t qi = lane_read(cq, t), yi = lane_read(cy, t), li = lane_read(cl, t);
            uint64_t packed = 0;
            if (hidx != kChainNoPred) {  // (i - hidx is 1 .. 64 by the ring)
                const int64_t dq = (int64_t)qi - (int64_t)hq, dy = (int64_t)yi - (int64_t)hy;
                if (dq >= 1 && dy >= 1) {
                    const int64_t far = dq > dy ? dq : dy, diff = dq > dy ? dq - dy : dy - dq;
                    int64_t mn = dq < dy ? dq : dy;
                    mn = mn < (int64_t)li ? mn : (int64_t)li;
                    const int64_t cand = (int64_t)hf + mn - diff;
                    if (far <= (int64_t)max_gap && diff <= (int64_t)bandwidth && cand > (int64_t)li)
                        packed = ((uint64_t)cand << 32) | hidx;  // (cand < 2^32: the file comment)
                }
            }
            packed = wave_max_u64(packed);
            const uint32_t fi = packed ? (uint32_t)(packed >> 32) : li;
            const uint32_t pi = packed ? (uint32_t)packed : kChainNoPred;
            const uint32_t dp = lane_read(hd, pi & 63u);  // (lane pred mod 64 holds pred: it lies inside the ring)
            const uint32_t di = packed ? dp + 1u : 1u;
            if (lane == t) {  // anchor i replaces i - 64 in the ring
                hq = qi;
                hy = yi;
                hf = fi;
                hd = di;
                hidx = i;
                out_f = fi;
                out_p = pi;
            }
            if (fi > best_f) {  // strictly: the smallest index with maximal f
                best_f = fi;
                best_i = i;
                best_d = di;
            }
        }
        if (lane < cnt) {
            f[start + base + lane] = out_f;
            pred[start + base + lane] = out_p;
        }
    }
    if (lane == 0) {
        const uint32_t keep = (size && (uint64_t)best_f >= min_score) ? 1u : 0u;
        gend[g] = best_i;
        gscore[g] = best_f;
        gdepth[g] = best_d;
        kept[g] = keep;
        kept_depth[g] = keep ? best_d : 0u;
    }
}

// One lane per group: a kept group goes to its slot of the chain list.  The slot is clamped to the G entries.  No loop.
__global__ __launch_bounds__(kThreads) void rlz_chain_list_kernel(const uint32_t *__restrict__ kept,
                                                                  const uint32_t *__restrict__ cslot, uint32_t G,
                                                                  uint32_t *__restrict__ chain_group) {
    const uint64_t gid = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (gid >= G) return;
    if (!kept[gid]) return;
    const uint32_t c = cslot[gid];
    chain_group[c < G ? c : G - 1] = (uint32_t)gid;
}

// One lane per kept chain: walks pred from the end of its group and writes the anchors back to front into its CSR range,
// the extents in Rblk coordinates (min of x, max of x + L: y + L is not monotone along a chain) and the record.  Loop:
// the depth of the chain, at most the size of the group; pred must lie below the current index or the walk ends.
__global__ __launch_bounds__(kThreads) void rlz_chain_backtrack_kernel(const uint64_t *__restrict__ keys,
                                                                       const uint32_t *__restrict__ aq,
                                                                       const uint32_t *__restrict__ alen, uint32_t n,
                                                                       const uint32_t *__restrict__ gstart, uint32_t G,
                                                                       const uint32_t *__restrict__ chain_group,
                                                                       const uint32_t *__restrict__ gend,
                                                                       const uint32_t *__restrict__ gscore,
                                                                       const uint32_t *__restrict__ gdepth,
                                                                       const uint32_t *__restrict__ aoff,
                                                                       const uint32_t *__restrict__ pred, uint32_t C,
                                                                       uint32_t A, uint32_t records, uint32_t B,
                                                                       ChainRec *__restrict__ chains,
                                                                       uint64_t *__restrict__ offsets,
                                                                       ChainAnchorRec *__restrict__ anchors) {
    const uint64_t gid = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (gid >= C) return;
    const uint32_t c = (uint32_t)gid;
    uint32_t g = chain_group[c];
    g = g < G ? g : G - 1;  // (a group by construction)
    uint32_t start = gstart[g], end = gstart[g + 1];
    end = end < n ? end : n;  // (anchors by construction)
    end = end ? end : 1u;     // (n >= 1)
    start = start < end ? start : end - 1;
    const uint32_t size = end - start;
    uint32_t i = gend[g];
    i = i < size ? i : size - 1;  // (an anchor of the group by construction)
    uint32_t depth = gdepth[g];
    depth = depth < size ? depth : size;
    uint32_t ao = aoff[g];
    ao = ao < A ? ao : A - 1;  // (the chain's range lies inside the A anchors by construction)
    depth = depth <= A - ao ? depth : A - ao;
    const uint64_t head = keys[start];
    const uint32_t group = (uint32_t)(head >> 32) & 0xffu;
    const uint32_t is_rc = group >= records ? 1u : 0u;
    uint64_t t_start = 0, t_end = 0, r_start = ~0ull, r_end = 0;
    for (uint32_t step = 0; step < depth; ++step) {
        const uint32_t at = start + i;
        const uint64_t q = aq[at], L = alen[at], y = keys[at] & 0xffffffffull;
        const uint64_t x = is_rc ? 2ull * B + 1ull - y - L : y;
        ChainAnchorRec a;
        a.t_start = q;
        a.position = x;
        a.length = L;
        anchors[ao + (depth - 1u - step)] = a;
        if (step == 0) t_end = q + L;
        t_start = q;
        r_start = x < r_start ? x : r_start;
        r_end = x + L > r_end ? x + L : r_end;
        const uint32_t p = pred[at];
        if (p >= i) break;  // (no predecessor; a chain of `depth` anchors ends here by construction)
        i = p;
    }
    ChainRec r;
    r.target = head >> 40;
    r.t_start = t_start;
    r.t_end = t_end;
    r.r_start = r_start;
    r.r_end = r_end;
    r.score = gscore[g];
    r.record = group - (is_rc ? records : 0u);
    r.is_rc = is_rc;
    r.num_anchors = depth;
    r.primary = 0;
    chains[c] = r;
    offsets[c] = ao;
    if (c == C - 1) offsets[C] = (uint64_t)ao + depth;
}

// One lane per chain; the first chain of a target scans the chains of its target, which follow it in the list -- one per
// group, at most 256 -- and flags the one of largest score, the first of equals.  Loop: at most 255 steps.
__global__ __launch_bounds__(kThreads) void rlz_chain_primary_kernel(ChainRec *__restrict__ chains, uint32_t C) {
    const uint64_t gid = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (gid >= C) return;
    const uint32_t c = (uint32_t)gid;
    const uint64_t target = chains[c].target;
    if (c && chains[c - 1].target == target) return;
    uint32_t best = c;
    uint64_t best_score = chains[c].score;
    for (uint32_t d = c + 1; d < C && d - c < 256u; ++d) {
        if (chains[d].target != target) break;
        const uint64_t s = chains[d].score;
        if (s > best_score) {
            best_score = s;
            best = d;
        }
    }
    chains[best].primary = 1u;
}

int bits_of(uint64_t v) {  // the number of bits that hold v
    int b = 0;
    while (b < 64 && (v >> b)) ++b;
    return b;
}

}  // namespace

// The digits of key = (target << 40) | (group << 32) | y that can differ: y in bits [0, bits of y_end - 1), the group in
// bits [32, 40) and the target from bit 40 on, each as far up as a bit can be set.  The fields start on digit boundaries,
// so no digit mixes two of them.
int rlz_chain_sort_shifts(uint64_t y_end, uint64_t groups, uint64_t k, int *shifts) {
    const int low = y_end ? bits_of(y_end - 1) : 0;                           // (<= 32)
    const int mid = groups > 1 ? bits_of(groups - 1) : 0;                     // (<= 8)
    const int high = k > 1 ? bits_of(k - 1) : 0;                              // (<= 24)
    int npasses = 0;
    for (int b = 0; b < (low < 32 ? low : 32); b += kRadixBits) shifts[npasses++] = b;
    if (mid) shifts[npasses++] = 32;
    for (int b = 0; b < (high < 24 ? high : 24); b += kRadixBits) shifts[npasses++] = 40 + b;
    return npasses;
}

void rlz_index_rep_total(Context &ctx, const uint32_t *d_rep, uint32_t S, uint64_t *d_total) {
    ProfScope ps(ctx.profiler(), "rlz_chain_hit_total", ctx.stream, 4.0 * (double)S);
    ArenaRewind rewind(ctx.arena);  // (one stream: the partial sums have been read when the arena is used again)
    const unsigned parts = (unsigned)std::min<size_t>(div_up((size_t)S, kThreads), kTotalParts);
    uint64_t *d_parts = ctx.arena.alloc<uint64_t>(kTotalParts);
    rlz_chain_total_kernel<uint32_t><<<parts ? parts : 1u, kThreads, 0, ctx.stream>>>(d_rep, S, d_parts);
    KERNEL_CHECK();
    rlz_chain_total_kernel<uint64_t><<<1, kThreads, 0, ctx.stream>>>(d_parts, parts ? parts : 1u, d_total);
    KERNEL_CHECK();
}

ChainAnchors rlz_seed_chain_anchors(Context &ctx, const RlzIndexView &ix, uint32_t records, const PackedText &batch,
                                    const uint32_t *d_seeds, const uint32_t *d_len, uint32_t S, const LocateSorted &sorted,
                                    uint32_t T) {
    ChainAnchors out;
    if (T == 0 || S == 0) return out;
    hipStream_t s = ctx.stream;
    const unsigned blocks = (unsigned)div_up((size_t)T, kThreads);
    uint64_t *keys[2] = {ctx.arena.alloc<uint64_t>(T), ctx.arena.alloc<uint64_t>(T)};
    uint32_t *vals[2] = {ctx.arena.alloc<uint32_t>(T), ctx.arena.alloc<uint32_t>(T)};
    uint32_t *slot_q = ctx.arena.alloc<uint32_t>(T), *slot_len = ctx.arena.alloc<uint32_t>(T);
    uint32_t *aq = ctx.arena.alloc<uint32_t>(T), *alen = ctx.arena.alloc<uint32_t>(T);
    {
        ProfScope ps(ctx.profiler(), "rlz_chain_keys", s, 36.0 * (double)T);
        rlz_chain_keys_kernel<<<blocks, kThreads, 0, s>>>(batch.terms, batch.n, ix.text.n, ix.B, records, d_seeds, d_len, S,
                                                          sorted.keys, sorted.vals, T, keys[0], vals[0], slot_q, slot_len);
        KERNEL_CHECK();
    }
    int shifts[kLocateMaxPasses];
    const int npasses = rlz_chain_sort_shifts(ix.text.n, ix.with_rc ? 2ull * records : records, batch.terms.count, shifts);
    int at = 0;
    {
        // Stability is relied on: equal (target, group, y) keep the input order, which is that of the sorted hits -- by
        // seed, and the seeds ascend by (target, start) -- so the anchors of one y ascend by q.
        ProfScope ps(ctx.profiler(), "rlz_chain_sort", s, 24.0 * (double)T * npasses);
        at = radix_sort_pairs(keys, vals, T, shifts, npasses, ctx.arena, s, ctx.profiler());
    }
    {
        ProfScope ps(ctx.profiler(), "rlz_chain_gather", s, 20.0 * (double)T);
        rlz_chain_gather_kernel<<<blocks, kThreads, 0, s>>>(vals[at], T, slot_q, slot_len, aq, alen);
        KERNEL_CHECK();
    }
    out.keys = keys[at];
    out.q = aq;
    out.len = alen;
    out.n = T;
    return out;
}

ChainsOut rlz_seed_chain_run(Context &ctx, const ChainAnchors &a, const ChainRules &rules) {
    ChainsOut out;
    const uint32_t n = a.n;
    if (n == 0) return out;
    hipStream_t s = ctx.stream;
    const unsigned blocks = (unsigned)div_up((size_t)n, kThreads);
    uint32_t *flag = ctx.arena.alloc<uint32_t>(n), *slot = ctx.arena.alloc<uint32_t>(n);
    uint32_t *gstart = ctx.arena.alloc<uint32_t>((size_t)n + 1);
    uint32_t *d_totals = ctx.arena.alloc<uint32_t>(2);
    uint32_t *f = ctx.arena.alloc<uint32_t>(n), *pred = ctx.arena.alloc<uint32_t>(n);
    uint32_t G = 0;
    {
        ProfScope ps(ctx.profiler(), "rlz_chain_heads", s, 28.0 * (double)n);
        rlz_chain_heads_kernel<<<blocks, kThreads, 0, s>>>(a.keys, n, flag);
        KERNEL_CHECK();
        scan_exclusive_add_u32(flag, slot, n, d_totals, ctx.arena, s);
        rlz_chain_starts_kernel<<<blocks, kThreads, 0, s>>>(flag, slot, n, gstart);
        KERNEL_CHECK();
    }
    HIP_CHECK(hipMemcpyAsync(&G, d_totals, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));  // (G is a local)
    if (G == 0 || G > n) throw HipError("rlz seed chains: the anchors fall into no group, or into more groups than anchors");
    uint32_t *gend = ctx.arena.alloc<uint32_t>(G), *gscore = ctx.arena.alloc<uint32_t>(G), *gdepth = ctx.arena.alloc<uint32_t>(G);
    uint32_t *kept = ctx.arena.alloc<uint32_t>(G), *kept_depth = ctx.arena.alloc<uint32_t>(G);
    uint32_t *cslot = ctx.arena.alloc<uint32_t>(G), *aoff = ctx.arena.alloc<uint32_t>(G);
    uint32_t *chain_group = ctx.arena.alloc<uint32_t>(G);
    const unsigned gblocks = (unsigned)div_up((size_t)G, kThreads);
    {
        ProfScope ps(ctx.profiler(), "rlz_chain_recurrence", s, 24.0 * (double)n + 24.0 * (double)G);
        rlz_chain_recurrence_kernel<<<(unsigned)div_up((size_t)G, kWaves), kThreads, 0, s>>>(
            a.keys, a.q, a.len, n, gstart, G, rules.max_gap, rules.bandwidth, rules.min_score, f, pred, gend, gscore, gdepth,
            kept, kept_depth);
        KERNEL_CHECK();
    }
    uint32_t totals[2] = {0, 0};
    {
        ProfScope ps(ctx.profiler(), "rlz_chain_offsets", s, 28.0 * (double)G);
        scan_exclusive_add_u32(kept, cslot, G, d_totals, ctx.arena, s);
        scan_exclusive_add_u32(kept_depth, aoff, G, d_totals + 1, ctx.arena, s);
        rlz_chain_list_kernel<<<gblocks, kThreads, 0, s>>>(kept, cslot, G, chain_group);
        KERNEL_CHECK();
    }
    HIP_CHECK(hipMemcpyAsync(totals, d_totals, sizeof totals, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));  // (totals is a local)
    const uint32_t C = totals[0], A = totals[1];
    if (C > G || A > n || A < C) throw HipError("rlz seed chains: more chains than groups, or more chain anchors than anchors");
    out.f = f;
    out.pred = pred;
    if (C == 0) return out;
    ChainRec *chains = ctx.arena.alloc<ChainRec>(C);
    uint64_t *offsets = ctx.arena.alloc<uint64_t>((size_t)C + 1);
    ChainAnchorRec *anchors = ctx.arena.alloc<ChainAnchorRec>(A);
    const unsigned cblocks = (unsigned)div_up((size_t)C, kThreads);
    {
        ProfScope ps(ctx.profiler(), "rlz_chain_backtrack", s, 72.0 * (double)C + 40.0 * (double)A);
        rlz_chain_backtrack_kernel<<<cblocks, kThreads, 0, s>>>(a.keys, a.q, a.len, n, gstart, G, chain_group, gend, gscore,
                                                                gdepth, aoff, pred, C, A, rules.records, rules.B, chains,
                                                                offsets, anchors);
        KERNEL_CHECK();
    }
    {
        ProfScope ps(ctx.profiler(), "rlz_chain_primary", s, 32.0 * (double)C);
        rlz_chain_primary_kernel<<<cblocks, kThreads, 0, s>>>(chains, C);
        KERNEL_CHECK();
    }
    out.num_chains = C;
    out.num_anchors = A;
    out.chains = chains;
    out.offsets = offsets;
    out.anchors = anchors;
    return out;
}

}  // namespace nolzss
