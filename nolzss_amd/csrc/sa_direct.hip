// sa_direct.hip -- the direct rounds of the suffix-array construction: tied suffixes are ordered by comparing the packed
// text itself.  The first round (group_refine_kernel) takes every group of up to 64 suffixes right behind the key
// sort; the group-sort passes (group_sort.hpp) take what little it leaves -- the second direct round --, only the
// groups it did not touch -- the equalising round --, or every group of a collection of similar sequences against
// pivots -- the pivot passes.  Shared declarations: sa_internal.hpp.
#include "sa_internal.hpp"

#include "queues.hpp"
#include "scan.hpp"

#include <algorithm>

namespace nolzss {

namespace {

// First round after the key sort: members of a group are ordered by comparing their suffixes
// DIRECTLY in the packed text (they agree on the first h0 symbols; at most `cap` symbols are
// inspected).  For sequence data nearly every group is small and its members differ within a few
// hundred symbols, so this one round finishes them -- order, new group boundaries and the LCP to
// the predecessor -- where prefix doubling would need log2(LCP / h0) gather + sort + scatter
// rounds.  Members that still agree after `cap` symbols stay grouped (out_lo = number of strictly
// smaller members is equal for them) and go on to the doubling rounds; groups larger than
// kSmallGroup are flagged for the radix path (one ordinary doubling step).

// One workgroup refines all groups that START inside its kRefineTile list positions; every member
// is a thread, all state lives in LDS.
//   * Per round each still-tied member fetches the next kRefineWords * 64 bits (128 bases) of its suffix
//     (one random window per member per round -- never a pairwise re-read; an MI355X sustains
//     ~40 G such windows/s, tools/gatherbench.hip) and parks it in LDS.
//   * The comparisons are organised by PAIR, not by member: the unordered pairs of every group are
//     listed in LDS once, each wavefront owns a stretch of that list, compares the two windows of
//     64 pairs at a time and credits the loser (one more smaller member; the longest common prefix
//     with a smaller member) with LDS atomics.  A decided pair never comes back; tied pairs are
//     compacted to the front of the stretch for the next round.  Lanes therefore stay busy whatever
//     the group sizes are -- a member-per-lane loop runs every wavefront as long as its largest
//     group (group sizes on repeat-rich DNA: mean 3, size-weighted mean 6, tail to the cap), and
//     the kernel is bound by instruction issue, not by the fetches (rocprofv3 SQ_INSTS_*).
//   * cls = number of strictly smaller members; members still tied at the end keep list order.
// A group whose pairs do not fit the list any more is left as it is (out_lo = 0): the doubling
// rounds handle it like any other unfinished group.
// 192 list positions + the 64-member span = 256 threads: four wavefronts, one per SIMD, 8 workgroups per CU.
// (Round 1 ran 256 + 64 = 320 threads: five wavefronts load the SIMDs unevenly and every workgroup stayed for
// 6.25 comparison rounds on average -- as long as its slowest member; phase clocks, NOLZSS_REFINE_PHASES:
// set-up 6.7 k, fetch 12.4 k, compare 13.7 k cycles.  128 / 192 / 256 / 320 positions: 25.5 / 24.5 / 30.8 / 30.6 ms;
// 192 with the pair list cut to 20 KiB of LDS per workgroup (8 instead of 7 per CU): 22.1 ms.)
constexpr int kRefineWaves = kRefineThreads / 64;
constexpr int kPairCap = 1664;  // pairs per workgroup (192 members in groups of up to ~18 fit); 20 KiB of LDS: 8 workgroups = 32 waves per CU

template <int BITS, bool kTimed>
__global__ __launch_bounds__(kRefineThreads) __attribute__((amdgpu_waves_per_eu(kTimed ? 4 : 8, 8))) void group_refine_kernel(
    const uint32_t *__restrict__ act_slot, const uint32_t *__restrict__ act_grp, uint32_t *sa,
    const uint64_t *__restrict__ words, TermTable terms, uint32_t m, uint32_t h0, uint32_t cap,
    uint32_t *__restrict__ lcp, uint32_t *__restrict__ rank_by_slot, uint32_t *__restrict__ surv_slot,
    uint32_t *__restrict__ surv_head, uint32_t *__restrict__ surv_count, uint32_t *__restrict__ min_depth,
    unsigned long long *__restrict__ phases, bool no_stragglers) {
    const bool timed = kTimed && phases != nullptr && (blockIdx.x & 31) == 0 && threadIdx.x == 0;
    unsigned long long ck0 = 0, ck_fetch = 0, ck_cmp = 0, ck_rounds = 0, ck1 = 0, ck2 = 0;
    if (timed) ck0 = __builtin_readcyclecounter();
    constexpr int kW32 = 2 * kRefineWords;  // window in 32-bit words, text order
    constexpr int kChunks = kW32 / 4;
    constexpr uint32_t kPer32 = 32 / BITS;
    constexpr uint32_t kPerRound = kW32 * kPer32;
    __shared__ uint4 s_w[kChunks][kRefineThreads];  // chunk-major: a wave reads whole 16-byte rows
    __shared__ uint32_t s_pair[kPairCap];           // (higher member) | (lower member) << 16
    __shared__ uint32_t s_lim[kRefineThreads];      // symbols before the member's next terminator
    __shared__ uint32_t s_cls[kRefineThreads];      // strictly smaller members found so far
    __shared__ uint32_t s_best[kRefineThreads];     // longest common prefix with a smaller member
    __shared__ uint32_t s_goff[kRefineThreads];     // [first member of a group] first pair of the group
    __shared__ uint16_t s_term[kRefineThreads];     // index of the member's next terminator
    __shared__ uint8_t s_tied[2][kRefineThreads];   // member takes part in a tied pair (ping-pong)
    __shared__ uint32_t s_wtot[kRefineWaves];
    __shared__ uint32_t s_npairs;
    const size_t a0 = (size_t)blockIdx.x * kRefineTile;
    const size_t a1 = (a0 + kRefineTile < m) ? a0 + kRefineTile : m;
    const int t = threadIdx.x;
    const int lane = lane_id();
    const int w = t >> 6;
    const size_t a = a0 + t;

    // ---- who is here: members of groups that start in this tile -------------------------------
    // The size of a group is found in LDS: its last member (the next list element belongs to another
    // group) sits inside the span whenever the group has at most kSmallGroup members.
    uint32_t my_pos = 0, my_lim = 0, my_term = 0;
    int my_gl = 0, my_gs = 0, my_j = 0;  // first member (local), group size (0: not mine), my index
    bool starts_here = false;
    uint32_t j = 0, my_head = 0;  // my index in the group, slot of the group's first member
    bool last = false;
    bool stays = false;  // a member of a group this round leaves as it is, reported by this workgroup
    s_goff[t] = 0;  // doubles as the group size table until the pair offsets are written
    if (a < m) {
        const uint32_t g = act_grp[a];
        const uint32_t slot = act_slot[a];
        my_head = g;
        last = a + 1 == m || act_grp[a + 1] != g;
        my_pos = sa[slot];
        j = slot - g;  // my index inside the group
        const size_t g0 = a - j;
        starts_here = g0 >= a0 && g0 < a1;
        my_gl = starts_here ? (int)(g0 - a0) : 0;
    }
    __syncthreads();
    if (starts_here && last) s_goff[my_gl] = j + 1;
    __syncthreads();
    if (a < m) {
        const uint32_t sz = starts_here ? s_goff[my_gl] : 0u;  // 0: the group ends beyond the span
        const bool large = starts_here ? (sz == 0 || sz > kSmallGroup) : false;
        // too large for this round: stays one group, in place.  Its first kSmallGroup members are
        // written by the tile it starts in, the others by the tile that owns their list position.
        stays = (large && j < kSmallGroup) || (a < a1 && j >= kSmallGroup);  // (sa keeps its order)
        // the symbols every group that stays tied is known to agree on: h0 for the groups this round does
        // not touch, the depth reached for the others (the doubling rounds start from the minimum)
        if (large && j == 0) lower_min(min_depth + 1, h0);  // ([1]: groups this round does not touch)
        if (starts_here && !large) {
            my_gs = (int)sz;
            my_j = (int)j;
            // (one segment: no table look-up, and above all no load between my position and my first window)
            my_lim = term_limit(terms, my_pos, my_term);
        }
    }
    __syncthreads();  // everybody has read the sizes
    // member j of a group lists its pairs with members 0 .. j-1: the list position is an exclusive
    // scan of j over the tile
    uint32_t inc = wave_scan_inclusive_dpp((uint32_t)my_j, 0u, OpAdd<uint32_t>());
    if (lane == 63) s_wtot[w] = inc;
    if (t == 0) s_npairs = 0;
    s_lim[t] = my_lim;
    s_term[t] = (uint16_t)my_term;
    s_cls[t] = 0;
    s_best[t] = 0;
    __syncthreads();
    uint32_t my_off = inc - (uint32_t)my_j, all_pairs = 0;
#pragma unroll
    for (int k = 0; k < kRefineWaves; ++k) {
        if (k < w) my_off += s_wtot[k];
        all_pairs += s_wtot[k];
    }
    bool handled = my_gs != 0;
    uint32_t npairs = all_pairs;
    if (all_pairs > (uint32_t)kPairCap) {  // (rare, workgroup-uniform) not every group fits the list:
        // the handled groups are a prefix of the tile's groups
        if (my_gs && my_j == 0) s_goff[t] = my_off;
        __syncthreads();
        uint32_t gend = 0;
        if (my_gs) {
            gend = s_goff[my_gl] + (uint32_t)(my_gs * (my_gs - 1) / 2);
            handled = gend <= (uint32_t)kPairCap;
            if (handled && my_j == my_gs - 1) atomicMax(&s_npairs, gend);
            if (!handled) stays = true;  // no room for its pairs: the group stays as it is
            if (!handled && my_j == 0) lower_min(min_depth + 1, h0);
        }
        __syncthreads();
        npairs = s_npairs;
    }
    if (handled)
        for (int y = 0; y < my_j; ++y) s_pair[my_off + y] = (uint32_t)t | ((uint32_t)(my_gl + y) << 16);
    s_tied[0][t] = handled ? 1 : 0;
    __syncthreads();
    if (timed) ck1 = __builtin_readcyclecounter();
    // each wavefront owns a stretch of the pair list
    const uint32_t seg = ((npairs + kRefineWaves - 1) / kRefineWaves + 63u) & ~63u;
    const uint32_t seg0 = (uint32_t)w * seg;
    uint32_t cnt = seg0 < npairs ? (npairs - seg0 < seg ? npairs - seg0 : seg) : 0u;
    const uint64_t lt = lanemask_lt();

    int cur = 0;
    uint32_t depth = h0;
    constexpr int kStragglers = 64, kStragWindows = kRefineThreads / kStragglers;
    uint32_t strag_from = 0xffffffffu;
    if (npairs > 0) {
        for (uint32_t h = h0; h < cap; h += kPerRound) {
            if (s_tied[cur][t]) {  // the next kRefineWords words of my suffix, from symbol h
                const uint64_t bit = ((uint64_t)my_pos + h) * BITS;
                const uint64_t *src = words + (bit >> 6);
                uint32_t r[kW32 + 2];  // text order: high half of each 64-bit word first
#pragma unroll
                for (int k = 0; k <= kRefineWords; ++k) {
                    const uint64_t v = src[k];
                    r[2 * k] = (uint32_t)(v >> 32);
                    r[2 * k + 1] = (uint32_t)v;
                }
                // bit-select instead of ?: -- the compiler turns the conditional form into a
                // scratch array with a dynamic offset
                const uint32_t skip = (bit & 32) ? 0xffffffffu : 0u;
                const uint32_t o = (uint32_t)bit & 31;
                uint32_t q[kW32 + 1], win[kW32];
#pragma unroll
                for (int k = 0; k <= kW32; ++k) q[k] = (r[k + 1] & skip) | (r[k] & ~skip);
#pragma unroll
                for (int k = 0; k < kW32; ++k) win[k] = o ? __builtin_amdgcn_alignbit(q[k], q[k + 1], 32 - o) : q[k];
#pragma unroll
                for (int c = 0; c < kChunks; ++c)
                    s_w[c][t] = make_uint4(win[4 * c], win[4 * c + 1], win[4 * c + 2], win[4 * c + 3]);
            }
            s_tied[cur ^ 1][t] = 0;
            unsigned long long ca = timed ? __builtin_readcyclecounter() : 0;
            __syncthreads();
            unsigned long long cb = timed ? __builtin_readcyclecounter() : 0;

            uint32_t kept = 0;
            bool any_tie = false;
            for (uint32_t c0 = 0; c0 < cnt; c0 += 64) {
                const bool have = c0 + lane < cnt;
                const uint32_t item = have ? s_pair[seg0 + c0 + lane] : 0u;
                const int x = (int)(item & 0xffffu), u = (int)(item >> 16);  // x > u in list order
                bool tie = false;
                if (have) {
                    const uint32_t rem_x = s_lim[x] - h, rem_u = s_lim[u] - h;  // symbols before the terminators
                    uint32_t valid = rem_x < rem_u ? rem_x : rem_u;
                    valid = valid < kPerRound ? valid : kPerRound;
                    // both windows in one go: the compare is bound by LDS round trips, not LDS bytes
                    uint4 p[kChunks], y[kChunks];
#pragma unroll
                    for (int c = 0; c < kChunks; ++c) {
                        p[c] = s_w[c][x];
                        y[c] = s_w[c][u];
                    }
                    uint32_t xd = 0, yd = 0, wi = (uint32_t)kW32;  // the first differing word and its index
#pragma unroll
                    for (int c = kChunks - 1; c >= 0; --c) {
                        const uint32_t px[4] = {p[c].x, p[c].y, p[c].z, p[c].w};
                        const uint32_t yx[4] = {y[c].x, y[c].y, y[c].z, y[c].w};
#pragma unroll
                        for (int i = 3; i >= 0; --i) {
                            const bool diff = px[i] != yx[i];
                            xd = diff ? px[i] : xd;
                            yd = diff ? yx[i] : yd;
                            wi = diff ? (uint32_t)(4 * c + i) : wi;
                        }
                    }
                    uint32_t d = wi == (uint32_t)kW32 ? kPerRound : wi * kPer32 + (uint32_t)__clz((int)(xd ^ yd)) / BITS;
                    bool u_smaller = yd < xd;
                    if (d >= valid) {
                        if (valid == kPerRound) {  // equal windows, both suffixes go on
                            tie = true;
                        } else {  // a terminator is reached: nearer one first, then lower index
                            d = valid;
                            u_smaller = rem_u != rem_x ? rem_u < rem_x : s_term[u] < s_term[x];
                        }
                    }
                    if (!tie) {
                        const int loser = u_smaller ? x : u;  // the greater suffix
                        atomicAdd(&s_cls[loser], 1u);
                        atomicMax(&s_best[loser], h + d);  // deeper rounds only find longer prefixes
                    } else {
                        s_tied[cur ^ 1][x] = 1;
                        s_tied[cur ^ 1][u] = 1;
                    }
                }
                const uint64_t bal = __ballot(tie);  // tied pairs move to the front of the stretch
                if (tie) s_pair[seg0 + kept + (uint32_t)__popcll(bal & lt)] = item;
                kept += (uint32_t)__popcll(bal);
                any_tie |= tie;
            }
            cnt = kept;
            cur ^= 1;
            depth = h + kPerRound;  // pairs that are still tied agree on a whole window more
            // A workgroup that is still mostly tied after two windows sits on a long exact repeat:
            // comparing on to the cap would cost a window fetch per member per round for nothing.
            // Leave those ties to the doubling rounds, which need only log2(LCP) steps.
            const int busy = __syncthreads_count(any_tie);
            if (timed) { const unsigned long long cc = __builtin_readcyclecounter(); ck_fetch += cb - (ck2 ? ck2 : ck1); ck_cmp += cc - cb; ck2 = cc; ck_rounds += 1; (void)ca; }
            if (busy == 0 || (h >= h0 + kPerRound && busy > kRefineThreads / 4)) break;
            if (!no_stragglers && busy <= kStragglers / 2) {  // few tied pairs left: the rounds below
                strag_from = h + kPerRound;
                break;
            }
        }
    }


    // STRAGGLERS.  A workgroup stays as long as its deepest tie: after the first rounds a handful of members
    // is left, and every further round costs them a round trip to the text plus the barriers (phase clocks:
    // ~4 k cycles per round whatever the number of pairs; six rounds on average).  Once at most kStragglers
    // members are tied they are numbered, and the whole workgroup fetches for them: wavefront q takes window q
    // of every straggler, so ONE round trip brings kStragWindows windows each, compared in LDS one after the
    // other.  (s_tied[cur] holds the straggler's number + 1, s_goff its text position: no LDS is added.  The
    // loop is kept apart from the one above: woven into it, the common rounds ran 12-20 % slower.)
    static_assert(kStragWindows * kStragglers == kRefineThreads, "one fetching thread per straggler and window");
    if (strag_from < cap) {  // (workgroup-uniform)
        uint4 *s_flat = &s_w[0][0];
        for (uint32_t h = strag_from; h < cap;) {
            uint32_t nq = (cap - h + kPerRound - 1) / kPerRound;
            nq = nq < (uint32_t)kStragWindows ? nq : (uint32_t)kStragWindows;
            const bool tied = s_tied[cur][t] != 0;
            const uint64_t tb = __ballot(tied);
            if (lane == 0) s_wtot[w] = (uint32_t)__popcll(tb);
            __syncthreads();
            uint32_t sidx = (uint32_t)__popcll(tb & lt), ntied = 0;
#pragma unroll
            for (int k = 0; k < kRefineWaves; ++k) {
                if (k < w) sidx += s_wtot[k];
                ntied += s_wtot[k];
            }
            // (more members than fit -- a wavefront held several tied pairs per lane: their ties stay for the
            // doubling rounds, like ties at the cap)
            if (ntied > (uint32_t)kStragglers) break;
            if (tied) {
                s_tied[cur][t] = (uint8_t)(sidx + 1);
                s_goff[sidx] = my_pos;
            }
            __syncthreads();
            {
                const uint32_t q = (uint32_t)t / kStragglers, i = (uint32_t)t % kStragglers;
                // (a window behind the end of the text is never compared: its pair is decided where the
                // shorter suffix ends; the packed text is padded for windows that START inside it)
                if (i < ntied && q < nq && (uint64_t)s_goff[i] + h + (uint64_t)q * kPerRound <= (uint64_t)terms.end) {
                    const uint64_t bit = ((uint64_t)s_goff[i] + h + (uint64_t)q * kPerRound) * BITS;
                    const uint64_t *src = words + (bit >> 6);
                    uint32_t r[kW32 + 2];
#pragma unroll
                    for (int k = 0; k <= kRefineWords; ++k) {
                        const uint64_t v = src[k];
                        r[2 * k] = (uint32_t)(v >> 32);
                        r[2 * k + 1] = (uint32_t)v;
                    }
                    const uint32_t skip = (bit & 32) ? 0xffffffffu : 0u;
                    const uint32_t o = (uint32_t)bit & 31;
                    uint32_t qq[kW32 + 1], win[kW32];
#pragma unroll
                    for (int k = 0; k <= kW32; ++k) qq[k] = (r[k + 1] & skip) | (r[k] & ~skip);
#pragma unroll
                    for (int k = 0; k < kW32; ++k) win[k] = o ? __builtin_amdgcn_alignbit(qq[k], qq[k + 1], 32 - o) : qq[k];
#pragma unroll
                    for (int c = 0; c < kChunks; ++c)
                        s_flat[((size_t)q * kChunks + c) * kStragglers + i] = make_uint4(win[4 * c], win[4 * c + 1], win[4 * c + 2], win[4 * c + 3]);
                }
            }
            s_tied[cur ^ 1][t] = 0;
            __syncthreads();
            uint32_t kept = 0;
            bool any_tie = false;
            for (uint32_t c0 = 0; c0 < cnt; c0 += 64) {
                const bool have = c0 + lane < cnt;
                const uint32_t item = have ? s_pair[seg0 + c0 + lane] : 0u;
                const int x = (int)(item & 0xffffu), u = (int)(item >> 16);
                bool tie = have;
                if (have) {
                    const uint32_t sx = (uint32_t)s_tied[cur][x] - 1u, su = (uint32_t)s_tied[cur][u] - 1u;
                    uint32_t hq = h;
#pragma unroll 1
                    for (uint32_t q = 0; q < nq; ++q, hq += kPerRound) {
                        const uint32_t rem_x = s_lim[x] - hq, rem_u = s_lim[u] - hq;
                        uint32_t valid = rem_x < rem_u ? rem_x : rem_u;
                        valid = valid < kPerRound ? valid : kPerRound;
                        uint4 p[kChunks], y[kChunks];
#pragma unroll
                        for (int c = 0; c < kChunks; ++c) {
                            p[c] = s_flat[((size_t)q * kChunks + c) * kStragglers + sx];
                            y[c] = s_flat[((size_t)q * kChunks + c) * kStragglers + su];
                        }
                        uint32_t xd = 0, yd = 0, wi = (uint32_t)kW32;
#pragma unroll
                        for (int c = kChunks - 1; c >= 0; --c) {
                            const uint32_t px[4] = {p[c].x, p[c].y, p[c].z, p[c].w};
                            const uint32_t yx[4] = {y[c].x, y[c].y, y[c].z, y[c].w};
#pragma unroll
                            for (int i = 3; i >= 0; --i) {
                                const bool diff = px[i] != yx[i];
                                xd = diff ? px[i] : xd;
                                yd = diff ? yx[i] : yd;
                                wi = diff ? (uint32_t)(4 * c + i) : wi;
                            }
                        }
                        uint32_t d = wi == (uint32_t)kW32 ? kPerRound : wi * kPer32 + (uint32_t)__clz((int)(xd ^ yd)) / BITS;
                        bool u_smaller = yd < xd;
                        if (d >= valid) {
                            if (valid == kPerRound) continue;  // equal windows: on to the next one
                            d = valid;  // a terminator is reached: nearer one first, then lower index
                            u_smaller = rem_u != rem_x ? rem_u < rem_x : s_term[u] < s_term[x];
                        }
                        const int loser = u_smaller ? x : u;
                        atomicAdd(&s_cls[loser], 1u);
                        atomicMax(&s_best[loser], hq + d);
                        tie = false;
                        break;
                    }
                    if (tie) {
                        s_tied[cur ^ 1][x] = 1;
                        s_tied[cur ^ 1][u] = 1;
                    }
                }
                const uint64_t bal = __ballot(tie);
                if (tie) s_pair[seg0 + kept + (uint32_t)__popcll(bal & lt)] = item;
                kept += (uint32_t)__popcll(bal);
                any_tie |= tie;
            }
            cnt = kept;
            cur ^= 1;
            depth = h + nq * kPerRound;
            if (timed) ck_rounds += 1;
            if (__syncthreads_count(any_tie) == 0) break;
            h += nq * kPerRound;
        }
    }

    const unsigned long long ck3 = timed ? __builtin_readcyclecounter() : 0;
    if (cnt > 0 && lane == 0) lower_min(min_depth, depth);
    // ---- members still tied keep their list order: count the tied partners in front of me --------
    // (s_goff is free now; s_tied[0] marks the members of pairs that are still tied)
    s_goff[t] = 0;
    s_tied[0][t] = 0;
    __syncthreads();
    for (uint32_t c0 = 0; c0 < cnt; c0 += 64)
        if (c0 + lane < cnt) {
            const uint32_t item = s_pair[seg0 + c0 + lane];
            atomicAdd(&s_goff[item & 0xffffu], 1u);
            s_tied[0][item & 0xffffu] = 1;
            s_tied[0][item >> 16] = 1;
        }
    // What used to be a pass of its own over the whole list (regroup_kernel: 4.9 ms at 2^30 bases) happens here:
    // the LCP of every boundary that appeared goes straight to its slot, and the members that stay tied --
    // a percent of the list on sequence data -- are collected IN SLOT ORDER: parked at their new position inside
    // the workgroup's 256 list positions, compacted, and written to the workgroup's own region; a small kernel
    // concatenates the regions (compact_survivors_kernel).  (The window buffer is free: it holds the parking lot.)
    uint32_t *s_sv_slot = reinterpret_cast<uint32_t *>(&s_w[0][0]);
    uint32_t *s_sv_head = s_sv_slot + kRefineThreads;
    static_assert(sizeof(s_w) >= 2 * kRefineThreads * sizeof(uint32_t), "the parking lot fits the window buffer");
    s_sv_slot[t] = 0xffffffffu;
    __syncthreads();
    if (handled) {
        const uint32_t cls = s_cls[t], ties_before = s_goff[t];
        const uint32_t head = my_head + cls, slot = head + ties_before;
        // the new order goes straight into the suffix array: my group occupies the slots from my_head
        // on, in list order (only members of the group, all threads of this workgroup, ever read or
        // write those slots, and every read happened before the barriers above)
        sa[slot] = my_pos;
        // LCP to the predecessor in the new order: the closest smaller member shares the longest prefix
        // (the first member of the group keeps the entry it has; a tied predecessor: no boundary, stays pending)
        if (ties_before == 0 && cls > 0) lcp[slot] = s_best[t];
        // a boundary that stays undecided INSIDE a class this round compared: its own pending code, so that the
        // groups the round did not touch (code kLcpPending) can be told from it (the equalising round, below)
        if (ties_before > 0) lcp[slot] = kLcpPendingCompared;
        if (rank_by_slot) rank_by_slot[slot] = head + 1u;
        if (s_tied[0][t]) {
            const uint32_t nl = (uint32_t)my_gl + cls + ties_before;
            s_sv_slot[nl] = slot;
            s_sv_head[nl] = head;
        }
    } else if (stays) {
        const uint32_t slot = my_head + j;
        if (rank_by_slot) rank_by_slot[slot] = my_head + 1u;
        s_sv_slot[t] = slot;
        s_sv_head[t] = my_head;
    }
    __syncthreads();
    {
        const uint32_t sv = s_sv_slot[t], hd = s_sv_head[t];
        const bool keep = sv != 0xffffffffu;
        const uint64_t kb = __ballot(keep);
        if (lane == 0) s_wtot[w] = (uint32_t)__popcll(kb);
        __syncthreads();
        uint32_t at = (uint32_t)__popcll(kb & lt), total = 0;
#pragma unroll
        for (int k = 0; k < kRefineWaves; ++k) {
            if (k < w) at += s_wtot[k];
            total += s_wtot[k];
        }
        if (keep) {
            surv_slot[(size_t)blockIdx.x * kRefineThreads + at] = sv;
            surv_head[(size_t)blockIdx.x * kRefineThreads + at] = hd;
        }
        if (t == 0) surv_count[blockIdx.x] = total;
    }
    // how much of what stays tied was not compared at all: counted in every 64th workgroup (an estimate for the host's
    // choice of what runs next; one atomic per counting workgroup)
    if ((blockIdx.x & 63u) == 0) {
        const int untouched = __syncthreads_count(stays);
        if (t == 0 && untouched) atomicAdd(min_depth + 2, (uint32_t)untouched);
    }
    if (timed) {
        __builtin_amdgcn_s_waitcnt(0);
        const unsigned long long ck4 = __builtin_readcyclecounter();
        atomicAdd(phases + 0, ck1 - ck0);
        atomicAdd(phases + 1, ck_fetch);
        atomicAdd(phases + 2, ck_cmp);
        atomicAdd(phases + 3, ck4 - ck3);
        atomicAdd(phases + 4, ck_rounds);
        atomicAdd(phases + 5, 1ull);
        atomicAdd(phases + 6, ck4 - ck0);
    }
}

#include "group_sort.hpp"

}  // namespace

// ---- the launches of the first direct round (sa_internal.hpp): the only launch site of group_refine_kernel ----
void direct_round_launch(Context &ctx, const PackedText &text, const uint32_t *slot, const uint32_t *grp, uint32_t m, uint32_t *sa,
                         uint32_t *lcp, uint32_t *rank_by_slot, uint32_t h0, uint32_t cap, bool no_stragglers, bool timed,
                         uint32_t *new_slot, uint32_t *new_grp, uint32_t *d_new_m, uint32_t *d_min_depth) {
    hipStream_t s = ctx.stream;
    Arena &arena = ctx.arena;
    // the members that stay tied come back in one region per workgroup (group_refine_kernel's epilogue)
    const unsigned g = (unsigned)div_up(m, kRefineTile);
    uint32_t *surv_slot = arena.alloc<uint32_t>((size_t)g * kRefineThreads);
    uint32_t *surv_head = arena.alloc<uint32_t>((size_t)g * kRefineThreads);
    uint32_t *surv_count = arena.alloc<uint32_t>(g);
    uint32_t *surv_off = arena.alloc<uint32_t>(g);
    HIP_CHECK(hipMemsetAsync(d_min_depth, 0xff, 2 * sizeof(uint32_t), s));
    HIP_CHECK(hipMemsetAsync(d_min_depth + 2, 0, sizeof(uint32_t), s));
    {
        ProfScope ps(ctx.profiler(), "sa_direct_sort", s);
        unsigned long long *rphases = nullptr;
        if (timed) {
            rphases = arena.alloc<unsigned long long>(8);
            HIP_CHECK(hipMemsetAsync(rphases, 0, 64, s));
        }
        dispatch_bits(text.bits, [&](auto B) {
            constexpr int kBits = decltype(B)::value;
            auto launch = [&](auto T) {
                group_refine_kernel<kBits, decltype(T)::value><<<g, kRefineThreads, 0, s>>>(
                    slot, grp, sa, text.words, text.terms, m, h0, cap, lcp, rank_by_slot, surv_slot, surv_head, surv_count,
                    d_min_depth, rphases, no_stragglers);
            };
            if (rphases) launch(std::true_type{});
            else launch(std::false_type{});
        });
        KERNEL_CHECK();
        if (rphases) {
            unsigned long long hp[8];
            HIP_CHECK(hipMemcpyAsync(hp, rphases, 64, hipMemcpyDeviceToHost, s));
            HIP_CHECK(hipStreamSynchronize(s));
            const double wn = hp[5] ? (double)hp[5] : 1.0;
            fprintf(stderr, "[nolzss] group_refine phases (cycles per workgroup, %llu sampled): set-up %.0f  fetch+wait %.0f  compare %.0f  output %.0f  total %.0f  rounds %.2f\n",
                    hp[5], hp[0] / wn, hp[1] / wn, hp[2] / wn, hp[3] / wn, hp[6] / wn, hp[4] / wn);
        }
    }
    compact_survivors(ctx, surv_slot, surv_head, surv_count, surv_off, g, new_slot, new_grp, d_new_m);
}

// ---- direct round: small groups are finished by comparing packed suffixes ---------------
// (groups larger than kSmallGroup stay as they are; rank[] is not needed before the doubling
// rounds, so it is written once, after the direct rounds, instead of after each of them)
void direct_round(SaBuild &b, int k_syms) {
    const SaKnobs &knobs = sa_knobs();
    const PackedText &text = b.text;
    Arena &arena = b.arena();
    const size_t direct_mark = arena.mark();
    uint32_t *rbs = b.store_ranks ? b.rank_by_slot : nullptr;
    const uint32_t cap = (uint32_t)k_syms + knobs.refine_words * (64u / (uint32_t)text.bits);
    // [0] classes the round compared and left tied, [1] groups it did not touch, [2] members of such groups in every 64th workgroup
    uint32_t *d_min_depth = arena.alloc<uint32_t>(3);
    direct_round_launch(b.ctx, text, b.slot(), b.grp(), b.m, b.sa, b.lcp, rbs, (uint32_t)b.h, cap, knobs.no_stragglers,
                        knobs.refine_phases, b.next_slot(), b.next_grp(), b.d_total, d_min_depth);
    b.ctx.read_back(b.d_total, &b.m, 1);
    b.a_cur ^= 1;
    // every group that is still tied agrees on at least min_depth symbols (K if a group was too large
    // for the round, more if the round left all its ties at the cap or at a bail-out depth): the
    // doubling rounds start there instead of repeating the steps K, 2K, 4K, ...
    if (b.m > 0) {
        uint32_t depth2[3] = {0, 0, 0};
        b.ctx.read_back(d_min_depth, depth2, 3);
        b.depth_compared = depth2[0];
        b.depth_untouched = depth2[1];
        b.untouched_members = (uint64_t)depth2[2] * 64u;
        const uint32_t depth = depth2[0] < depth2[1] ? depth2[0] : depth2[1];
        if (depth != 0xffffffffu && depth > b.h) b.h = depth;
    }
    arena.rewind(direct_mark);
    if (knobs.trace) fprintf(stderr, "[nolzss]   direct round (cap %u symbols): %u still tied, on at least %llu symbols\n", cap, b.m, (unsigned long long)b.h);
}

// The rounds of one pass without the regroup behind them (sa_internal.hpp): the queues of the larger groups, group_dir_kernel
// and the four group_sort_kernel launches, all on the context's stream.  What it takes from the arena is the caller's to rewind.
void group_sort_rounds(Context &ctx, const PackedText &text, const uint32_t *slot, const uint32_t *grp, uint32_t m, uint32_t *sa,
                       uint32_t h0, bool pivot, uint32_t max_rounds, uint32_t depth_cap, const uint32_t *lcp_mark,
                       uint32_t *out_lo, uint32_t *lcp_list, uint32_t *d_min_depth) {
    hipStream_t s = ctx.stream;
    Arena &arena = ctx.arena;
    HIP_CHECK(hipMemsetAsync(d_min_depth, 0xff, sizeof(uint32_t), s));
    const unsigned dir_blocks = (unsigned)div_up(m, kThreads);
    ShardQueue q_mid0, q_mid, q_big;
    q_mid0.cap = q_mid.cap = q_big.cap = (uint32_t)shard_queue_cap(dir_blocks, kThreads);
    uint32_t *qcounts = arena.alloc<uint32_t>(3 * kQShards * kQPad);
    ShardQueue *queues[3] = {&q_mid0, &q_mid, &q_big};
    for (int k = 0; k < 3; ++k) {
        queues[k]->items = arena.alloc<uint32_t>((size_t)kQShards * q_big.cap);
        queues[k]->items2 = arena.alloc<uint32_t>((size_t)kQShards * q_big.cap);
        queues[k]->counts = qcounts + (size_t)k * kQShards * kQPad;
    }
    HIP_CHECK(hipMemsetAsync(qcounts, 0, 3 * kQShards * kQPad * sizeof(uint32_t), s));
    {
        ProfScope ps(ctx.profiler(), "sa_direct_sort2", s);
        group_dir_kernel<<<dir_blocks, kThreads, 0, s>>>(slot, grp, m, h0, out_lo, lcp_list, q_mid0, q_mid, q_big, d_min_depth, lcp_mark);
        KERNEL_CHECK();
        // small groups by tiles of the list; the larger ones from the queues (the consumers read the shard
        // counts on the device: no read-back in between)
        constexpr int kSmallN = 2 * (int)kGroupSortSmall, kMid0N = (int)kGroupSortMid0, kMidN = (int)kGroupSortMid,
                      kBigN = (int)kGroupSortMax;
        const unsigned tiles = (unsigned)div_up(m, kGroupSortSmall);
        const unsigned ym = (unsigned)std::min<size_t>(64, std::max<size_t>(1, div_up(m, (size_t)kQShards * 64)));
        const unsigned yb = (unsigned)std::min<size_t>(16, std::max<size_t>(1, div_up(m, (size_t)kQShards * 256)));
        const dim3 gm(kQShards, ym), gb(kQShards, yb);
        // (NOLZSS_GROUP_SORT_PHASES: the timed instantiations, one row of clocks per launch)
        unsigned long long *gphases = nullptr;
        if (sa_knobs().group_sort_phases) {
            gphases = arena.alloc<unsigned long long>(4 * kGroupSortPhaseWords);
            HIP_CHECK(hipMemsetAsync(gphases, 0, 4 * kGroupSortPhaseWords * sizeof(unsigned long long), s));
        }
        dispatch_bits(text.bits, [&](auto B) {
            constexpr int kBits = decltype(B)::value;
            auto launch = [&](auto P, auto T) {
                constexpr bool kP = decltype(P)::value, kT = decltype(T)::value;
                unsigned long long *ph = gphases;
                auto row = [&](int k) { return ph ? ph + k * kGroupSortPhaseWords : nullptr; };
                group_sort_kernel<kBits, kGroupSortTiledThreads, kSmallN, true, kP, kT><<<tiles, kGroupSortTiledThreads, 0, s>>>(
                    q_mid, slot, grp, m, sa, text.words, text.terms, h0, out_lo, lcp_list, d_min_depth, lcp_mark, max_rounds, depth_cap, row(0));
                constexpr int kT0 = kP ? 128 : kGroupSortMid0Threads, kT1 = kP ? 256 : kGroupSortMidThreads;
                group_sort_kernel<kBits, kT0, kMid0N, false, kP, kT><<<gm, kT0, 0, s>>>(
                    q_mid0, slot, grp, m, sa, text.words, text.terms, h0, out_lo, lcp_list, d_min_depth, lcp_mark, max_rounds, depth_cap, row(1));
                group_sort_kernel<kBits, kT1, kMidN, false, kP, kT><<<gm, kT1, 0, s>>>(
                    q_mid, slot, grp, m, sa, text.words, text.terms, h0, out_lo, lcp_list, d_min_depth, lcp_mark, max_rounds, depth_cap, row(2));
                group_sort_kernel<kBits, 256, kBigN, false, kP, kT><<<gb, 256, 0, s>>>(
                    q_big, slot, grp, m, sa, text.words, text.terms, h0, out_lo, lcp_list, d_min_depth, lcp_mark, max_rounds, depth_cap, row(3));
            };
            if (pivot) {
                if (gphases) launch(std::true_type{}, std::true_type{});
                else launch(std::true_type{}, std::false_type{});
            } else {
                if (gphases) launch(std::false_type{}, std::true_type{});
                else launch(std::false_type{}, std::false_type{});
            }
        });
        KERNEL_CHECK();
        if (gphases) {
            unsigned long long hp[4 * kGroupSortPhaseWords];
            HIP_CHECK(hipMemcpyAsync(hp, gphases, sizeof(hp), hipMemcpyDeviceToHost, s));
            HIP_CHECK(hipStreamSynchronize(s));
            static const char *const kForm[4] = {"tiles", "up to 128", "up to 256", "up to 1024"};
            for (int k = 0; k < 4; ++k) {
                const unsigned long long *r = hp + k * kGroupSortPhaseWords;
                if (!r[7]) continue;
                const double g = (double)r[7];
                fprintf(stderr, "[nolzss] group_sort %s phases %s (cycles per group, %llu sampled): set-up %.0f  scan %.0f  window %.0f  ranking %.0f  "
                                "boundaries+segments %.0f  output %.0f  rounds %.2f  scan words per scanning member %.2f (%llu scans)\n",
                        pivot ? "pivot" : "window", kForm[k], r[7], r[0] / g, r[1] / g, r[2] / g, r[3] / g, r[4] / g, r[5] / g, r[6] / g,
                        r[9] ? (double)r[8] / (double)r[9] : 0.0, r[9]);
            }
        }
    }
}

namespace {

enum class GroupSortMode { kDirect2, kEqualise, kPivot };

// One pass of the group-sort kernels over the active list, depth_cap symbols deep at the most (pivot passes), and the
// regroup behind it.
void group_sort_pass(SaBuild &b, GroupSortMode mode, uint32_t depth_cap) {
    const PackedText &text = b.text;
    Arena &arena = b.arena();
    const uint32_t m = b.m;
    const bool pivot = mode == GroupSortMode::kPivot, equalise = mode == GroupSortMode::kEqualise;
    const uint32_t max_rounds = equalise ? std::min<uint32_t>(kGroupSortRounds, (b.depth_compared - (uint32_t)b.h + 63u) / 64u) : kGroupSortRounds;
    const uint32_t *lcp_mark = equalise ? b.lcp : nullptr;
    const uint32_t *slot = b.slot(), *grp = b.grp();
    const size_t d2_mark = arena.mark();
    uint32_t *out_lo = arena.alloc<uint32_t>(m);
    uint32_t *lcp_list = arena.alloc<uint32_t>(m);
    uint32_t *d_min_depth = arena.alloc<uint32_t>(1);
    group_sort_rounds(b.ctx, text, slot, grp, m, b.sa, (uint32_t)b.h, pivot, max_rounds, depth_cap, lcp_mark, out_lo, lcp_list, d_min_depth);
    RegroupIn in;
    in.lo = out_lo;
    in.lcp_list = lcp_list;
    in.dbl_h = (uint32_t)b.h;
    in.sa_is_current = true;
    in.by_slot = true;
    regroup<false>(b, in);
    if (b.m > 0) {
        uint32_t depth = 0;
        b.ctx.read_back(d_min_depth, &depth, 1);
        // (equalising: the classes the first round compared were not looked at; they keep their depth)
        if (equalise && b.depth_compared < depth) depth = b.depth_compared;
        if (depth != 0xffffffffu && depth > b.h) b.h = depth;
    }
    arena.rewind(d2_mark);
    if (sa_knobs().trace) fprintf(stderr, "[nolzss]   %s: %u of %u finished, %u still tied, on at least %llu symbols\n",
                                  pivot ? "pivot rounds" : equalise ? "equalising round (untouched groups only)" : "second direct round", m - b.m, m, b.m, (unsigned long long)b.h);
}

}  // namespace

// ---- the passes over group_sort.hpp: what is left is sorted group by group, by the text ----
void group_sort_passes(SaBuild &b) {
    const SaKnobs &knobs = sa_knobs();
    const PackedText &text = b.text;
    const uint32_t n = b.n, m = b.m;
    const uint64_t h = b.h;
    // SECOND DIRECT round: where little is tied (at most 1 / NOLZSS_DIRECT2_MAX of the text), everything that is.
    // The EQUALISING round (collections of similar genomes): where much is tied and the first direct round left groups
    // untouched -- more than 64 members, or pairs that did not fit its list -- the doubling rounds would start at the
    // key depth for everything, four rounds over the whole list below the depth the compared classes already have.
    // The same kernels take only the untouched groups (told by their pending code) for as many rounds as reach that
    // depth: every round adds a window of 64 symbols to what a tied segment is known to agree on.  Only where the
    // untouched groups hold a minor part of what is tied (estimated by the first round): a wavefront per group of 65 and
    // more members that ALL stay tied takes 170 us per group and round -- 96 genomes of 2^28 bases in all, every suffix
    // in such a group, spent 480 ms here -- and the tiles of small groups 85 ms on 48 genomes, what four doubling rounds cost.
    const bool force_pivot = knobs.pivot_min >= 0 && (long long)m >= knobs.pivot_min;
    const bool full_direct2 = !force_pivot && !knobs.no_direct2 && m > 0 && h < n && !b.independent && knobs.direct2_div > 0 &&
                              m <= n / knobs.direct2_div + 1024u;
    const bool equalise = !full_direct2 && !knobs.no_direct2 && !knobs.no_equalise && m > 0 && h < n && !b.independent && text.bits == 2 &&
                          b.depth_untouched != 0xffffffffu && b.depth_untouched == h &&
                          b.depth_compared != 0xffffffffu && b.depth_compared >= 2 * h && b.untouched_members <= m / 3;
    if (knobs.trace && m > 0 && b.depth_untouched != 0xffffffffu)
        fprintf(stderr, "[nolzss]   about %llu of the tied suffixes sit in groups the direct round did not compare (depth %u; compared classes: %u)\n",
                (unsigned long long)b.untouched_members, b.depth_untouched, b.depth_compared);
    // PIVOT rounds (group_sort.hpp, kPivot): a repetitive text whose tied suffixes sit in groups of more than two or three
    // -- a collection of similar sequences -- has every tied group of up to kGroupSortMax members sorted against pivots,
    // kPivotDepth symbols deep: what stays tied agrees that far, and the doubling rounds start there instead of at the
    // key depth.  Texts whose ties are pairs (two copies: the pair-run pass) or runs of a short period (groups as large as
    // the runs: the periodic pass) are told by a count over the list and skip it.
    bool pivot = false;
    if (!knobs.no_pivot && !full_direct2 && m > 0 && h < n && !b.independent) {
        uint32_t c4[4] = {0, 0, 0, 0};
        count_large_groups(b, kGroupSortMax, b.arena().alloc<uint32_t>(4), c4);
        const uint64_t huge = (uint64_t)c4[0] + (uint64_t)kGroupSortMax * c4[1];  // members of groups beyond the kernels' reach
        pivot = force_pivot || ((uint64_t)m * 4 > (uint64_t)c4[2] * 10 && huge <= m / 2 && c4[3] <= m / 2);
        if (knobs.trace) fprintf(stderr, "[nolzss]   %u tied suffixes in %u groups, %llu in groups of more than %u, %u next to a member at most %u symbols away: %s\n",
                                 m, c4[2], (unsigned long long)huge, kGroupSortMax, c4[3], kPerVerifyMax, pivot ? "pivot rounds" : "no pivot rounds");
    }
    if (!full_direct2 && !equalise && !pivot) return;
    // (group_sort.hpp carries the terminator index of a suffix that ends inside a comparison in 16 bits)
    if (text.terms.count > 0x10000u) throw HipError("suffix array: the group-sort rounds take texts of at most 65536 segments");
    // (pivot rounds come in PASSES: what a pass leaves tied agrees on its cap, and while a pass finishes at least half of what
    // it was given the next one goes four times as deep over what is left -- 96 genomes 0.1 % apart: 2.65e8 -> 5.9e7 -> 1e6
    // tied suffixes after caps of 2048 and 8192 symbols, where the doubling rounds would take four rounds and the rank scatter
    // in front of them.  A pass that finishes less than half -- exact copies -- hands over to the doubling rounds.)
    // (the depth is given in symbols of 2-bit DNA; wider symbols get proportionally fewer, so that a member reads the same
    // number of text words whatever the alphabet: 2048 bases = 512 bytes)
    uint32_t pass_depth = std::max<uint32_t>(64u, knobs.pivot_depth * 2u / (uint32_t)text.bits);
    const GroupSortMode mode = pivot ? GroupSortMode::kPivot : equalise ? GroupSortMode::kEqualise : GroupSortMode::kDirect2;
    for (int pass = 0;; ++pass) {
        const uint32_t before = b.m;
        group_sort_pass(b, mode, (uint32_t)std::min<uint64_t>(b.h + pass_depth, 0xfffffff0u));
        // another pass?  only pivot passes repeat: while they make progress, something is left, and the depth has room
        if (!pivot || b.m == 0 || b.h >= n || pass + 1 >= knobs.pivot_passes || (uint64_t)(before - b.m) * 2 < before) break;
        pass_depth = pass_depth < (1u << 28) ? pass_depth * 4 : pass_depth;
    }
}

}  // namespace nolzss
