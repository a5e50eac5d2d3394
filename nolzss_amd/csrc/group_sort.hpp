// group_sort.hpp -- the SECOND direct round of the suffix-array construction (included by sa_direct.hip
// inside its anonymous namespace, behind the first direct round's kernel).
//
// The first direct round (group_refine_kernel) finishes groups of up to 64 suffixes by comparing pairs,
// 1024 bases deep.  What it leaves on ordinary sequence data is little -- 0.6 % of the suffixes of the 2^30-base
// benchmark text -- but it used to cost the whole machinery behind it: rank[] written for every suffix (a full
// random permutation, 13 ms) so that six prefix-doubling rounds could look up rank[i + h] for that 0.6 %.
// What is left are (a) groups of more than 64 members -- regions with dozens to hundreds of copies, which
// diverge after a few dozen bases --, (b) groups whose pairs did not fit the first round's pair list, and (c) the
// few ties deeper than its cap.  None of them needs ranks: here ONE workgroup takes ONE group, whatever its size
// up to kGroupSortMax, and sorts it by the text itself, round by round:
//   * the members of a still-tied segment measure how far they agree with the segment's first member (a scan of
//     at most kScanWords words): the segment's depth jumps to the first symbol at which somebody differs -- a
//     deep tie costs a few rounds, not one round per window;
//   * every tied member fetches the 128 text bits at that depth (masked at its terminator; the distance to the
//     terminator and the terminator's index break ties the way text.hpp defines) and finds its place inside its
//     segment by counting the members with a smaller (window, terminator);
//   * neighbours that differ become segment boundaries, with LCP = depth + common prefix of the two windows.
// Output is what the first round hands to the regroup kernel: the new order in sa, per list position the number
// of strictly smaller members of its group (out_lo) and the LCP of every boundary that appeared (lcp_list).
// A group that runs out of its budget keeps what it has separated; the rest stays tied for the doubling rounds,
// which then pay for rank[] as before.
// How a round is issued (profiles/group_sort_trips_ab.txt): one trip to the text -- a member that scans asks for the words
// of its scan, of its segment's first member and of the window behind them at once, and cuts the window out of its
// registers when the segment's depth is known --, one thread per position in the queue kernels, a ranking walk whose
// end is known in advance, and queue items taken from a counter of the shard.
#pragma once

constexpr uint32_t kGroupSortSmall = 64;   // groups up to here: by tiles of the list, one wavefront per tile
constexpr uint32_t kGroupSortMid = 256;    // up to here: one workgroup per group, a thread per member (two queues: up to 128,
                                           // up to 256 -- the LDS and the wavefronts of a workgroup, i.e. how many groups a CU
                                           // works on at a time)
constexpr uint32_t kGroupSortMid0 = 128;
constexpr uint32_t kGroupSortMax = 1024;   // up to here: 256 threads per group; beyond: left to the doubling rounds
constexpr uint32_t kScanWords = 8;         // 64-bit words a member scans per round to find where its segment splits
// (kGroupSortRounds, the rounds before a group gives up: sa_internal.hpp, the test hook checks its argument against it)

// PIVOT rounds (round 4; kPivot): collections of similar sequences -- dozens to hundreds of copies of a genome, a
// fraction of a percent apart -- tie in groups as large as the collection, and somebody in such a group differs
// every few symbols: the window rounds above advance to the NEXT difference of ANY member, a hundred rounds for a
// thousand symbols.  A pivot round compares every member of a segment with the segment's FIRST member R only, as
// far as they agree (up to kPivotWords words per round, kPivotBatch words per trip to the text, all loads of a
// batch in flight): member x learns l = lcp(x, R), which of the two is smaller, and its own symbol at l.  That
// orders the whole segment at once -- the members below R by ascending l (x differs from R where y still agrees:
// x < y), then R and what equals it as far as was compared, then the members above R by descending l; equal l:
// by the symbol at l (the end of a suffix in front of every symbol, ends by terminator index, text.hpp) -- and
// neighbours of different classes have LCP = the smaller l.  Members with the same (side, l, symbol) agree on l + 1
// symbols and go on as a smaller segment with a pivot of their own.  With k copies that mutate independently a
// round finishes every member that differs from the consensus before the pivot does -- half of the segment --
// so a group is done in about log2(k) rounds, and every member reads the text about as far as its own LCP.
// Segments that agree up to depth_cap are left tied for the doubling rounds, which start there.
constexpr uint32_t kPivotWords = 32;  // words a member compares with its pivot per round (1024 bases of DNA)
constexpr uint32_t kPivotBatch = 8;   // ... of which this many per dependent trip to the text
// threads of the window-round kernels (the pivot kernels: 64, 128, 256, 256).  The two queue kernels: one position per
// thread, so that a member keeps the words of its scan in registers and walks its segment once.  The tiles of small
// groups stay at two positions per thread: a second wavefront per tile halves the tiles a CU works on (128 threads:
// 0.70 against 0.49 ms on the benchmark text, profiles/group_sort_trips_ab.txt).
constexpr int kGroupSortTiledThreads = 64, kGroupSortMid0Threads = 128, kGroupSortMidThreads = 256;
// words a scanning member asks for in ONE trip: the kScanWords of the scan and what a window that starts at the scan's
// stop still needs (2 words and the one that the shift takes from).  A member only asks where a symbol of its own is
// left, so the first of them lies inside the text and the last inside the zero words behind it (text.hpp, PackedText)
constexpr uint32_t kScanFetch = kScanWords + 2;
static_assert(kScanFetch + 1 <= 12, "a fetch that starts inside the text ends inside the pad words of the packed text");

// one queue entry per LARGE group of the leftover list (items = first list position, items2 = members); groups
// of up to kGroupSortSmall members are found by the tile kernel itself
__global__ __launch_bounds__(kThreads) void group_dir_kernel(const uint32_t *__restrict__ act_slot,
                                                             const uint32_t *__restrict__ act_grp, uint32_t m,
                                                             uint32_t h0, uint32_t *__restrict__ out_lo,
                                                             uint32_t *__restrict__ lcp_list, ShardQueue q_mid0,
                                                             ShardQueue q_mid, ShardQueue q_big,
                                                             uint32_t *__restrict__ min_depth,
                                                             const uint32_t *__restrict__ lcp_mark) {
    const uint32_t shard = blockIdx.x % kQShards;
    const size_t a = (size_t)blockIdx.x * blockDim.x + threadIdx.x;  // (the grid covers the list once: every lane
    bool mid0 = false, mid = false, big = false;                     //  stays for the ballots of shard_slot)
    uint32_t first = 0, sz = 0;
    if (a < m) {
        out_lo[a] = 0;  // (a group nobody takes stays one group, in place)
        lcp_list[a] = kLcpPending;
        const uint32_t g = act_grp[a], j = act_slot[a] - g;
        // (lcp_mark, the equalising round: only the groups the first direct round did not touch -- the boundary behind
        // the group's first member still holds the plain pending code)
        if ((a + 1 == m || act_grp[a + 1] != g) && (lcp_mark == nullptr || lcp_mark[g + 1] == kLcpPending)) {  // the last member knows the size
            sz = j + 1;
            first = (uint32_t)a - j;
            mid0 = sz > kGroupSortSmall && sz <= kGroupSortMid0;
            mid = sz > kGroupSortMid0 && sz <= kGroupSortMid;
            big = sz > kGroupSortMid && sz <= kGroupSortMax;
            if (sz > kGroupSortMax) lower_min(min_depth, h0);

        }
    }
    const uint32_t s0 = shard_slot(q_mid0, shard, mid0);
    if (mid0) {
        q_mid0.items[s0] = first;
        q_mid0.items2[s0] = sz;
    }
    const uint32_t s1 = shard_slot(q_mid, shard, mid);
    const uint32_t s2 = shard_slot(q_big, shard, big);
    if (mid) {
        q_mid.items[s1] = first;
        q_mid.items2[s1] = sz;
    }
    if (big) {
        q_big.items[s2] = first;
        q_big.items2[s2] = sz;
    }
}

// 128 text bits of suffix p at depth h (two words), zero behind the member's terminator; tt = symbols before the
// terminator (capped at the window) << 16 | index of the terminator for a suffix that ends inside the window.
// Two suffixes that agree on everything in front of the window order by (k0, k1, tt): text.hpp, "nearer
// terminator first, then the lower index" -- a masked window equals a longer one only where that one continues
// with zero symbols, and then the shorter suffix (smaller tt) is the smaller one.
template <int BITS>
__device__ __forceinline__ void group_window(const uint64_t *__restrict__ words, uint32_t p, uint32_t h, uint32_t lim,
                                             uint32_t term, uint64_t &k0, uint64_t &k1, uint32_t &tt) {
    constexpr uint32_t kPer = 64 / BITS;
    const uint32_t rem = lim > h ? lim - h : 0u;
    const uint32_t tag = rem < 2 * kPer ? rem : 2 * kPer;
    uint64_t w0 = 0, w1 = 0;
    if (tag) {
        // three consecutive words cover both windows
        const uint64_t bit = ((uint64_t)p + h) * BITS;
        const uint64_t *src = words + (bit >> 6);
        const int o = (int)(bit & 63);
        const uint64_t a = src[0], b = src[1], c = src[2];
        w0 = o ? ((a << o) | (b >> (64 - o))) : a;
        w1 = o ? ((b << o) | (c >> (64 - o))) : b;
        if (tag < kPer) {
            w0 &= ~((~0ull) >> (tag * BITS));
            w1 = 0;
        } else if (tag == kPer) {
            w1 = 0;
        } else if (tag < 2 * kPer) {
            w1 &= ~((~0ull) >> ((tag - kPer) * BITS));
        }
    }
    k0 = w0;
    k1 = w1;
    tt = (tag << 16) | (tag < 2 * kPer ? (term & 0xffffu) : 0u);
}

// pivot rounds: the sort key of a member relative to its pivot, one 64-bit word (one LDS read and one comparison per
// step of the ranking): [side : 2 | l - D, descending above the pivot : 11 | symbol : 9] in the high half, the
// terminator index + 1 of a suffix that ends at l in the low half (D = depth of the segment, l - D <= kPivotWords
// words of symbols; symbol 0 = the suffix ends, else 1 + the member's symbol at l)
static_assert(kPivotWords * 32 <= 1024, "l - D fits 11 bits");
__device__ __forceinline__ uint64_t pivot_key(uint32_t side, uint32_t lrel, uint32_t sym, uint32_t tword) {
    const uint32_t k = (side << 30) | ((side == 2 ? 2047u - lrel : (side == 0 ? lrel : 0u)) << 9) | sym;
    return ((uint64_t)k << 32) | tword;
}
// l - D of a key (0xffffffff for the pivot's own class: every other class decides an LCP with it)
__device__ __forceinline__ uint32_t pivot_lrel_of(uint64_t key) {
    const uint32_t k = (uint32_t)(key >> 32), side = k >> 30, v = (k >> 9) & 2047u;
    return side == 1 ? 0xffffffffu : (side == 2 ? 2047u - v : v);
}
// kPivotBatch words of suffix p from symbol h on, as 2 * kPivotBatch 32-bit words in text order (the high half of
// a 64-bit word first): kPivotBatch + 1 loads, one funnel shift per 32 bits
template <int BITS, uint32_t W = kPivotBatch>
__device__ __forceinline__ void pivot_fetch(const uint64_t *__restrict__ words, uint64_t p, uint32_t h, uint32_t (&win)[2 * W]) {
    const uint64_t bit = (p + h) * BITS;
    const uint64_t *src = words + (bit >> 6);
    uint32_t r[2 * W + 2];
#pragma unroll
    for (uint32_t k = 0; k <= W; ++k) {
        const uint64_t v = src[k];
        r[2 * k] = (uint32_t)(v >> 32);
        r[2 * k + 1] = (uint32_t)v;
    }
    const uint32_t skip = (bit & 32) ? 0xffffffffu : 0u;
    const uint32_t o = (uint32_t)bit & 31;
    uint32_t q[2 * W + 1];
#pragma unroll
    for (uint32_t k = 0; k <= 2 * W; ++k) q[k] = (r[k + 1] & skip) | (r[k] & ~skip);
#pragma unroll
    for (uint32_t k = 0; k < 2 * W; ++k) win[k] = o ? __builtin_amdgcn_alignbit(q[k], q[k + 1], 32 - o) : q[k];
}

// first symbol at which the scans x and y of two members differ, counted from the scan's start (kScanWords words: the
// scan's reach if they agree)
template <int BITS, uint32_t WX, uint32_t WY>
__device__ __forceinline__ uint32_t scan_first_diff(const uint32_t (&x)[WX], const uint32_t (&y)[WY]) {
    uint32_t fb = 2 * kScanWords, xw = 0, yw = 0;
#pragma unroll
    for (int b = 2 * (int)kScanWords - 1; b >= 0; --b) {
        const bool diff = x[b] != y[b];
        fb = diff ? (uint32_t)b : fb;
        xw = diff ? x[b] : xw;
        yw = diff ? y[b] : yw;
    }
    return fb < 2 * kScanWords ? fb * (32 / BITS) + (uint32_t)__clz((int)(xw ^ yw)) / BITS : kScanWords * (64 / BITS);
}

// group_window of a member whose text from depth d0 on stands in x (kScanFetch words): the window at depth D, d0 <= D <= d0 +
// kScanWords words, cut from the registers
template <int BITS>
__device__ __forceinline__ void group_window_cut(const uint32_t (&x)[2 * kScanFetch], uint32_t d0, uint32_t D, uint32_t lim,
                                                 uint32_t term, uint64_t &k0, uint64_t &k1, uint32_t &tt) {
    constexpr uint32_t kPer = 64 / BITS, kPer32 = 32 / BITS;
    const uint32_t rem = lim > D ? lim - D : 0u;
    const uint32_t tag = rem < 2 * kPer ? rem : 2 * kPer;
    uint64_t w0 = 0, w1 = 0;
    if (tag) {
        const uint32_t i = (D - d0) / kPer32, o = ((D - d0) % kPer32) * BITS;
        uint32_t a[5] = {0, 0, 0, 0, 0};
#pragma unroll
        for (uint32_t j = 0; j <= 2 * kScanWords; ++j) {
#pragma unroll
            for (uint32_t c = 0; c < 5; ++c) a[c] = (i == j && j + c < 2 * kScanFetch) ? x[j + c < 2 * kScanFetch ? j + c : 0] : a[c];
        }
        uint32_t v[4];
#pragma unroll
        for (uint32_t c = 0; c < 4; ++c) v[c] = o ? __builtin_amdgcn_alignbit(a[c], a[c + 1], 32 - o) : a[c];
        w0 = ((uint64_t)v[0] << 32) | v[1];
        w1 = ((uint64_t)v[2] << 32) | v[3];
        if (tag < kPer) {
            w0 &= ~((~0ull) >> (tag * BITS));
            w1 = 0;
        } else if (tag == kPer) {
            w1 = 0;
        } else if (tag < 2 * kPer) {
            w1 &= ~((~0ull) >> ((tag - kPer) * BITS));
        }
    }
    k0 = w0;
    k1 = w1;
    tt = (tag << 16) | (tag < 2 * kPer ? (term & 0xffffu) : 0u);
}

// kTiled = false: one workgroup per queue entry (a group of up to NMAX members), grid (kQShards, Y).
// kTiled = true: one workgroup per tile of NMAX / 2 list positions; it takes the groups of up to NMAX / 2 members
//   that START in its tile -- all of them at once, as the segments the rounds begin with: sequence data leaves
//   hundreds of thousands of groups of two to eight members, and a wavefront per group would idle on their
//   round trips to the text.  List positions are sorted positions: a group's members hold consecutive list
//   positions (and slots), and sorting only ever moves members inside their group.
// kPivot: pivot rounds instead of window rounds (above); depth_cap: segments that agree that far stay tied.
// kTimed (NOLZSS_GROUP_SORT_PHASES): a separate instantiation whose thread 0 adds, in every 8th workgroup, the cycles of each
// phase to phases[0 .. 5] (set-up, scan, window, ranking, boundaries + next segments, output), the rounds to [6], the groups
// (tiles) to [7]; the words its scanning members needed to [8] and their number to [9].  The untimed form has none of it.
constexpr int kGroupSortPhaseWords = 16;
template <int BITS, int THREADS, int NMAX, bool kTiled, bool kPivot = false, bool kTimed = false>
__global__ __launch_bounds__(THREADS) void group_sort_kernel(ShardQueue q, const uint32_t *__restrict__ act_slot,
                                                             const uint32_t *__restrict__ act_grp, uint32_t m,
                                                             uint32_t *sa, const uint64_t *__restrict__ words,
                                                             TermTable terms, uint32_t h0,
                                                             uint32_t *__restrict__ out_lo,
                                                             uint32_t *__restrict__ lcp_list,
                                                             uint32_t *__restrict__ min_depth,
                                                             const uint32_t *__restrict__ lcp_mark, uint32_t max_rounds,
                                                             uint32_t depth_cap = 0xffffffffu,
                                                             unsigned long long *__restrict__ phases = nullptr) {
    constexpr uint32_t kPer = 64 / BITS;
    const bool wg_timed = kTimed && phases != nullptr && ((blockIdx.x + blockIdx.y) & 7) == 0;
    const bool timed = wg_timed && threadIdx.x == 0;
    __shared__ uint32_t s_stat[kTimed ? 2 : 1];  // (timed) words the scanning members needed, scanning members
    if (kTimed && timed) s_stat[0] = s_stat[1] = 0;
    unsigned long long ck_last = 0, ck_acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    auto tick = [&](int phase) {  // (the cycles since the last tick go to `phase`)
        if (kTimed && timed) {
            const unsigned long long now = __builtin_readcyclecounter();
            ck_acc[phase] += now - ck_last;
            ck_last = now;
        }
    };
    constexpr int kWavesB = THREADS / 64;
    constexpr uint32_t kTile = NMAX / 2;  // (tiled) list positions whose groups this workgroup takes
    static_assert(!kTiled || kTile == kGroupSortSmall, "a tile's span holds every small group that starts in it");
    // by member (= the position it was loaded from; never changes)
    __shared__ uint32_t s_pos[NMAX], s_lim[NMAX];
    __shared__ uint16_t s_term[NMAX], s_seg[NMAX];  // s_seg: sorted position of the first member of my segment
    __shared__ uint8_t s_act[NMAX];                 // my segment has more than one member
    // by sorted position
    __shared__ uint64_t s_key[NMAX], s_key2[NMAX];  // the window of the member at this position, and its
    __shared__ uint32_t s_tt[NMAX];                  // terminator word (group_window)
    __shared__ uint16_t s_ord[NMAX];       // member at this position
    __shared__ uint16_t s_gstart[NMAX];    // first position of the GROUP this position belongs to; 0xffff: not mine
    __shared__ uint8_t s_head[NMAX + 1];   // a segment starts here
    __shared__ uint8_t s_split[NMAX];      // [segment starts] a boundary appeared inside this segment in this round
    __shared__ uint8_t s_scanit[NMAX];     // [segment starts] the last round did not split it: scan ahead first
    __shared__ uint32_t s_blcp[NMAX];      // [new heads] LCP with the position in front
    __shared__ uint32_t s_depth[NMAX];     // [segment starts] symbols all members of the segment agree on
    __shared__ uint32_t s_tmp[NMAX];       // scratch: the depth of the next round (pivot rounds: first the minimum of the scans)
    __shared__ uint32_t s_dmin[kPivot ? 1 : NMAX];  // [segment starts, window rounds] depth of this round: the segment's own,
                                                    // or the minimum of its members' scans (preset by the round in front)
    __shared__ uint16_t s_end[kPivot ? 1 : NMAX];   // [segment starts, window rounds] position behind the segment's last member
    __shared__ uint32_t s_scan[kWavesB + 1];
    __shared__ uint32_t s_any;
    const uint32_t t = threadIdx.x;
    const uint32_t shard = blockIdx.x;
    const uint32_t count = kTiled ? 1u : q.counts[shard * kQPad];
    // (queue kernels) items are TAKEN, not dealt: the first gridDim.y items of a shard go to its workgroups by their number,
    // every further one to whoever asks the shard's second counter first -- a workgroup that drew slow groups leaves the
    // others to its neighbours.  One atomic per item, asked for while the group before is set up; nobody waits for anybody.
    __shared__ uint32_t s_item;
    for (uint32_t item = kTiled ? 0u : blockIdx.y; item < count;) {
        // list positions [base, base + span): position e of the arrays is list element base + e
        uint32_t base, span, N;
        if (kTiled) {
            base = blockIdx.x * kTile;
            span = m - base < (uint32_t)NMAX ? m - base : (uint32_t)NMAX;
            N = NMAX;
        } else {
            base = q.items[(size_t)shard * q.cap + item];
            span = q.items2[(size_t)shard * q.cap + item];
            N = 2;
            while (N < span) N <<= 1;
        }
        __syncthreads();  // (the arrays of the group before this one are done with)
        uint32_t next_item = 0;
        if (!kTiled && t == 0) next_item = gridDim.y + atomicAdd(q.counts + shard * kQPad + 1, 1u);
        if (kTimed && timed) {
            ck_last = __builtin_readcyclecounter();
            ck_acc[7] += 1;
        }
        if (kTiled) {  // sizes of the groups that start in the tile, told by their last member
            for (uint32_t e = t; e < (uint32_t)NMAX; e += THREADS) s_tmp[e] = 0;
            __syncthreads();
            for (uint32_t e = t; e < span; e += THREADS) {
                const uint32_t a = base + e, g = act_grp[a], j = act_slot[a] - g;
                if ((a + 1 == m || act_grp[a + 1] != g) && j <= e && e - j < kTile) s_tmp[e - j] = j + 1;
            }
            __syncthreads();
        }
        for (uint32_t e = t; e < N; e += THREADS) {
            bool mine = e < span;
            uint32_t j = e, slot = 0;
            if (kTiled && mine) {
                const uint32_t a = base + e, g = act_grp[a];
                slot = act_slot[a];
                j = slot - g;
                mine = j <= e && e - j < kTile;                    // my group starts in this tile ...
                if (mine) {
                    const uint32_t gs = s_tmp[e - j];
                    mine = gs != 0 && gs <= kGroupSortSmall;       // ... and is small
                    if (mine && lcp_mark != nullptr) mine = lcp_mark[g + 1] == kLcpPending;  // ... and was not compared yet
                    if constexpr (!kPivot)
                        if (mine && j + 1 == gs) s_end[e - j] = (uint16_t)(e + 1);  // (the group's last member)
                }
            } else if (mine) {
                slot = act_grp[base] + e;  // (the group's members hold the slots from its head slot on)
                if constexpr (!kPivot)
                    if (e + 1 == span) s_end[0] = (uint16_t)span;
            }
            uint32_t p = 0, lim = 0, term = 0;
            if (mine) {
                p = sa[slot];
                lim = term_limit(terms, p, term);
            }
            s_pos[e] = p;
            s_lim[e] = lim;
            s_term[e] = (uint16_t)term;
            // what is not mine is a segment of its own (it never moves) -- behind the span: sorts behind everything
            s_seg[e] = mine ? (uint16_t)(e - j) : (e < span ? (uint16_t)e : (uint16_t)0xffff);
            s_gstart[e] = mine ? (uint16_t)(e - j) : (uint16_t)0xffff;
            s_act[e] = mine ? 1 : 0;  // (a group of the list has at least two members)
            s_key[e] = 0;
            s_key2[e] = 0;
            s_tt[e] = 0;
            s_scanit[e] = 0;
            s_ord[e] = (uint16_t)e;
            s_head[e] = (!mine || j == 0) ? 1 : 0;
            s_blcp[e] = kLcpPending;
            s_depth[e] = h0;
            if constexpr (!kPivot) s_dmin[e] = h0;  // (the first round does not scan)
        }
        if (t == 0) {
            s_head[N] = 1;
            s_item = next_item;
        }
        __syncthreads();
        tick(0);
        bool tied = true;
        for (uint32_t round = 0; tied && round < max_rounds; ++round) {
            if (kTimed && timed) ck_acc[6] += 1;
            constexpr int kE = NMAX / THREADS;  // positions per thread: e = t + k * THREADS
            uint64_t rk0[kE], rk1[kE];
            uint32_t rtt[kE], rmem[kE], rhs[kE];
            bool ract[kE];
            if constexpr (kPivot) {
                // ---- 1p. every member against the first member of its segment
#pragma unroll
                for (int k = 0; k < kE; ++k) {
                    const uint32_t e = t + (uint32_t)k * THREADS;
                    ract[k] = false;
                    rk0[k] = rk1[k] = 0;
                    rtt[k] = rmem[k] = rhs[k] = 0;
                    if (e >= span) continue;
                    const uint32_t mem = s_ord[e];
                    if (!s_act[mem]) continue;
                    ract[k] = true;
                    rmem[k] = mem;
                    const uint32_t hs = s_seg[mem];
                    rhs[k] = hs;
                    s_split[e] = 0;
                    uint64_t key = pivot_key(1u, 0u, 0u, 0u);  // the pivot itself, and what equals it as far as compared
                    if (e != hs) {
                        const uint32_t D = s_depth[hs];
                        const uint32_t lead = s_ord[hs];
                        const uint32_t la = s_lim[mem], lb = s_lim[lead];
                        const uint32_t limit = la < lb ? la : lb;  // symbols before the nearer terminator
                        uint32_t stop = D + kPivotWords * kPer;
                        stop = stop < depth_cap ? stop : depth_cap;
                        const uint32_t stop2 = limit < stop ? limit : stop;
                        const uint64_t pa = s_pos[mem], pb = s_pos[lead];
                        constexpr uint32_t kPer32 = 32 / BITS;
                        uint32_t h = D, xw = 0, yw = 0;
                        bool found = false;
                        while (h < stop2) {
                            uint32_t x[2 * kPivotBatch], y[2 * kPivotBatch];
                            pivot_fetch<BITS>(words, pa, h, x);
                            pivot_fetch<BITS>(words, pb, h, y);
                            uint32_t fb = 2 * kPivotBatch;
#pragma unroll
                            for (int b = 2 * (int)kPivotBatch - 1; b >= 0; --b) {
                                const bool diff = x[b] != y[b];
                                fb = diff ? (uint32_t)b : fb;
                                xw = diff ? x[b] : xw;
                                yw = diff ? y[b] : yw;
                            }
                            if (fb < 2 * kPivotBatch) {
                                h += fb * kPer32 + (uint32_t)__clz((int)(xw ^ yw)) / BITS;
                                found = true;
                                break;
                            }
                            h += kPivotBatch * kPer;
                        }
                        if (found && h < stop2) {  // a difference in front of both terminators and of the round's reach
                            const uint32_t in_word = (uint32_t)__clz((int)(xw ^ yw)) / BITS;
                            const uint32_t sym = (xw >> (32 - BITS * (in_word + 1))) & ((1u << BITS) - 1u);
                            key = pivot_key(xw < yw ? 0u : 2u, h - D, sym + 1u, 0u);
                        } else if (limit <= stop) {  // a terminator is reached first
                            if (la < lb) {  // mine: the suffix that ends is the smaller one
                                key = pivot_key(0u, limit - D, 0u, (uint32_t)s_term[mem] + 1u);
                            } else if (la > lb) {  // the pivot's: I go on with a symbol of my own
                                const uint32_t sym = (uint32_t)(sym_word<BITS>(words, pa + limit) >> (64 - BITS));
                                key = pivot_key(2u, limit - D, sym + 1u, 0u);
                            } else {  // both end here: the lower terminator index first
                                key = pivot_key(s_term[mem] < s_term[lead] ? 0u : 2u, limit - D, 0u, (uint32_t)s_term[mem] + 1u);
                            }
                        }
                        // (else: equal as far as this round looks: the pivot's class)
                    }
                    rk0[k] = key;
                    s_key[e] = key;
                }
                __syncthreads();
                tick(1);
            } else {
            // ---- 1. ONE trip to the text per round.  A segment that the last round did not split scans: how far does every
            // member agree with its first member (up to kScanWords words)?  The segment's depth is the minimum, known behind
            // the barrier, and the window stands there -- so a member of such a segment (its first member too) asks for
            // its kScanFetch words at once, those of the first member next to them, and cuts its window out of them when the
            // depth is known (kCut: one position per thread; with more the words would not stay in registers, and the
            // window is fetched behind the barrier as it used to be).  The others take their window where they stand.
            constexpr bool kCut = kE == 1;
            uint32_t xs[kCut ? 2 * kScanFetch : 1], rd0 = 0;
            bool cut = false;
#pragma unroll
            for (int k = 0; k < kE; ++k) {
                const uint32_t e = t + (uint32_t)k * THREADS;
                ract[k] = false;
                rk0[k] = rk1[k] = 0;
                rtt[k] = rmem[k] = rhs[k] = 0;
                if (e >= span) continue;
                const uint32_t mem = s_ord[e];
                s_split[e] = 0;
                if (!s_act[mem]) continue;
                ract[k] = true;
                rmem[k] = mem;
                const uint32_t hs = s_seg[mem];
                rhs[k] = hs;
                const uint32_t d0 = s_depth[hs];
                const uint32_t la = s_lim[mem];
                const uint64_t pa = s_pos[mem];
                if (!s_scanit[hs]) {
                    if constexpr (kCut) {
                        group_window<BITS>(words, (uint32_t)pa, d0, la, s_term[mem], rk0[k], rk1[k], rtt[k]);
                        s_key[e] = rk0[k];
                        s_key2[e] = rk1[k];
                        s_tt[e] = rtt[k];
                    }
                    continue;
                }
                const uint32_t lead = s_ord[hs];
                const uint32_t lb = s_lim[lead];
                const uint32_t limit = la < lb ? la : lb;
                const uint32_t stop = d0 + kScanWords * kPer;
                uint32_t h = d0;
                if constexpr (kCut) {
                    cut = true;
                    rd0 = d0;
#pragma unroll
                    for (uint32_t c = 0; c < 2 * kScanFetch; ++c) xs[c] = 0;
                    if (d0 < la) pivot_fetch<BITS, kScanFetch>(words, pa, d0, xs);
                    if (e != hs && d0 < limit) {
                        uint32_t y[2 * kScanWords];
                        pivot_fetch<BITS, kScanWords>(words, (uint64_t)s_pos[lead], d0, y);
                        h = d0 + scan_first_diff<BITS>(xs, y);
                    }
                } else {
                    if (e != hs && d0 < limit) {
                        uint32_t x[2 * kScanWords], y[2 * kScanWords];
                        pivot_fetch<BITS, kScanWords>(words, pa, d0, x);
                        pivot_fetch<BITS, kScanWords>(words, (uint64_t)s_pos[lead], d0, y);
                        h = d0 + scan_first_diff<BITS>(x, y);
                    }
                }
                if (e == hs) continue;  // (the first member itself: somebody else reports)
                h = h < limit ? h : limit;
                h = h < stop ? h : stop;
                if (kTimed && wg_timed) {  // words this member needed
                    atomicAdd(&s_stat[0], d0 < limit ? (h - d0) / kPer + (h < stop ? 1u : 0u) : 0u);
                    atomicAdd(&s_stat[1], 1u);
                }
                atomicMin(&s_dmin[hs], h);
            }
            __syncthreads();
            tick(1);
            // ---- 2. the window at the segment's depth: kept in registers and parked BY POSITION for the ranking
#pragma unroll
            for (int k = 0; k < kE; ++k) {
                const uint32_t e = t + (uint32_t)k * THREADS;
                if (!ract[k]) continue;
                const uint32_t D = s_dmin[rhs[k]];
                if constexpr (kCut) {
                    if (cut) {
                        const uint32_t mem = rmem[k];
                        group_window_cut<BITS>(xs, rd0, D, s_lim[mem], s_term[mem], rk0[k], rk1[k], rtt[k]);
                        s_key[e] = rk0[k];
                        s_key2[e] = rk1[k];
                        s_tt[e] = rtt[k];
                    }
                } else {
                    const uint32_t mem = rmem[k];
                    group_window<BITS>(words, s_pos[mem], D, s_lim[mem], s_term[mem], rk0[k], rk1[k], rtt[k]);
                    s_key[e] = rk0[k];
                    s_key2[e] = rk1[k];
                    s_tt[e] = rtt[k];
                }
                if (rhs[k] == e) s_depth[e] = D;  // (a segment start: read in front of the barrier, written here)
            }
            __syncthreads();
            tick(2);
            }  // (!kPivot)
            // ---- 3. my place inside my segment: members with a smaller (window, terminator), plus the equal ones in
            // front of me.  Every lane walks its own segment (the members of a segment read the same entries: LDS
            // broadcasts); segments shrink round by round, so the walks get short quickly -- a sorting network over
            // the whole group paid log^2 N dependent LDS round trips in every round.
            uint32_t npos[kE];
#pragma unroll
            for (int k = 0; k < kE; ++k) {
                const uint32_t e = t + (uint32_t)k * THREADS;
                npos[k] = e;
                if (!ract[k]) continue;
                uint32_t less = 0, eqb = 0;
                if constexpr (kPivot) {  // one key word per member
                    for (uint32_t x = rhs[k];; ++x) {
                        if (x > rhs[k] && s_head[x]) break;
                        const uint64_t xk = s_key[x];
                        less += xk < rk0[k] ? 1u : 0u;
                        eqb += (xk == rk0[k] && x < e) ? 1u : 0u;
                    }
                    npos[k] = rhs[k] + less + eqb;
                    continue;
                }
                // (the segment's end is known, s_end: four first words are read at a time, none of them waits for a test
                // of the one in front; the second word and the terminator word only where the first one is equal)
                const uint32_t end = s_end[rhs[k]];
                const uint64_t my0 = rk0[k], my1 = rk1[k];
                const uint32_t mytt = rtt[k];
                auto rest = [&](uint32_t x) {  // an entry whose first word equals mine
                    const uint64_t xk1 = s_key2[x];
                    const uint32_t xtt = s_tt[x];
                    less += (xk1 != my1 ? xk1 < my1 : xtt < mytt) ? 1u : 0u;
                    eqb += (xk1 == my1 && xtt == mytt && x < e) ? 1u : 0u;
                };
                uint32_t x = rhs[k];
                for (; x + 4 <= end; x += 4) {
                    uint64_t a[4];
#pragma unroll
                    for (uint32_t c = 0; c < 4; ++c) a[c] = s_key[x + c];
                    bool same = false;
#pragma unroll
                    for (uint32_t c = 0; c < 4; ++c) {
                        less += a[c] < my0 ? 1u : 0u;
                        same |= a[c] == my0;
                    }
                    if (same) {
#pragma unroll
                        for (uint32_t c = 0; c < 4; ++c)
                            if (a[c] == my0) rest(x + c);
                    }
                }
                for (; x < end; ++x) {
                    const uint64_t xk0 = s_key[x];
                    if (xk0 == my0) rest(x);
                    else less += xk0 < my0 ? 1u : 0u;
                }
                npos[k] = rhs[k] + less + eqb;
            }
            __syncthreads();
            tick(3);
#pragma unroll
            for (int k = 0; k < kE; ++k) {
                if (!ract[k]) continue;
                s_ord[npos[k]] = (uint16_t)rmem[k];
                s_key[npos[k]] = rk0[k];
                s_key2[npos[k]] = rk1[k];
                s_tt[npos[k]] = rtt[k];
            }
            __syncthreads();
            // ---- 4. new boundaries inside the old segments, with their LCP; depth of the next round
            for (uint32_t e = t; e < span; e += THREADS) {
                const uint32_t mem = s_ord[e];
                if (!s_act[mem]) continue;
                const uint32_t hs = s_seg[mem];
                const uint32_t D = s_depth[hs];
                if constexpr (kPivot) {
                    // members that stay together: the pivot's class agrees as far as the round looked, the others
                    // on their common l and the symbol behind it
                    const uint64_t ka = s_key[e];
                    const uint32_t la = pivot_lrel_of(ka);
                    uint32_t stop = D + kPivotWords * kPer;
                    stop = stop < depth_cap ? stop : depth_cap;
                    s_tmp[e] = la == 0xffffffffu ? stop : D + la + 1u;
                    if (e == hs) continue;
                    const uint64_t kb = s_key[e - 1];
                    if (ka != kb) {
                        const uint32_t lb = pivot_lrel_of(kb);
                        s_head[e] = 1;
                        s_split[hs] = 1;
                        s_blcp[e] = D + (la < lb ? la : lb);
                    }
                    continue;
                }
                s_tmp[e] = D + 2 * kPer;  // members that stay together agree on the whole window
                if (e == hs) continue;
                const uint64_t ka = s_key[e], kb = s_key[e - 1], ka2 = s_key2[e], kb2 = s_key2[e - 1];
                const uint32_t ta = s_tt[e], tb = s_tt[e - 1];
                if (ka != kb || ka2 != kb2 || ta != tb) {
                    uint32_t d = 2 * kPer;
                    if (ka != kb)
                        d = (uint32_t)__clzll((long long)(ka ^ kb)) / BITS;
                    else if (ka2 != kb2)
                        d = kPer + (uint32_t)__clzll((long long)(ka2 ^ kb2)) / BITS;
                    const uint32_t va = ta >> 16, vb = tb >> 16;
                    const uint32_t valid = va < vb ? va : vb;
                    s_head[e] = 1;
                    s_split[hs] = 1;
                    s_blcp[e] = D + (d < valid ? d : valid);
                }
            }
            __syncthreads();
            // ---- 5. segments of the next round: start of my segment = nearest head at or in front of me
            {
                const uint32_t K = N > (uint32_t)THREADS ? N / THREADS : 1u;
                const uint32_t e0 = t * K;
                uint32_t last = 0;  // (position + 1) of the last head in my chunk
                if (e0 < N)
                    for (uint32_t k = 0; k < K; ++k)
                        if (s_head[e0 + k]) last = e0 + k + 1;
                uint32_t total;
                uint32_t run = block_scan_exclusive<kWavesB>(last, OpMax<uint32_t>(), s_scan, total);
                if (t == 0) s_any = 0;
                __syncthreads();
                bool any = false;
                if (e0 < N)
                    for (uint32_t k = 0; k < K; ++k) {
                        const uint32_t e = e0 + k;
                        if (s_head[e]) run = e + 1;
                        if (e >= span) continue;
                        const uint32_t mem = s_ord[e];
                        const bool was = s_act[mem] != 0;
                        if (!was) continue;  // (finished members, and what is not mine, keep their state)
                        const uint32_t hs = run - 1;
                        const uint32_t old_hs = s_seg[mem];
                        s_seg[mem] = (uint16_t)hs;
                        bool act = !(s_head[e] && s_head[e + 1]);
                        if constexpr (kPivot) {
                            // a segment that agrees up to the cap stays tied: the doubling rounds start at its depth
                            // (s_tmp of a position: the depth of the class it sits in, equal for the whole new segment)
                            if (act && s_tmp[hs] >= depth_cap) {
                                act = false;
                                if (hs == e) lower_min(min_depth, s_tmp[e]);
                            }
                        }
                        s_act[mem] = act ? 1 : 0;
                        any |= act;
                        if (hs == e) {  // a segment start (old or new) of a segment that was tied
                            s_depth[e] = s_tmp[e];
                            const bool scan = kPivot ? false : s_split[old_hs] == 0;
                            s_scanit[e] = scan ? 1 : 0;
                            if constexpr (!kPivot) s_dmin[e] = scan ? 0xffffffffu : s_tmp[e];
                        }
                        if constexpr (!kPivot)
                            if (s_head[e + 1]) s_end[hs] = (uint16_t)(e + 1);  // (the segment's last member)
                    }
                if (any) s_any = 1;
                __syncthreads();
                tied = s_any != 0;
            }
            tick(4);
        }
        // ---- output
        if (tied) {  // the depth every group that stays tied agrees on (the doubling rounds start there)
            uint32_t dmin = 0xffffffffu;
            for (uint32_t e = t; e < span; e += THREADS) {
                const uint32_t mem = s_ord[e];
                if (s_act[mem] && s_seg[mem] == e) dmin = s_depth[e] < dmin ? s_depth[e] : dmin;
            }
            dmin = wave_reduce(dmin, OpMinU32x());
            if (lane_id() == 0 && dmin != 0xffffffffu) lower_min(min_depth, dmin);
        }
        for (uint32_t e = t; e < span; e += THREADS) {
            const uint32_t gs = s_gstart[e];
            if (gs == 0xffffu) continue;
            const uint32_t mem = s_ord[e];
            const uint32_t a = base + e;
            sa[kTiled ? act_slot[a] : act_grp[base] + e] = s_pos[mem];
            out_lo[a] = (uint32_t)s_seg[mem] - gs;  // strictly smaller members of my group
            lcp_list[a] = e == gs ? 0u : (s_head[e] ? s_blcp[e] : kLcpPending);
        }
        tick(5);
        item = kTiled ? count : s_item;  // (written in front of the barrier behind the set-up, next behind the one at the top)
    }
    if (kTimed && timed) {
#pragma unroll
        for (int k = 0; k < 8; ++k) atomicAdd(phases + k, ck_acc[k]);
        atomicAdd(phases + 8, (unsigned long long)s_stat[0]);
        atomicAdd(phases + 9, (unsigned long long)s_stat[1]);
    }
}
