// sa_regroup.hip -- the shared tail of every round of the suffix-array construction: the sorted view of the suffixes
// that are still tied becomes group heads, ranks, the LCP of every boundary that appeared and the compacted list of
// the suffixes still tied -- one single-pass kernel with decoupled look-back (regroup_kernel).  Beside it the two other
// producers of an active list or of rank[]: the survivors of the direct round (compact_survivors) and the one pass
// that writes rank[] for everybody (write_all_ranks) -- and the safety net behind the LCP values the rounds decide
// (lcp_finish_kernel, build_lcp_pyramid).  Shared declarations: sa_internal.hpp.
#include "sa_internal.hpp"

#include "lookback.hpp"
#include "scan.hpp"

namespace nolzss {

namespace {

// ---------------------------------------------------------------------------------------
// regrouping after a sort
// ---------------------------------------------------------------------------------------
// The sorted view of the m active elements is either the 64-bit round-0 keys (kRound0) or, in
// the doubling rounds, the pair (grp[a], lo[a]) = (slot of the element's current group head,
// rank of the suffix h symbols further on).  Element a starts a new group iff its view differs
// from element a-1.
template <bool kRound0>
__device__ __forceinline__ bool is_head(const uint64_t *__restrict__ keys, const uint32_t *__restrict__ grp,
                                        const uint32_t *__restrict__ lo, size_t a) {
    if (a == 0) return true;
    if (kRound0) return keys[a] != keys[a - 1];
    return grp[a] != grp[a - 1] || lo[a] != lo[a - 1];
}

// ---- single-pass regroup --------------------------------------------------------------------
// One kernel does what used to be five passes (mark heads, max-scan, commit, add-scan, compact):
// every workgroup takes the next tile of the sorted view (ticket order), finds the group heads,
// and obtains the two running values it needs from the tiles in front of it -- the slot of the
// last group head (a max-scan) and the number of elements that stay active (an add-scan) -- by
// decoupled look-back over per-tile descriptors in HBM: [status : value] in one 64-bit word,
// status 1 = the tile's own aggregate, 2 = inclusive prefix.  Tickets are handed out in start
// order, so a workgroup only ever waits for workgroups that are already running.
// It then writes the new order (sa), the rank of every element (slot of its group head + 1), the
// LCP of every boundary that became known, and the compacted active list for the next round.
// HBM traffic at round 0: 12 B read + 12 B written per suffix plus 8 B per surviving element,
// where the five passes moved ~88 B.
constexpr int kFuseThreads = 512;  // 8 items per thread keep the registers low: 4 workgroups = 32 waves per CU
constexpr int kFuseItems = 8;
constexpr int kFuseTile = kFuseThreads * kFuseItems;
// Both running values in ONE descriptor, [status:2 | last head slot:31 | kept:31], for lists shorter
// than 2^31: one walk over the tiles in front instead of two.  (The walk is what a regroup tile
// waits for -- with ~1800 small tiles in flight, most of them published but not yet finished, it
// goes back through dozens of 64-descriptor windows, each a device-scope round trip.)
struct MaxSum {
    uint32_t mx, sum;
};
__device__ __forceinline__ uint64_t pack_desc(uint32_t status, MaxSum v) {
    return ((uint64_t)status << 62) | ((uint64_t)v.mx << 31) | (uint64_t)v.sum;
}
#ifndef NOLZSS_LOOKBACK_WINDOWS
#define NOLZSS_LOOKBACK_WINDOWS 1
#endif
__device__ __forceinline__ MaxSum lookback_exclusive_packed(uint64_t *desc, uint32_t tile, MaxSum aggregate,
                                                            uint32_t *err) {
    // kWin windows of 64 descriptors are loaded per round trip and evaluated nearest first.  (Measured with
    // NOLZSS_REGROUP_PHASES at 2^30: a tile spends 27 k cycles on loads and heads, 15 k in this walk, 6 k on
    // its output; four windows per round trip did not shorten the walk -- it waits for the slowest of the
    // tiles in front to publish, not for the number of descriptors -- so one window stays the default.)
    constexpr int kWin = NOLZSS_LOOKBACK_WINDOWS;
    const int lane = lane_id();
    MaxSum excl{0u, 0u};
    if (tile == 0) {
        if (lane == 0) desc_store(desc, pack_desc(2u, aggregate));
        return excl;
    }
    if (lane == 0) desc_store(desc + tile, pack_desc(1u, aggregate));
    int64_t look = (int64_t)tile - 1;
    uint32_t spins = 0;
    for (;;) {
        uint64_t d[kWin];
#pragma unroll
        for (int j = 0; j < kWin; ++j) {
            const int64_t idx = look - 64 * j - lane;
            d[j] = idx >= 0 ? desc_load(desc + idx) : (2ull << 62);  // in front of tile 0: inclusive identity
        }
        bool done = false, stalled = false;
#pragma unroll
        for (int j = 0; j < kWin; ++j) {
            if (done || stalled) continue;  // (wave-uniform)
            const uint32_t st = (uint32_t)(d[j] >> 62);
            const uint64_t inc = __ballot(st == 2);
            // every lane up to and including the first inclusive one must have been published
            const uint64_t need = inc ? (((inc & (~inc + 1ull)) << 1) - 1ull) : ~0ull;
            const uint64_t missing = __ballot(st == 0) & need;
            if (missing) {  // not published yet: wait and read again from this window on
                stalled = true;
                continue;
            }
            const bool use = (need >> lane) & 1ull;
            const uint32_t vm = use ? (uint32_t)(d[j] >> 31) & 0x7fffffffu : 0u;
            const uint32_t vs = use ? (uint32_t)d[j] & 0x7fffffffu : 0u;
            const uint32_t wm = wave_reduce(vm, OpMax<uint32_t>());
            excl.mx = wm > excl.mx ? wm : excl.mx;
            excl.sum += wave_reduce(vs, OpAdd<uint32_t>());
            look -= 64;
            if (inc) done = true;  // an inclusive prefix was reached
        }
        if (done) break;
        if (stalled) {
            if (++spins > kSpinLimit) {  // cannot happen with ticket order; never hang the GPU
                if (lane == 0) atomicExch(err, 1u);
                return excl;
            }
            __builtin_amdgcn_s_sleep(1);
        }
    }
    if (lane == 0) {
        MaxSum incl{excl.mx > aggregate.mx ? excl.mx : aggregate.mx, excl.sum + aggregate.sum};
        desc_store(desc + tile, pack_desc(2u, incl));
    }
    return excl;
}

struct RegroupArgs {
    const uint64_t *keys;     // round 0: sorted keys ...
    const uint32_t *keys32;   // ... or their low halves, the top byte implied by the bucket (seg)
    SegView seg;
    uint32_t num_tiles;
    uint32_t short_tag;       // round 0: elements whose length tag is below this are groups of their own
    uint32_t seq_shift;       // round 0, independent sequences: key bits from here up = number of the sequence
    int sa_is_current;        // the producer has already written the new order into sa (direct round)
    const uint32_t *grp;      // later rounds: (group head slot, secondary key) per list element
    const uint32_t *lo;
    const uint32_t *vals;     // suffix start per element
    const uint32_t *act_slot; // later rounds: slot per list element
    uint32_t m;
    uint32_t *sa;
    uint32_t *rank_val;       // (when rank_by_slot == nullptr) new rank of the elements whose rank changes ...
    uint32_t *chg_idx;        // ... and their suffix starts, appended in any order; chg_count counts them
    uint32_t *chg_count;
    uint32_t *rank_by_slot;   // non-null: the rounds before rank[] exists (no list of changed ranks is kept)
    int store_ranks;          // ... and the rank of every slot is stored there
    uint32_t *lcp;
    int sym_bits, tag_bits, bits, low_bits;  // round 0 key layout
    int bits_shift;                          // log2(bits): a division by a run-time value costs ~20 instructions per item
    const uint32_t *lcp_list; // later rounds: LCP decided by the direct comparison round
    uint32_t dbl_h;
    Pyramid Plcp;
    uint32_t *new_slot, *new_grp;  // compacted active list of the next round
    uint64_t *desc_max, *desc_sum;
    int packed;               // both scans share the descriptors in desc_max (n < 2^31)
    uint32_t *ticket;         // [0] tile tickets, [1] error flag
    uint32_t *d_total;        // number of elements that stay active
    unsigned long long *phases;  // (diagnostics, NOLZSS_REGROUP_PHASES) cycles per phase, summed over sampled tiles
};

// value of the previous / next lane of the wavefront (lane 0 / lane 63 keep `edge`)
__device__ __forceinline__ uint32_t lane_prev(uint32_t v, uint32_t edge) {
    return (uint32_t)__builtin_amdgcn_update_dpp((int)edge, (int)v, 0x138, 0xf, 0xf, false);  // wave_shr:1
}
__device__ __forceinline__ uint32_t lane_next(uint32_t v, uint32_t edge) {
    return (uint32_t)__builtin_amdgcn_update_dpp((int)edge, (int)v, 0x130, 0xf, 0xf, false);  // wave_shl:1
}

// kLayout (round 0 of the bucketed 2-bit key sorts): the key layout is known at compile time, which folds the
// shifts and masks of every item (the kernel is bound by VALU issue: ~1300 instructions per wavefront and 512
// suffixes).  1 = plain DNA: 34 symbol bits, 6-bit tag, no low bits, no sequence numbers, short suffixes flagged;
// 2 = long independent records, bucket = record: 28 symbol bits, 4-bit tag, the record number above bit 32;
// 3 = plain DNA with the 16-base key: 32 symbol bits (bucket + 24 stored bits), the tag in the low byte of the stored word;
// 4 = plain DNA with the 35-bit key: 35 "symbol" bits (bucket + 27 stored bits, 17 1/2 bases), a 5-bit tag, short below 17.
template <bool kRound0, int kLayout>
__global__ __launch_bounds__(kFuseThreads) void regroup_kernel(RegroupArgs A) {
    constexpr bool kDnaFast = kLayout != 0;  // (bucketed, compile-time layout)
    const int low_bits = kDnaFast ? 0 : A.low_bits;
    const int tag_bits = kLayout == 1 ? KeyLayout<2>::kTagBits : (kLayout == 2 ? kRecTagBits : (kLayout == 3 ? kP16TagBits : (kLayout == 4 ? kP35TagBits : A.tag_bits)));
    const int sym_bits = kLayout == 1 ? 2 * KeyLayout<2>::kSyms : (kLayout == 2 ? 2 * kRecSyms : (kLayout == 3 ? 2 * kP16Syms : (kLayout == 4 ? kP35KeyBits : A.sym_bits)));
    const int bits_shift = kDnaFast ? 1 : A.bits_shift;
    const uint32_t short_tag = kLayout == 1 ? (uint32_t)KeyLayout<2>::kSyms : (kLayout == 2 ? 0u : (kLayout == 3 ? (uint32_t)kP16Syms : (kLayout == 4 ? (uint32_t)kP35Syms : A.short_tag)));
    const uint32_t seq_shift = (kLayout == 1 || kLayout == 3 || kLayout == 4) ? 0u : (kLayout == 2 ? 32u : A.seq_shift);
    constexpr int kWaves = kFuseThreads / 64;
    constexpr int kSegs = kFuseItems * kWaves;  // 64-element segments of the tile, in element order
    __shared__ uint32_t s_tile;
    __shared__ uint32_t s_seg_max[kSegs], s_seg_sum[kSegs];  // per segment: last head slot, kept; then prefixes
    __shared__ uint32_t s_excl[2];
    const bool timed = A.phases != nullptr && (blockIdx.x & 15) == 0 && threadIdx.x == 0;
    unsigned long long clk[5] = {0, 0, 0, 0, 0};
    if (timed) clk[0] = __builtin_readcyclecounter();
    if (threadIdx.x == 0) s_tile = atomicAdd(A.ticket, 1u);  // (blockIdx order measured 5 % faster, not guaranteed)
    __syncthreads();
    if (timed) clk[1] = __builtin_readcyclecounter();
    const uint32_t tile = s_tile;
    const uint32_t m = A.m;
    // the regroup tiles are the tiles of the segmented sort, or kSubTiles equal pieces of each (a piece behind
    // the end of a partial sort tile is empty)
    static_assert(kSortTile % kFuseTile == 0, "a sort tile is a whole number of regroup tiles");
    constexpr uint32_t kSubTiles = kSortTile / kFuseTile;
    TileExtent ext;
    if (A.seg.desc == nullptr) {
        ext = tile_extent(0, m, 1, A.seg);
        ext.first = (size_t)tile * kFuseTile;
        ext.count = (uint32_t)((m - ext.first < (size_t)kFuseTile) ? (m - ext.first) : (size_t)kFuseTile);
    } else {
        ext = tile_extent(tile / kSubTiles, m, A.num_tiles / kSubTiles, A.seg);
        const uint32_t off = (tile % kSubTiles) * (uint32_t)kFuseTile;
        const uint32_t skip = off < ext.count ? off : ext.count;
        ext.first += skip;
        ext.count -= skip;
        ext.count = ext.count < (uint32_t)kFuseTile ? ext.count : (uint32_t)kFuseTile;
    }
    const size_t tile_base = ext.first;
    const int lane = lane_id();
    const int w = threadIdx.x >> 6;
    const uint64_t lt = lanemask_lt();
    const bool bucketed = kDnaFast || (kRound0 && A.keys32 != nullptr);

    auto load_view = [&](size_t a) -> uint64_t {
        if (kRound0) {
            if (!bucketed) return A.keys[a];
            // the element's bucket: the tile's own, unless a is a neighbour across the bucket's end
            const uint32_t b = a < ext.bkt_first ? ext.prev_ne : (a >= ext.bkt_end ? ext.next_ne : ext.bucket);
            return ((uint64_t)b << 32) | A.keys32[a];
        }
        return ((uint64_t)A.grp[a] << 32) | A.lo[a];
    };
    // striped: item k of thread t is element tile_base + k * kFuseThreads + t (coalesced rows).
    // Every load of the tile goes out first (the LCP stores further down may alias the inputs as
    // far as the compiler knows; interleaved, each of the 16 rows would wait for its own round
    // trips to HBM): the view of my elements, their slots, and per row ONE neighbour -- the
    // element in front of the wavefront for lane 0, the element behind it for lane 63.
    uint32_t slot[kFuseItems];
    uint64_t view[kFuseItems], edge[kFuseItems];
#pragma unroll
    for (int k = 0; k < kFuseItems; ++k) {
        const size_t a = tile_base + (size_t)k * kFuseThreads + threadIdx.x;
        const bool in = (uint32_t)k * kFuseThreads + threadIdx.x < ext.count;
        view[k] = in ? load_view(a) : 0ull;
        slot[k] = kRound0 ? (uint32_t)a : (in ? A.act_slot[a] : 0u);
        edge[k] = 0;
        if (lane == 0 && in && a > 0) edge[k] = load_view(a - 1);
        if (lane == 63 && in && a + 1 < m) edge[k] = load_view(a + 1);
    }
    uint64_t hmask[kFuseItems], kmask[kFuseItems];  // wave-uniform: heads / kept elements of my segment
    uint32_t old_head[kFuseItems];                  // later rounds: head slot of the group I come from
#pragma unroll
    for (int k = 0; k < kFuseItems; ++k) {
        const size_t a = tile_base + (size_t)k * kFuseThreads + threadIdx.x;
        const bool in = (uint32_t)k * kFuseThreads + threadIdx.x < ext.count;
        const uint64_t v = view[k];
        old_head[k] = (uint32_t)(v >> 32);
        // the element in front: the previous lane's, except for lane 0
        const uint64_t pv = ((uint64_t)lane_prev((uint32_t)(v >> 32), (uint32_t)(edge[k] >> 32)) << 32) |
                            lane_prev((uint32_t)v, (uint32_t)edge[k]);
        bool head = !in || a == 0 || v != pv;  // "past the end" counts as a head
        // a suffix that meets a terminator inside the key window ties only with copies of itself at
        // other terminators, and the stable sort has left those in their final order
        const bool short_head = kRound0 && short_tag && ((uint32_t)(v >> low_bits) & ((1u << tag_bits) - 1u)) < short_tag;
        head = head || short_head;
        // is the element behind me a head?  (across the wavefront's edge only its key is at hand: with my key it has my
        // tag, so it is short -- a head -- exactly if I am; a short suffix kept as "tied" with its copy at another
        // terminator went through the direct round as a group of one)
        const uint32_t edge_next = (lane == 63 && in && a + 1 < m) ? ((edge[k] != v || short_head) ? 1u : 0u) : 1u;
        const bool next_head = lane_next(head ? 1u : 0u, edge_next) != 0;
        const bool keep = in && !(head && next_head);
        hmask[k] = __ballot(in && head);
        kmask[k] = __ballot(keep);
        // the LCP of a boundary that has just appeared needs nothing from the other tiles
        if (in && !kRound0) {
            // a new boundary inside an old group
            if (head && a > 0 && (uint32_t)(v >> 32) == (uint32_t)(pv >> 32)) {
                uint32_t l = A.lcp_list ? A.lcp_list[a] : kLcpPending;
                if (l >= kLcpPendingMin) {
                    // created by a doubling step with offset h: the two suffixes agree on h symbols
                    // and continue with suffixes of DIFFERENT h-groups, whose LCP is the minimum of
                    // the boundaries already decided between those groups (undecided entries hold
                    // pending codes, i.e. +infinity):  lcp = h + min LCP(head1 .. head2]
                    const uint32_t p = (uint32_t)pv, q = (uint32_t)v;  // rank codes: head slot + 1
                    l = A.dbl_h;
                    if (p != 0) l += pyr_range<false>(A.Plcp, p, q - 1);
                }
                A.lcp[slot[k]] = l;
                // the range-minimum pyramid over the LCP array is kept up to date instead of being
                // rebuilt every round: a decided value only ever replaces a pending code (+infinity)
                for (int lev = 1; lev < A.Plcp.nlev; ++lev) {
                    uint32_t *up = const_cast<uint32_t *>(A.Plcp.lvl[lev]) + (slot[k] >> (kPyrShift * lev));
                    if (atomicMin(up, l) <= l) break;
                }
            }
        } else if (in) {
            // LCP of neighbours that round 0 already separates can be read off the two keys
            // (symbol prefix, capped by both length tags); the rest is marked pending.
            uint32_t l = kLcpPending;
            if (a == 0) {
                l = 0;
            } else if (head) {
                const uint64_t ka = v >> low_bits, kb = pv >> low_bits;
                const uint64_t tmask = (1ull << tag_bits) - 1ull;
                const uint32_t ta = (uint32_t)(ka & tmask), tb = (uint32_t)(kb & tmask);
                const uint64_t x = (ka ^ kb) >> tag_bits << (64 - sym_bits);  // symbols, left-aligned
                uint32_t ls = x ? (uint32_t)__clzll((long long)x) >> bits_shift : 0xffffffffu;  // (bits per symbol is 2, 4 or 8)
                ls = ls < ta ? ls : ta;
                l = ls < tb ? ls : tb;
                if (seq_shift && (v >> seq_shift) != (pv >> seq_shift)) l = 0;  // different sequences
            }
            A.lcp[a] = l;
        }
        // segment aggregate: slot of its last head (slots grow along the list), elements kept
        uint32_t last = 0;
        if (hmask[k]) last = (uint32_t)__builtin_amdgcn_readlane((int)slot[k], 63 - __builtin_clzll(hmask[k]));
        if (lane == 0) {
            s_seg_max[k * kWaves + w] = last;
            s_seg_sum[k * kWaves + w] = (uint32_t)__popcll(kmask[k]);
        }
    }
    __syncthreads();
    if (timed) clk[2] = __builtin_readcyclecounter();
    if (w == 0) {  // prefixes over the segments, then over the tiles in front
        static_assert(kSegs <= 64, "one lane per segment");
        const uint32_t vmax = lane < kSegs ? s_seg_max[lane] : 0u;
        const uint32_t vsum = lane < kSegs ? s_seg_sum[lane] : 0u;
        const uint32_t imax = wave_scan_inclusive_dpp(vmax, 0u, OpMax<uint32_t>());
        const uint32_t isum = wave_scan_inclusive_dpp(vsum, 0u, OpAdd<uint32_t>());
        const uint32_t agg_max = (uint32_t)__builtin_amdgcn_readlane((int)imax, 63);
        const uint32_t agg_sum = (uint32_t)__builtin_amdgcn_readlane((int)isum, 63);
        const uint32_t emax = lane_prev(imax, 0u);
        if (lane < kSegs) {
            s_seg_max[lane] = emax;
            s_seg_sum[lane] = isum - vsum;
        }
        uint32_t xm, xs;
        if (A.packed) {  // lists shorter than 2^31: one walk for both values
            const MaxSum x = lookback_exclusive_packed(A.desc_max, tile, MaxSum{agg_max, agg_sum}, A.ticket + 1);
            xm = x.mx;
            xs = x.sum;
        } else {
            xm = lookback_exclusive(A.desc_max, tile, agg_max, OpMax<uint32_t>(), A.ticket + 1);
            xs = lookback_exclusive(A.desc_sum, tile, agg_sum, OpAdd<uint32_t>(), A.ticket + 1);
        }
        if (lane == 0) {
            s_excl[0] = xm;
            s_excl[1] = xs;
            if (tile + 1 == A.num_tiles) *A.d_total = xs + agg_sum;  // the last tile
        }
    }
    __syncthreads();
    if (timed) clk[3] = __builtin_readcyclecounter();
    const uint32_t xmax = s_excl[0], xsum = s_excl[1];

    // slot of my group head: the last head at or in front of me
    auto head_slot = [&](int k, size_t a) -> uint32_t {
        const uint64_t mine = hmask[k] & ((2ull << lane) - 1ull);
        const int hl = mine ? 63 - __builtin_clzll(mine) : lane;
        uint32_t head_of = kRound0 ? (uint32_t)(a - (size_t)(lane - hl)) : (uint32_t)__shfl((int)slot[k], hl, 64);
        if (!mine) {
            const uint32_t pm = s_seg_max[k * kWaves + w];
            head_of = pm > xmax ? pm : xmax;
        }
        return head_of;
    };
    // Doubling rounds: rank[i] changes only for the members of groups that split off their old group
    // (on long exact repeats a round moves a few hundred of 10^8 tied suffixes).  Those go, in any
    // order, to the list that bucketed_scatter writes into rank[]: the tile counts them, takes its part
    // of the list with ONE atomic, and every wavefront appends its own.
    const bool list_changes = !kRound0 && !A.rank_by_slot;  // (uniform)
    uint64_t cmask[kFuseItems];
    uint32_t chg_base = 0;
    if (list_changes) {
        __shared__ uint32_t s_chg[kWaves + 1];
        uint32_t mine_total = 0;
#pragma unroll
        for (int k = 0; k < kFuseItems; ++k) {
            const size_t a = tile_base + (size_t)k * kFuseThreads + threadIdx.x;
            const bool in = (uint32_t)k * kFuseThreads + threadIdx.x < ext.count;
            cmask[k] = __ballot(in && head_slot(k, a) != old_head[k]);
            mine_total += (uint32_t)__popcll(cmask[k]);
        }
        if (lane == 0) s_chg[w] = mine_total;
        __syncthreads();
        if (threadIdx.x == 0) {
            uint32_t all = 0;
#pragma unroll
            for (int k = 0; k < kWaves; ++k) {
                const uint32_t c = s_chg[k];
                s_chg[k] = all;
                all += c;
            }
            s_chg[kWaves] = all ? atomicAdd(A.chg_count, all) : 0u;
        }
        __syncthreads();
        chg_base = s_chg[kWaves] + s_chg[w];
    }

#pragma unroll
    for (int k = 0; k < kFuseItems; ++k) {
        const size_t a = tile_base + (size_t)k * kFuseThreads + threadIdx.x;
        const bool in = (uint32_t)k * kFuseThreads + threadIdx.x < ext.count;
        const uint32_t head_of = head_slot(k, a);
        if (list_changes) {
            if ((cmask[k] >> lane) & 1ull) {
                const uint32_t q = chg_base + (uint32_t)__popcll(cmask[k] & lt);
                A.chg_idx[q] = A.vals[a];
                A.rank_val[q] = head_of + 1u;
            }
            chg_base += (uint32_t)__popcll(cmask[k]);
        }
        if (!in) continue;
        // (round 0: the key sort left the suffixes in sa itself; direct round: group_refine_kernel did)
        if (!kRound0 && !A.sa_is_current) A.sa[slot[k]] = A.vals[a];
        // (A.rank_by_slot != nullptr: rank[] is written later, in one pass -- or never: build_suffix_array, which then
        // asks for no store here; should ranks be needed after all, they are recovered from the LCP array)
        if (A.rank_by_slot && A.store_ranks) A.rank_by_slot[slot[k]] = head_of + 1u;
        if ((kmask[k] >> lane) & 1ull) {  // surviving elements keep their slot, learn their group head
            const uint32_t kk = xsum + s_seg_sum[k * kWaves + w] + (uint32_t)__popcll(kmask[k] & lt);
            A.new_slot[kk] = slot[k];
            A.new_grp[kk] = head_of;
        }
    }
    if (timed) {
        __builtin_amdgcn_s_waitcnt(0);
        clk[4] = __builtin_readcyclecounter();
        for (int k = 0; k < 4; ++k) atomicAdd(A.phases + k, clk[k + 1] - clk[k]);
        atomicAdd(A.phases + 4, 1ull);
    }
}

// the survivors of the direct round, region by region (one region of kRefineThreads entries per workgroup of
// group_refine_kernel, `count` of them used), to the active list: four threads per region
__global__ __launch_bounds__(kThreads) void compact_survivors_kernel(const uint32_t *__restrict__ surv_slot,
                                                                     const uint32_t *__restrict__ surv_head,
                                                                     const uint32_t *__restrict__ count,
                                                                     const uint32_t *__restrict__ offset,
                                                                     uint32_t regions, uint32_t *__restrict__ new_slot,
                                                                     uint32_t *__restrict__ new_grp) {
    const size_t stride = (size_t)gridDim.x * blockDim.x / 4;
    for (size_t r = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) / 4; r < regions; r += stride) {
        const uint32_t c = count[r], o = offset[r];
        for (uint32_t k = threadIdx.x & 3u; k < c; k += 4) {
            new_slot[o + k] = surv_slot[r * kRefineThreads + k];
            new_grp[o + k] = surv_head[r * kRefineThreads + k];
        }
    }
}

// out[q] = q + 1 where a group starts at slot q (its LCP entry is decided), else 0
__global__ __launch_bounds__(kThreads) void head_flags_kernel(const uint32_t *__restrict__ lcp, uint32_t n,
                                                              uint32_t *__restrict__ out) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x; q < n; q += stride)
        out[q] = lcp[q] < kLcpPendingMin ? (uint32_t)q + 1u : 0u;
}

}  // namespace

// shared tail of every round: sorted view of m active elements -> sa / rank / next active list
template <bool kRound0> void regroup(SaBuild &b, const RegroupIn &in) {
    Context &ctx = b.ctx;
    hipStream_t s = ctx.stream;
    const uint32_t m = b.m, n = b.n;
    uint32_t *d_total = b.d_total;
    const size_t pmark = ctx.arena.mark();
    const size_t tiles = in.seg ? (size_t)in.seg->num_tiles * (kSortTile / kFuseTile) : div_up(m, kFuseTile);
    {
        const double bytes = kRound0 ? 20.0 * m : 28.0 * m;  // view (+ vals) in, (sa +) rank + lcp out (+ survivors)
        ProfScope ps(ctx.profiler(), "sa_regroup", s, bytes);
        // descriptors of both scans, then [ticket, error flag]
        uint64_t *desc = ctx.arena.alloc<uint64_t>(2 * tiles + 1);
        HIP_CHECK(hipMemsetAsync(desc, 0, (2 * tiles + 1) * sizeof(uint64_t), s));
        RegroupArgs A{};
        A.keys = in.keys; A.keys32 = in.keys32; A.seg = in.seg ? *in.seg : SegView{}; A.num_tiles = (uint32_t)tiles;
        A.short_tag = in.short_tag; A.seq_shift = in.seq_shift;
        A.sym_bits = in.sym_bits; A.tag_bits = in.tag_bits; A.bits = in.bits; A.low_bits = in.low_bits;
        A.bits_shift = in.bits == 2 ? 1 : (in.bits == 4 ? 2 : 3);
        A.grp = kRound0 ? nullptr : (in.grp ? in.grp : b.grp()); A.lo = in.lo; A.vals = in.vals; A.act_slot = kRound0 ? nullptr : b.slot(); A.m = m;
        A.sa_is_current = in.sa_is_current ? 1 : 0;
        A.lcp_list = in.lcp_list; A.dbl_h = in.dbl_h;
        A.sa = b.sa; A.lcp = b.lcp;
        A.new_slot = b.next_slot(); A.new_grp = b.next_grp();
        if (in.by_slot) {  // (the rank of every slot is stored only if somebody will read it: SaBuild::store_ranks)
            A.rank_by_slot = b.rank_by_slot; A.store_ranks = b.store_ranks ? 1 : 0;
        } else {
            A.rank_val = b.rank_val; A.chg_idx = b.scratch_idx; A.store_ranks = 1;
            A.Plcp = b.Plcp;  // doubling boundaries read range minima of the LCP values decided so far
        }
        A.chg_count = d_total + 2;
        HIP_CHECK(hipMemsetAsync(d_total + 2, 0, sizeof(uint32_t), s));
        A.desc_max = desc; A.desc_sum = desc + tiles;
        A.packed = n < 0x80000000u ? 1 : 0;  // slots and counts fit 31 bits
        A.ticket = reinterpret_cast<uint32_t *>(desc + 2 * tiles);
        A.d_total = d_total;
        const bool want_phases = sa_knobs().regroup_phases;
        if (want_phases) {
            A.phases = ctx.arena.alloc<unsigned long long>(8);
            HIP_CHECK(hipMemsetAsync(A.phases, 0, 64, s));
        }
        const bool two_bit_buckets = kRound0 && in.keys32 && in.seg && in.low_bits == 0 && in.bits == 2;
        const bool fast_layout = two_bit_buckets && in.tag_bits == KeyLayout<2>::kTagBits &&
                                 in.sym_bits == 2 * KeyLayout<2>::kSyms && in.seq_shift == 0 &&
                                 in.short_tag == (uint32_t)KeyLayout<2>::kSyms;
        const bool rec_layout = two_bit_buckets && in.tag_bits == kRecTagBits && in.sym_bits == 2 * kRecSyms &&
                                in.seq_shift == 32 && in.short_tag == 0;
        const bool p16_layout = two_bit_buckets && in.tag_bits == kP16TagBits && in.sym_bits == 2 * kP16Syms &&
                                in.seq_shift == 0 && in.short_tag == (uint32_t)kP16Syms;
        const bool p35_layout = two_bit_buckets && in.tag_bits == kP35TagBits && in.sym_bits == kP35KeyBits &&
                                in.seq_shift == 0 && in.short_tag == (uint32_t)kP35Syms;
        if (fast_layout)
            regroup_kernel<kRound0, kRound0 ? 1 : 0><<<(unsigned)tiles, kFuseThreads, 0, s>>>(A);  // (layouts only exist for round 0)
        else if (p16_layout)
            regroup_kernel<kRound0, kRound0 ? 3 : 0><<<(unsigned)tiles, kFuseThreads, 0, s>>>(A);
        else if (p35_layout)
            regroup_kernel<kRound0, kRound0 ? 4 : 0><<<(unsigned)tiles, kFuseThreads, 0, s>>>(A);
        else if (rec_layout)
            regroup_kernel<kRound0, kRound0 ? 2 : 0><<<(unsigned)tiles, kFuseThreads, 0, s>>>(A);
        else
            regroup_kernel<kRound0, 0><<<(unsigned)tiles, kFuseThreads, 0, s>>>(A);
        KERNEL_CHECK();
        if (want_phases) {
            unsigned long long h[8];
            HIP_CHECK(hipMemcpyAsync(h, A.phases, 64, hipMemcpyDeviceToHost, s));
            HIP_CHECK(hipStreamSynchronize(s));
            const double wn = h[4] ? (double)h[4] : 1.0;
            fprintf(stderr, "[nolzss] regroup<%d> m=%u tiles=%zu phases (cycles per tile, %llu sampled): ticket %.0f  loads+heads %.0f  look-back %.0f  output %.0f\n",
                    (int)kRound0, m, tiles, h[4], h[0] / wn, h[1] / wn, h[2] / wn, h[3] / wn);
        }
        HIP_CHECK(hipMemcpyAsync(d_total + 1, A.ticket + 1, sizeof(uint32_t), hipMemcpyDeviceToDevice, s));
    }
    ctx.arena.rewind(pmark);
    uint32_t total3[3] = {0, 0, 0};  // survivors, look-back error flag, elements whose rank changed
    ctx.read_back(d_total, total3, 3);
    if (total3[1]) throw HipError("suffix array: look-back scan timed out");
    if (!in.by_slot && total3[2] > 0) {
        // rank[start] = new rank for the elements whose rank changed: the one truly random write of the round
        ProfScope ps(ctx.profiler(), "sa_rank_scatter", s);
        uint32_t *idx[2] = {b.scratch_idx, in.vals};
        uint32_t *val[2] = {b.rank_val, b.scratch_val};
        bucketed_scatter(idx, val, total3[2], b.rank, n, ctx.arena, s, ctx.profiler(), false);
    }
    b.m = total3[0];
    b.a_cur ^= 1;
}
template void regroup<true>(SaBuild &, const RegroupIn &);
template void regroup<false>(SaBuild &, const RegroupIn &);

void compact_survivors(Context &ctx, const uint32_t *surv_slot, const uint32_t *surv_head, const uint32_t *surv_count,
                       uint32_t *surv_off, unsigned g, uint32_t *new_slot, uint32_t *new_grp, uint32_t *d_new_m) {
    hipStream_t s = ctx.stream;
    // the next active list: the regions one after the other (they are in slot order already)
    ProfScope ps(ctx.profiler(), "sa_regroup", s, 16.0 * (double)g);
    scan_exclusive_add_u32(surv_count, surv_off, g, d_new_m, ctx.arena, s);
    compact_survivors_kernel<<<grid_for((size_t)g * 4, kThreads), kThreads, 0, s>>>(
        surv_slot, surv_head, surv_count, surv_off, g, new_slot, new_grp);
    KERNEL_CHECK();
}

// (rank_by_slot is not needed afterwards: it serves as one of the ping-pong buffers)
void write_all_ranks(SaBuild &b) {
    hipStream_t s = b.stream();
    Arena &arena = b.arena();
    ProfScope ps(b.ctx.profiler(), "sa_rank_scatter", s);
    const size_t smark = arena.mark();
    // rank of a slot = slot of its group head + 1, and the heads are the slots whose LCP entry is decided: an
    // inclusive max-scan (the regroup kernels no longer write this array: when the direct rounds finish the
    // suffix array nobody reads it)
    if (!b.store_ranks) {
        head_flags_kernel<<<grid_for(b.n, kThreads), kThreads, 0, s>>>(b.lcp, b.n, b.rank_by_slot);
        KERNEL_CHECK();
        scan_inclusive_max_u32(b.rank_by_slot, b.rank_by_slot, b.n, arena, s);
    }
    uint32_t *idx[2] = {b.sa, arena.alloc<uint32_t>(b.n)};
    uint32_t *val[2] = {b.rank_by_slot, arena.alloc<uint32_t>(b.n)};
    bucketed_scatter(idx, val, b.n, b.rank, b.n, arena, s, b.ctx.profiler(), true, /*keep_val=*/false, b.ctx.rec_plan);
    arena.rewind(smark);
}

// ---- the LCP safety net --------------------------------------------------------------------------------------------------
// KEEP IN THIS FILE.  It would sit as well beside the driver in suffix_array.hip, but regroup_kernel<true, *> compiles
// differently without it: with lcp_finish_kernel (suffix_lcp, text.hpp) gone, regroup_kernel holds the only calls of the
// 64-bit count-leading-zeros routine of the device library in this translation unit, the inliner then takes them earlier
// and the routine's clamp for a zero input is dropped (four instantiations, 64 to 72 bytes shorter each; same registers
// and LDS, same results).  Moving this block is a kernel change and has to be measured as one.
// Every boundary receives its LCP from the regroup of the round in which it appears (or from the kernels of the direct
// rounds and the repeat passes); whatever is still pending when the construction is over is compared in the text.
// finishes the LCP entries that round 0 could not decide: both suffixes share their first
// `skip` symbols, so the packed-word comparison starts there
template <int BITS>
__global__ __launch_bounds__(kThreads) void lcp_finish_kernel(const uint64_t *__restrict__ words, uint32_t n,
                                                              TermTable terms, const uint32_t *__restrict__ sa,
                                                              uint32_t skip, uint32_t *__restrict__ lcp) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t r = (size_t)blockIdx.x * blockDim.x + threadIdx.x; r <= n; r += stride) {
        if (r == n) {
            lcp[r] = 0;
        } else {
            // safety net: every boundary is decided by the keys, the direct round or a doubling
            // step; anything still pending is compared in the packed text
            if (lcp[r] >= kLcpPendingMin) lcp[r] = suffix_lcp<BITS>(words, terms, sa[r - 1], sa[r], skip);
        }
    }
}

uint32_t pending_threshold() { return kLcpPendingMin; }

void inject_pending_for_test(Context &ctx, uint32_t *lcp, uint32_t n) {
    if (sa_knobs().inject_pending && n > 2) HIP_CHECK(hipMemsetAsync(lcp + n / 2, 0xff, sizeof(uint32_t), ctx.stream));
}

// safety net: compare the suffixes in the packed text wherever an LCP entry is still undecided
void finish_pending_lcp(Context &ctx, const PackedText &text, const uint32_t *sa, uint32_t *lcp) {
    const uint32_t n = text.n;
    hipStream_t s = ctx.stream;
    ProfScope ps(ctx.profiler(), "lcp_finish", s);
    const unsigned g = grid_for((size_t)n + 1, kThreads, 256u * 32u);
    const uint32_t skip = 1;  // (all that is known for sure: the suffixes differ somewhere)
    dispatch_bits(text.bits, [&](auto B) {
        lcp_finish_kernel<decltype(B)::value><<<g, kThreads, 0, s>>>(text.words, n, text.terms, sa, skip - 1, lcp);
    });
    KERNEL_CHECK();
}

Pyramid build_lcp_pyramid(Context &ctx, const PackedText &text, const uint32_t *sa, uint32_t *lcp) {
    const uint32_t n = text.n;
    hipStream_t s = ctx.stream;
    uint32_t *flag = ctx.arena.alloc<uint32_t>(1);
    HIP_CHECK(hipMemsetAsync(flag, 0, sizeof(uint32_t), s));
    inject_pending_for_test(ctx, lcp, n);
    const size_t mark = ctx.arena.mark();
    Pyramid P = build_pyramid(lcp, n + 1, false, ctx.arena, s, kLcpPendingMin, flag);
    uint32_t pending = 0;
    ctx.read_back(flag, &pending, 1);
    if (pending) {  // safety net: compare the suffixes in the packed text, then build again
        ctx.arena.rewind(mark);
        finish_pending_lcp(ctx, text, sa, lcp);
        P = build_pyramid(lcp, n + 1, false, ctx.arena, s);
    }
    return P;
}

}  // namespace nolzss
