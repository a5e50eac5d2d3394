// sa_internal.hpp -- what the translation units of the suffix-array construction share: text_pack.hip, sa_regroup.hip,
// sa_direct.hip, sa_repeats.hip and the driver, suffix_array.hip.  Kernels stay with the file that launches them; only
// constants, the state of one construction (SaBuild) and host functions cross files.  The public entry points are in
// pipeline.hpp.
#pragma once
#include "pipeline.hpp"
#include "radix_sort.hpp"
#include "text_order.hpp"

#include <type_traits>

namespace nolzss {

constexpr int kThreads = 256;

inline unsigned grid_for(size_t work_items, int per_block, unsigned cap = 256u * 16u) {
    size_t g = div_up(work_items, (size_t)per_block);
    if (g < 1) g = 1;
    return (unsigned)(g > cap ? cap : g);
}

struct OpMinU32x {
    __device__ __forceinline__ uint32_t operator()(uint32_t a, uint32_t b) const { return a < b ? a : b; }
};

// *p = min(*p, v) for a value that millions of wavefronts report and that soon stops changing: look
// first, the atomic only if it would lower the value (5 M atomics on one address cost 20 ms)
__device__ __forceinline__ void lower_min(uint32_t *p, uint32_t v) {
    if (*reinterpret_cast<volatile uint32_t *>(p) > v) atomicMin(p, v);
}

// LCP code while the suffix array is being built: the boundary has not appeared yet (values
// >= kLcpPendingMin act as +infinity in range minima).
constexpr uint32_t kLcpPending = 0xffffffffu;
constexpr uint32_t kLcpPendingMin = kLcpPending - 64u;
constexpr uint32_t kLcpPendingCompared = kLcpPending - 1u;  // pending, inside a class the direct round has compared

constexpr uint32_t kSmallGroup = 64;      // largest group the direct round and small_sort_kernel take
constexpr int kRefineTile = 192;          // group_refine_kernel (sa_direct.hip): list positions per workgroup ...
constexpr int kRefineThreads = kRefineTile + (int)kSmallGroup;  // ... and one thread per possible member
constexpr int kRefineWords = 4;           // 64-bit words of text a member fetches per round (the packed text is padded for it)
constexpr uint32_t kRunGroupMax = 16;     // largest group of the pair-run pass (sa_repeats.hip)
constexpr uint32_t kPerVerifyMax = 4096;  // longest period whose groups are checked against the text (sa_repeats.hip)

// the symbol width as a compile-time constant: f(std::integral_constant<int, 2 | 4 | 8>)
template <class F> inline void dispatch_bits(int bits, F &&f) {
    switch (bits) {
    case 2: f(std::integral_constant<int, 2>{}); break;
    case 4: f(std::integral_constant<int, 4>{}); break;
    default: f(std::integral_constant<int, 8>{}); break;
    }
}

// ---- knobs: every NOLZSS_* environment variable of the construction, read once at first use ------------------------
// (ALL of them are frozen by the first reader, whichever file it is in -- on some paths inject_pending_for_test, called
// from lpnf.hip and rc.hip: a variable set in the process after its first factorization is not seen.  The tests and
// tools set them on child processes only.  The knobs of the sorts and of the text-order permutation, NOLZSS_REC_BUCKET_MIN
// among them: SortKnobs, radix_sort.hpp.)
struct SaKnobs {
    SaKnobs();
    bool trace;               // NOLZSS_TRACE: active-list sizes to stderr
    uint32_t dna_fast_min;    // NOLZSS_DNA_FAST_MIN: smallest text that takes the bucketed sort; the tests lower it
    bool no_key16;            // NOLZSS_NO_KEY16: A/B switch back to the 40-bit key [17 bases][6-bit tag]
    bool no_defer;            // NOLZSS_NO_DEFER_ISA: A/B switch, rank[] is scattered although the direct rounds finish
    bool fused_sort;          // NOLZSS_FUSED_SORT: the 16-base key sort on fused 64-bit records, radix_sort.hip -- A/B switch
    bool regroup_phases;      // NOLZSS_REGROUP_PHASES: (diagnostics) cycles per phase of regroup_kernel
    uint32_t refine_words;    // NOLZSS_REFINE_WORDS: cap of the direct round, at most 32 words (1024 bases of DNA) deep;
                              // longer ties are cheaper in the doubling rounds
    bool refine_phases;       // NOLZSS_REFINE_PHASES: (diagnostics) cycles per phase of group_refine_kernel
    bool group_sort_phases;   // NOLZSS_GROUP_SORT_PHASES: (diagnostics) cycles per phase of the group_sort_kernel launches
    bool no_stragglers;       // NOLZSS_NO_STRAGGLERS: (A/B switch)
    bool no_direct2;          // NOLZSS_NO_DIRECT2: A/B switch, no second direct round (and no equalising round)
    uint32_t direct2_div;     // NOLZSS_DIRECT2_MAX: largest share of the text, 1 / this, that takes the second direct round --
                              // a text with more ties than that is repetitive, and the other passes are made for those
    bool no_equalise;         // NOLZSS_NO_EQUALISE: (A/B switch)
    long long pivot_min;      // NOLZSS_PIVOT_MIN: the tests and the fuzzer send every text with that many tied suffixes
                              // through the pivot rounds (-1: not set)
    bool no_pivot;            // NOLZSS_NO_PIVOT: A/B switch
    uint32_t pivot_depth;     // NOLZSS_PIVOT_DEPTH: cap of the first pivot pass, in symbols of 2-bit DNA
    int pivot_passes;         // NOLZSS_PIVOT_PASSES: at most this many pivot passes
    long long pair_runs_min;  // NOLZSS_PAIR_RUNS_MIN: smallest number of tied suffixes for which the pair-run pass runs,
                              // the tests set 1 (-1: not set)
    bool no_periodic;         // NOLZSS_NO_PERIODIC: switches the periodic pass off
    uint32_t runs_avg4;       // NOLZSS_PAIR_RUNS_AVG4: 4 x the largest mean group size that takes the pair-run passes
    bool no_mid_sort;         // NOLZSS_NO_MID_SORT: (A/B switch)
    bool no_seg_large;        // NOLZSS_NO_SEG_LARGE: A/B switch back to the global sort of 12-byte (group, key) records
    bool inject_pending;      // NOLZSS_TEST_INJECT_PENDING: (test hook) one LCP entry is made pending so that the safety net runs
};
const SaKnobs &sa_knobs();

// ---- round 0: one plan for the key sort and the regroup behind it ---------------------------------------------------
struct KeyPlan {
    // fused / key16 / key35 / dna_fast / rec_fast name their sort in radix_sort.hpp; the other three take the general sort
    enum Choice { kFused, kKey16, kKey35, kDnaFast, kRecFast, kIndependent, kSegmented, kGeneral } choice = kGeneral;
    int seq_bits = 0;                            // independent sequences: bits of the sequence number above the key
    int key_bits = 0, key_passes = 0;            // populated low bits of the key, radix passes over them
    int cur = 0;                                 // the buffer the sorted keys end in (the suffixes end in sa)
    int k_syms = 0, tag_bits = 0, low_bits = 0;  // [k_syms symbols][tag][low bits]
    bool bucketed = false;                       // 32-bit stored keys, the top of the key implied by the bucket (SegView)
    uint32_t short_tag = 0, seq_shift = 0;       // RegroupIn
    bool rec_fast() const { return choice == kRecFast; }
    bool independent() const { return choice == kRecFast || choice == kIndependent; }
};

// ---- the state of one construction ------------------------------------------------------------------------------------
struct SaBuild {
    Context &ctx;
    const PackedText &text;
    const uint32_t n;
    uint32_t *const sa, *const rank, *const lcp;
    // the two active lists (slot, head slot of its group) of the suffixes still tied: a phase reads list a_cur and
    // writes the other one
    uint32_t *act_slot[2] = {nullptr, nullptr}, *act_grp[2] = {nullptr, nullptr};
    int a_cur = 0;
    uint32_t *rank_by_slot = nullptr;  // rank of every slot until rank[] exists (write_all_ranks), then a work array
    uint32_t *d_total = nullptr;       // device: survivors, look-back error flag, elements whose rank changed, periodic hint
    uint32_t m = 0;                    // suffixes still tied
    uint64_t h = 0;                    // symbols every tied group agrees on
    bool store_ranks = true, can_defer = false;
    bool independent = false;
    // what the direct round reports (0xffffffff: none)
    uint32_t depth_compared = 0xffffffffu, depth_untouched = 0xffffffffu;
    uint64_t untouched_members = 0;  // (an estimate)
    // ---- the rounds behind write_all_ranks ----
    bool pair_runs = false;  // the passes of sa_repeats.hip may run: the work arrays hold n entries, not m
    size_t wlen = 0;
    uint32_t *tmp_a = nullptr, *tmp_b = nullptr, *tmp_c = nullptr, *rank_val = nullptr, *scratch_idx = nullptr;
    uint32_t *scratch_val = nullptr, *lo = nullptr, *out_lo = nullptr, *out_vals = nullptr;
    uint32_t *d_large = nullptr;  // four counters (count_large_groups, periodic_pass)
    // in_large = members beyond the first kRunGroupMax of their group, large_members = members of groups with more
    // than kRunGroupMax members
    uint32_t in_large = 0, large_members = 0, tied_groups = 0, near_members = 0;
    Pyramid Plcp{};  // range minima over the LCP values known so far; the regroup kernel keeps it current
    size_t pyr_mark = 0;
    uint32_t per_hint = 0;  // periodic pass: a longer period waits for this depth
    int per_attempts = 0;
    int half_passes = 0, shifts[8] = {}, npasses = 0;  // radix passes over (group head, rank) pairs

    hipStream_t stream() const { return ctx.stream; }
    Arena &arena() const { return ctx.arena; }
    const uint32_t *slot() const { return act_slot[a_cur]; }
    const uint32_t *grp() const { return act_grp[a_cur]; }
    uint32_t *next_slot() const { return act_slot[a_cur ^ 1]; }
    uint32_t *next_grp() const { return act_grp[a_cur ^ 1]; }
};

// ---- sa_regroup.hip -------------------------------------------------------------------------------------------------------
// The shared tail of every round: the sorted view of the b.m active elements -> sa / rank / lcp and the next active
// list.  Sets b.m and makes the list it wrote the current one.
struct RegroupIn {
    // round 0: the sorted keys -- or (bucketed) their stored 32-bit words and the buckets -- and the key layout
    const uint64_t *keys = nullptr;
    const uint32_t *keys32 = nullptr;
    const SegView *seg = nullptr;
    int sym_bits = 0, tag_bits = 0, bits = 0, low_bits = 0;
    uint32_t short_tag = 0;  // elements whose length tag is below this are groups of their own
    uint32_t seq_shift = 0;  // independent sequences: key bits from here up = number of the sequence
    // later rounds: per list element the sorted secondary key (the group is b.grp()), its suffix, the LCP a direct
    // comparison decided; h of a doubling step
    const uint32_t *grp = nullptr;  // (only where the sort moved elements across the list: default b.grp())
    const uint32_t *lo = nullptr;
    uint32_t *vals = nullptr;
    const uint32_t *lcp_list = nullptr;
    uint32_t dbl_h = 0;
    bool sa_is_current = false;  // the producer has already written the new order into sa
    // ranks: rank_by_slot in the rounds before rank[] exists (true), afterwards the changed ranks are scattered into rank[]
    bool by_slot = false;
};
template <bool kRound0> void regroup(SaBuild &b, const RegroupIn &in);
// the survivors of the direct round (group_refine_kernel: one region per workgroup, g of them) become the next active
// list new_slot / new_grp, *d_new_m (device) entries; surv_off[g] is work space, the scan's temporaries come from ctx.arena
void compact_survivors(Context &ctx, const uint32_t *surv_slot, const uint32_t *surv_head, const uint32_t *surv_count,
                       uint32_t *surv_off, unsigned g, uint32_t *new_slot, uint32_t *new_grp, uint32_t *d_new_m);
// one pass writes rank[] for everybody: rank[sa[slot]] = rank_by_slot[slot]
void write_all_ranks(SaBuild &b);

// ---- sa_direct.hip --------------------------------------------------------------------------------------------------------
void direct_round(SaBuild &b, int k_syms);
// The launches of the first direct round over the active list slot[m] / grp[m] (m >= 1): group_refine_kernel -- its only
// launch site -- and the compaction of what it leaves tied, on ctx.stream.  The members of a group agree on h0 symbols; at
// most `cap` symbols are inspected (h0 < cap).  timed: the instantiation with the phase clocks, reported to stderr.
// Out: the new order in sa, the boundaries that appeared (and the compared-pending code) in lcp, rank_by_slot (optional)
// for every listed member, the next active list new_slot / new_grp (room for m), *d_new_m, and d_min_depth[3]: [0] the
// depth of the compared classes left tied, [1] h0 if a group was not touched (0xffffffff: none), [2] the untouched members
// counted in every 64th workgroup.  All of them device memory; the work arrays come from ctx.arena: the caller owns the
// mark.  Shared by direct_round and the test hook nolzss_debug_direct_round.
void direct_round_launch(Context &ctx, const PackedText &text, const uint32_t *slot, const uint32_t *grp, uint32_t m, uint32_t *sa,
                         uint32_t *lcp, uint32_t *rank_by_slot, uint32_t h0, uint32_t cap, bool no_stragglers, bool timed,
                         uint32_t *new_slot, uint32_t *new_grp, uint32_t *d_new_m, uint32_t *d_min_depth);
void group_sort_passes(SaBuild &b);
// The rounds of one group-sort pass (group_sort.hpp) over the active list slot[m] / grp[m], without the regroup behind
// them: group_dir_kernel and the four group_sort_kernel launches, window rounds or (pivot) pivot rounds depth_cap symbols
// deep, on ctx.stream.  The members of a group agree on h0 symbols; lcp_mark (optional, the equalising round): only the
// groups whose boundary lcp_mark[g + 1] still holds the plain pending code are taken.  Out: the new order of every taken
// group in sa, out_lo[m], lcp_list[m] and *d_min_depth (0xffffffff: nothing stays tied below a known depth).  The queues
// come from ctx.arena: the caller owns the mark.  Shared by group_sort_pass and the test hook nolzss_debug_group_sort.
constexpr uint32_t kGroupSortRounds = 24;  // rounds before a group gives up (each: kScanWords words + one window)
void group_sort_rounds(Context &ctx, const PackedText &text, const uint32_t *slot, const uint32_t *grp, uint32_t m, uint32_t *sa,
                       uint32_t h0, bool pivot, uint32_t max_rounds, uint32_t depth_cap, const uint32_t *lcp_mark,
                       uint32_t *out_lo, uint32_t *lcp_list, uint32_t *d_min_depth);

// ---- sa_repeats.hip -------------------------------------------------------------------------------------------------------
// out[0] = members beyond the first `limit` of their group, [1] = groups with more than `limit` members, [2] = groups,
// [3] = members next to a member of their group at most kPerVerifyMax symbols away (per_count_large_kernel)
void count_large_groups(SaBuild &b, uint32_t limit, uint32_t *d_cnt, uint32_t out[4]);
bool periodic_pass(SaBuild &b);
// one pair-run pass over the whole text (b.pair_runs, b.m > 0): the sweep, the active list without the suffixes it
// finished and the pyramid over the LCP values it decided.  false: no progress, another pass is not worth it.
bool pair_run_pass(SaBuild &b);
void pair_run_passes(SaBuild &b);

// ---- suffix_array.hip -----------------------------------------------------------------------------------------------------
// What the rounds behind write_all_ranks start from: the work arrays, the counts of count_large_groups, the LCP pyramid
// and the radix shifts.  Shared by the driver and the test hook nolzss_debug_repeat_pass (force_pair_runs: b.pair_runs
// and work arrays of n entries for every m > 0, whatever the knobs say).
void set_up_late_rounds(SaBuild &b, bool force_pair_runs = false);

}  // namespace nolzss
