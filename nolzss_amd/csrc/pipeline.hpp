// pipeline.hpp -- per-device context and the stage entry points of the factorization pipeline.
#pragma once
#include "code16.hpp"
#include "common.hpp"
#include "pyramid.hpp"
#include "rank_blocks.hpp"
#include "text.hpp"

#include <vector>

namespace nolzss {

struct Context {
    int device = 0;
    hipStream_t stream = nullptr;
    Arena arena;
    Profiler prof;
    uint32_t *h_pinned = nullptr;  // 64 words of pinned host memory for small read-backs
    uint8_t *h_stage = nullptr;    // pinned host staging for uploads (grow-only, merged batch)
    size_t h_stage_cap = 0;
    // merged batch of long records (set for the duration of one run): the two permutation scatters of the
    // pipeline -- rank[sa[r]] and L*[sa[r]] -- stay inside the records (text_order.hpp, RecordScatterPlan)
    const struct RecordScatterPlan *rec_plan = nullptr;
    // length of the last text on which the 16-bit codes had to be given up (build_lstar): calls on a text of that
    // length start with 32-bit codes instead of paying the second run of the stage again
    uint32_t code16_off_n = 0;
    // what the last mark_chain on this context did (chain.hip; nolzss_debug_cursor): one of kCursor*, and the tiles
    // whose walk from the entry did not meet the speculative walk
    uint32_t cursor_path = 0, cursor_failed_tiles = 0;

    Profiler *profiler() { return prof.enabled() ? &prof : nullptr; }
    // copy `count` (<= 64) device words to host and wait for them
    void read_back(const uint32_t *d_src, uint32_t *dst, int count);
};

// ---- stage 1: text packing -------------------------------------------------------------
// Scans the byte text for its alphabet, builds dense codes and packs it (2/4/8 bits/symbol).
// A text of upper-case nucleotides plus at most 250 byte values that occur exactly once each is
// packed SEGMENTED at 2 bits per base, the unique bytes becoming terminators (text.hpp).
PackedText pack_text(Context &ctx, const uint8_t *d_text, size_t n);
// Many INDEPENDENT nucleotide sequences in one text (text.hpp, TermTable::seq_shift): records of
// A/C/G/T with one separator byte at each of the sorted positions.  false if the text holds other bytes.
// mirror: the text is T1 $ .. Tk $ rc(Tk) $ .. rc(T1) $ and segment t belongs with segment 2k - 1 - t.
bool pack_independent_text(Context &ctx, const uint8_t *d_text, size_t n, const std::vector<uint32_t> &separators,
                           PackedText &out, bool mirror = false);

// ---- stages 2+3: suffix array (prefix doubling over radix sorts) and LCP array -------------
// sa[r] = start of the r-th smallest suffix, isa[i] = rank of suffix i PLUS ONE (n u32 each);
// lcp[0] = 0, lcp[r] = lcp(suffix sa[r-1], suffix sa[r]), lcp[n] = 0 (n + 1 u32).  All
// caller-allocated.  LCP entries between suffixes that round 0 already separates come straight
// from the sort keys; only the others compare packed text.  Returns the doubling rounds run.
// isa_deferred (optional): the caller can do without isa[] until the factor-length codes have been brought into
// text order -- if the direct rounds finish the suffix array (no doubling round needs rank[]), isa[] is then NOT
// written here and *isa_deferred = true: the caller hands isa to the permutation of the codes, which delivers it
// as a second value (build_lstar's isa_fill; text_order.hpp, bucketed_scatter with out2).
int build_suffix_array(Context &ctx, const PackedText &text, uint32_t *sa, uint32_t *isa, uint32_t *lcp,
                       bool *isa_deferred = nullptr);
// The range-minimum pyramid over lcp[0..n]; checks on the way that the construction left no boundary
// undecided (and compares those suffixes in the text if it did).
Pyramid build_lcp_pyramid(Context &ctx, const PackedText &text, const uint32_t *sa, uint32_t *lcp);

struct Pyramid;

// ---- stage 4: per-position factor length codes (lpnf.hip) ---------------------------------
// lstar[i] = L*[i] (0 = literal), through a handle (code16.hpp).  Returns the number of positions that needed the exact
// search.  alloc_lstar makes the handle: the 16-bit form (2 n bytes and the wide-code list) if the caller can take it
// (want_narrow: isa is left to this stage and nothing behind it needs 32-bit codes) and the packed text-order
// permutation will run, else n 32-bit codes.  On return lstar.width says which array the cursor reads: 16 (no code
// reached the saturation value) or 32 (lstar.wide: the caller's array, or one this stage took from the arena BEHIND
// its own temporaries -- widened with the list applied, or from a second run when the list overflowed).
// widened_lstar: a 32-bit copy of the 16-bit array in the arena, with the first `listed` list entries applied.
LstarCodes alloc_lstar(Context &ctx, uint32_t n, bool want_narrow);
uint32_t *widened_lstar(Context &ctx, const LstarCodes &codes, uint32_t n, uint32_t listed);
// isa_fill (optional): isa[] has not been written yet (build_suffix_array, isa_deferred): it is filled here.
// fill_pyramids (optional): Psa / Plcp are allocated (alloc_pyramid over sa / lcp) but not computed: the tile kernel
// of this stage writes their first level from the blocks it has in LDS and the upper levels are filled here -- the
// caller skips build_pyramid / build_lcp_pyramid (whose check for undecided LCP entries happens here too).
// blocks (optional, plain mode): alloc_rank_blocks(n) of the caller; the tile kernel of this stage copies SA and LCP
// of its ranks into them (rank_blocks.hpp), on EVERY run of the stage -- the run after the pending-LCP safety net
// (which changes lcp[]) and the run with wide codes write them again, so they equal the final lcp[] on return.
uint32_t build_lstar(Context &ctx, uint32_t n, const uint32_t *sa, const uint32_t *isa, const uint32_t *lcp,
                     const Pyramid &Psa, const Pyramid &Plcp, LstarCodes &lstar, uint32_t *isa_fill = nullptr,
                     const PackedText *fill_pyramids = nullptr, RankBlock *blocks = nullptr);
// The block array of a text of n symbols, in the arena (128-byte aligned): whole tiles of the candidate kernel, so that
// its stores need no bound, and one block behind them for lcp[n] of a text that ends with a tile.  nullptr with
// NOLZSS_NO_RANK_BLOCKS.
RankBlock *alloc_rank_blocks(Context &ctx, uint32_t n);
// pieces of build_lcp_pyramid for that form (sa_regroup.hip): the code above which an LCP entry counts as
// undecided, the comparison of the suffixes around every undecided entry, and the test hook that leaves one undecided
uint32_t pending_threshold();
void finish_pending_lcp(Context &ctx, const PackedText &text, const uint32_t *sa, uint32_t *lcp);
void inject_pending_for_test(Context &ctx, uint32_t *lcp, uint32_t n);

// ---- stage 5: greedy cursor (chain.hip): mark the chain, then take outputs from it ----------------
// THE ARENA RULE of this stage and of the pipeline runners below (run_rc_pipeline*, run_rlz_pipeline, api::run_plain):
// they allocate from ctx.arena and leave what they return there; none of them rewinds below its results.  The caller
// takes arena.mark() before the call and rewinds when it has finished with the outputs -- the caller owns the mark.
//
// mark_chain runs the cursor over the codes from start_pos (start_pos >= n: z = 0, nothing launched) and leaves the
// marked chain: one bit per position and the scanned factor counts of the 4096-position tiles.  It reads the codes and
// nothing else; width 16: the cursor kernels read two bytes per position.  Its own temporaries are released before it
// returns.  A count is mark_chain followed by the caller's rewind.
enum : uint32_t {
    kCursorNone = 0,         // nothing ran (start_pos >= n)
    kCursorSpeculative = 1,  // the speculative walk delivered the mark
    kCursorFailedOver = 2,   // ... raised its flag, and the exact stages ran behind it
    kCursorExact = 3,        // the exact stages alone (NOLZSS_NO_SPEC_CURSOR)
};
struct Chain {
    uint32_t n = 0, z = 0;  // positions, factors
    LstarCodes codes;
    const unsigned long long *bits = nullptr;  // num_tiles x 64 words
    const uint32_t *tile_off = nullptr;        // factors in front of each tile
    uint32_t num_tiles = 0;
};
Chain mark_chain(Context &ctx, uint32_t n, uint32_t start_pos, const LstarCodes &codes);
// The z factor starts, ascending (nullptr for z = 0).  Reads the mark only.
uint32_t *chain_starts(Context &ctx, const Chain &chain);
// What a factor record needs beyond its start and the codes: the interval of the factor around its rank, then the
// leftmost occurrence.  Pmax + rcN (reverse-complement modes): the max pyramid over SA and the N of ref = 2N - max SA
// - L + 1; the codes then carry the strand in bit 31.  rebase (plain mode only, refused together with Pmax): the
// terminator table of a text of independent records; start and ref of every factor leave relative to its record.
// blocks (plain mode without rebase, optional): SA and LCP of every 16 ranks in one line (rank_blocks.hpp); the
// look-ups then read those instead of sa[] / lcp[].
struct RecordLookup {
    const uint32_t *sa = nullptr, *isa = nullptr, *lcp = nullptr;
    Pyramid Psa, Plcp;
    const Pyramid *Pmax = nullptr;
    uint32_t rcN = 0;
    const TermTable *rebase = nullptr;
    const RankBlock *blocks = nullptr;
};
// The z records (start, length, ref as u64) of the factors that begin at `starts` (chain_starts of the same chain).
// 16-bit codes: plain records only.
void *chain_records(Context &ctx, const Chain &chain, const uint32_t *starts, const RecordLookup &lookup);
// Debug hooks (debug_api.hip): the record of EVERY position i < n, i.e. the record output over the starts 0, 1, .., n - 1
// -- the distance to the next start is 1 everywhere, so the kernel takes length and flag from the code of each position.
void *position_factors(Context &ctx, uint32_t n, const LstarCodes &codes, const RecordLookup &lookup);
// Factor lengths without factor records ("Factor-length histograms"): the marked positions and their
// 32-bit codes only.  All device buffers are caller-allocated; hist (with_strand: 2 x T bins, the reverse-complement
// ones behind the forward ones) and *tail_count are zeroed by the caller.
constexpr uint32_t kLengthHistBins = 2048;  // T: dense bins for 1 <= L < T
struct ChainLengthsOut {
    uint32_t *hist = nullptr;        // per-length counts, or nullptr for no histogram
    uint64_t *tail = nullptr;        // lengths >= T: length | strand << 32, in no particular order
    uint32_t *tail_count = nullptr;  // entries written to tail
    uint32_t tail_cap = 0;           // floor(n / T) + 1: the lengths sum to at most n
    uint32_t **order = nullptr;      // optional: z lengths in factor order, left in the arena
};
inline uint32_t length_tail_cap(uint32_t n) { return n / kLengthHistBins + 1u; }
// with_strand: bit 31 of a code is the reverse-complement flag and selects the second half of hist
void chain_lengths(Context &ctx, const Chain &chain, const ChainLengthsOut &out, bool with_strand);

// What the caller of a pipeline runner wants from stage 5, and what the runner left in the arena for it.
struct ChainRequest {
    bool records = false, starts = false;      // wanted: factor records / factor starts
    const ChainLengthsOut *lengths = nullptr;  // wanted: factor lengths
    uint32_t z = 0;                            // result: the factor count, always
    void *d_records = nullptr;                 // result: z x (start, length, ref), if records
    uint32_t *d_starts = nullptr;              // result: z ascending starts, if records or starts
    bool leaves_output() const { return records || starts || (lengths && lengths->order); }
};
// The end of every runner: the marked chain's outputs as the request asks for them.
void chain_outputs(Context &ctx, const Chain &chain, const RecordLookup &lookup, bool with_strand, ChainRequest &rq);

// ---- reverse-complement mode (rc.hip): whole pipeline over the prepared string S -------------
struct RcPlainOut;
struct RcDebugOut;
// rq: ChainRequest above, over the reverse-complement chain
void run_rc_pipeline(Context &ctx, const uint8_t *d_S, size_t m, size_t start_pos, ChainRequest &rq,
                     RcPlainOut *plain = nullptr, RcDebugOut *dbg = nullptr);
// plain-mode counts as a by-product of a reverse-complement run: the plain L* of every position i < N comes out of
// the same candidate kernels (rc.hip) and is chained on its own; z = nolzss_count_factors of the original strand(s),
// fpos (want_fpos) = its factor starts in the arena, for the per-record split of a merged run
struct RcPlainOut {
    bool want_fpos = false;
    uint32_t z = 0;
    uint32_t *fpos = nullptr;
};
// Debug-out of a reverse-complement run (tests; debug_api.hip, in the spirit of api::DebugOut): HOST pointers, each may
// be null.  The arrays are copied out behind the far and exact kernels, before their queues are released; N = m / 2 - 1.
struct RcDebugOut {
    uint32_t *sa = nullptr;     // m
    uint32_t *lcp = nullptr;    // m + 1
    uint32_t *isa = nullptr;    // N entries, rank + 1 as on the device (the compact permutation fills no more)
    uint32_t *code = nullptr;   // N: length in bits 0..30, bit 31 = reverse complement, 0 = literal
    uint32_t *plain = nullptr;  // N: the plain-mode by-product; only in a run with RcPlainOut
    void *records = nullptr;    // N x (start, length, ref) as u64: position_factors over the codes
    // what the host read back on the way
    uint32_t far_ranks = 0;         // far queue behind the tile kernel
    uint32_t exact_from_tiles = 0;  // exact-search queue in front of rc_far_kernel
    uint32_t exact_total = 0;       // ... and behind it
    uint32_t compact = 0;           // the tile kernel wrote the compact output
    uint32_t pending_relaunch = 0;  // an undecided LCP entry sent the tile kernel round a second time
};
// the same over a text that has already been packed (merged batch); plain (optional): the plain-mode by-product above
void run_rc_pipeline_packed(Context &ctx, const PackedText &text, size_t start_pos, ChainRequest &rq,
                            RcPlainOut *plain = nullptr, RcDebugOut *dbg = nullptr);
// d_S (2n + 2 bytes) = T' sep revcomp(T') sep for the n bytes d_T = upper-case records with separator bytes
// between them; bytes that are not nucleotides (the separators) are copied to their mirror position.
void prepare_batch_rc_on_device(Context &ctx, const uint8_t *d_T, uint32_t n, uint8_t separator, uint8_t *d_S);
// d_S (2n + 2 bytes) = prepared string of the single sequence d_T; returns the index of the first
// invalid nucleotide or 0xffffffff.
uint32_t prepare_single_rc_on_device(Context &ctx, const uint8_t *d_T, uint32_t n, uint8_t *d_S);

// ---- relative LZ (rlz.hip): every target against the reference block only -----------------------
// The prepared string S = Rblk s T1 s .. Tk s [pad] rc-block s (rlz_api.hip builds it).  Without reverse complement S
// ends behind the sentinel of Tk, rc_block_start = total and rcN = 0.
struct RlzLayout {
    uint32_t total = 0;           // |S|
    uint32_t block_length = 0;    // B = |Rblk|; the chain starts at B + 1
    uint32_t rc_block_start = 0;  // E
    uint32_t chain_end = 0;       // position of the sentinel behind Tk
    uint32_t rcN = 0;             // (B - 1 + E) / 2
    bool with_rc = false;
};
// by_rank[r] = the code (length, bit 31 = reverse complement, 0 = no match) of the suffix of rank r against the
// suffixes that start below B (forward) or at E and beyond (reverse complement); m ranks, lcp as build_suffix_array
// leaves it once build_lcp_pyramid has decided every entry.  E is not read without with_rc.
void rlz_candidates(Context &ctx, const uint32_t *sa, const uint32_t *lcp, uint32_t m, uint32_t B, uint32_t E, bool with_rc,
                    uint32_t *by_rank);
// The whole pipeline over the device-resident S; rq: ChainRequest above (the sentinels between the targets come out as
// literals).  h_codes (optional, host): the code of every position below chain_end.
void run_rlz_pipeline(Context &ctx, const uint8_t *d_S, const RlzLayout &lay, ChainRequest &rq, uint32_t *h_codes = nullptr);
// counts[j] = entries of the ascending list d_fpos inside [bounds[2j], bounds[2j + 1]) (all device pointers)
void rlz_count_per_target(Context &ctx, const uint32_t *d_fpos, uint32_t z, const uint32_t *d_bounds, uint32_t k,
                          uint32_t *d_counts);

}  // namespace nolzss
