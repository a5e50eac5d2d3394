// rlz_index.hpp -- the relative-LZ index: the suffix structures of the reference kept resident, target batches matched
// against them by search ("Relative-LZ index: targets matched against a resident reference"; the kernels:
// rlz_index.hip, rlz_locate.hip for pattern queries, rlz_repeats.hip for the maximal repeats of the reference itself
// (its entry points: rlz_index_repeats_api.hip), rlz_seeds.hip for maximal match seeds, rlz_seed_chain.hip for
// their colinear chains, rlz_align.hip for the base-level alignments of those, rlz_pileup.hip for the pileup counts of
// the alignments, rlz_consensus.hip for the insertion alleles and the consensus of a pileup and rlz_cohort.hip for the bit planes of
// many samples and their comparison; the handle and its entry points: rlz_index_api.hip, rlz_index_query_api.hip, rlz_index_seeds_api.hip,
// rlz_pileup_api.hip, rlz_cohort_api.hip).
#pragma once
#include "pipeline.hpp"

namespace nolzss {

constexpr uint32_t kIndexMaxPrefix = 12;  // bases of the prefix table's key: 4^12 + 1 entries = 64 MiB

// The index text X = Rblk s [rc-block s] (rlz_api.hip, rlz_prepare without a target) packed segmented at 2 bits, and
// what a match reads of it.  Every pointer is device memory: arena memory while the index is being built, the handle's
// own allocation afterwards (rlz_index_copy_into).
struct RlzIndexView {
    PackedText text;
    const uint32_t *sa = nullptr;   // |X|
    const uint32_t *lcp = nullptr;  // |X| + 1
    Pyramid Plcp{}, Pmin{}, Pmax{};  // over lcp, min over sa, max over sa (= Pmin without reverse complement)
    // table[w], w in [0, 4^P]: the number of ranks whose suffix has a zero-padded P-base key below w
    const uint32_t *table = nullptr;
    uint32_t P = 0;
    uint32_t B = 0;  // |Rblk|: a suffix below B is a forward occurrence, one above it lies in the mirrored block
    bool with_rc = false;
};

struct IndexRec {
    uint64_t start, length, ref;
};

// One pipeline session over the device-resident X (n bytes): pack, suffix array, LCP array, pyramids, prefix table.
// Everything is left in the arena; the caller owns the mark.
RlzIndexView rlz_index_build(Context &ctx, const uint8_t *d_X, uint32_t n, uint32_t B, bool with_rc, uint32_t P);
// Bytes of one allocation that holds everything the view points to (every array 256-byte aligned and padded, as the
// pyramid queries and the text windows expect), and the copy into such an allocation: returns the rebased view.
size_t rlz_index_footprint(const RlzIndexView &v);
RlzIndexView rlz_index_copy_into(Context &ctx, const RlzIndexView &v, void *d_base);

// Per position p < n of the packed batch (pack_independent_text: the target ends are its terminators): len[p] = the
// longest match of the target suffix at p in X (0: none, and at a separator), rank[p] = a rank whose suffix attains it.
void rlz_index_search(Context &ctx, const RlzIndexView &ix, const PackedText &batch, uint32_t *d_len, uint32_t *d_rank);
// The record of each of the z factor starts fpos[k] (positions of the batch): start = B + 1 + fpos[k].
void rlz_index_records(Context &ctx, const RlzIndexView &ix, const uint32_t *d_fpos, uint32_t z, const uint32_t *d_len,
                       const uint32_t *d_rank, IndexRec *d_out);
// The same look-ups over EVERY position: len[p] |= 1 << 31 where the record of p would be a reverse-complement factor.
void rlz_index_strands(Context &ctx, const RlzIndexView &ix, uint32_t n, uint32_t *d_len, const uint32_t *d_rank);

// ---- pattern count and locate (rlz_locate.hip; DESIGN.md 5, "Relative-LZ index: pattern count and locate") -----------
// The batch is P1 s P2 s .. Pq s packed like a target batch: its terminator table (q + 1 entries) gives every pattern's
// first position and length.
struct LocateHit {  // nolzss_rlz_hit
    uint64_t position;
    uint32_t record, is_rc;
};
// Per pattern j < q: cnt[j] = its occurrences in X on both strands, lo[j] = the first rank of its suffix-array interval,
// rep[j] = cnt[j] where cnt[j] <= cap, else 0 (the hits a locate reports).
void rlz_index_patterns(Context &ctx, const RlzIndexView &ix, const PackedText &batch, uint32_t q, uint32_t cap,
                        uint32_t *d_lo, uint32_t *d_cnt, uint32_t *d_rep);
// off[j] = rep[0] + .. + rep[j - 1] (the caller has made sure the total stays below 2^32)
void rlz_index_hit_offsets(Context &ctx, const uint32_t *d_rep, uint32_t q, uint32_t *d_off);
// The T = sum(rep) hits expanded and sorted by (pattern, position, strand): keys[t] = (j << 33) | (position << 1) |
// is_rc, vals[t] = the 0-based reference record (`records` = their number m).  Arena memory, 24 bytes per hit.
struct LocateSorted {
    const uint64_t *keys = nullptr;
    const uint32_t *vals = nullptr;
};
// The bit offsets of the 8-bit digits the sort of the hits runs, least significant first, for a block of B bases and q
// patterns (host only): at most kLocateMaxPasses, none of them across bit 32 of the key.  Returns their number.
constexpr int kLocateMaxPasses = 8;
int rlz_locate_sort_shifts(uint64_t B, uint64_t q, int *shifts);
LocateSorted rlz_index_hits(Context &ctx, const RlzIndexView &ix, uint32_t records, const PackedText &batch, uint32_t q,
                            const uint32_t *d_off, const uint32_t *d_lo, uint32_t T);
// hits [first, first + count) of the sorted pairs unpacked into records
void rlz_index_hit_records(Context &ctx, const LocateSorted &sorted, size_t first, uint32_t count, LocateHit *d_out);

// ---- maximal match seeds (rlz_seeds.hip; DESIGN.md 5, "Relative-LZ index: maximal match seeds") ----------------------
// After rlz_index_search over a target batch of n positions: the seeds are the positions p with len[p] >= max(min_len, 1)
// and (p == 0 or len[p - 1] <= len[p]).
struct SeedRec {  // nolzss_rlz_seed
    uint64_t target, start, length, count;
};
// flag[p] = 1 at a seed, slot[p] = the seeds in front of p, seeds[0 .. S) = their positions, ascending; *d_total = S
// (device memory).  flag, slot and seeds hold n entries each.
void rlz_index_seed_list(Context &ctx, const uint32_t *d_len, uint32_t n, uint32_t min_len, uint32_t *d_flag,
                         uint32_t *d_slot, uint32_t *d_seeds, uint32_t *d_total);
// Per seed j of [first, first + count): d_first[j] = the first rank of the LCP interval that holds every occurrence of the
// seed on both strands, d_rep[j] = their number where it is <= cap, else 0 (the hits that are reported).  With d_out
// (count entries), the record of seed j -- target, start inside the target, length, occurrences -- goes to d_out[j - first].
void rlz_index_seed_intervals(Context &ctx, const RlzIndexView &ix, const PackedText &batch, const uint32_t *d_seeds,
                              uint32_t first, uint32_t count, uint32_t cap, const uint32_t *d_len, const uint32_t *d_rank,
                              uint32_t *d_first, uint32_t *d_rep, SeedRec *d_out);
// The T = sum(rep) hits of the S seeds expanded and sorted by (seed, position, strand), laid out as rlz_index_hits lays out
// the hits of patterns (the caller has made sure that T stays below 2^32 and S below 2^31).  Arena memory: 4 bytes per
// seed, 24 per hit and the sort's histograms.
LocateSorted rlz_index_seed_hits(Context &ctx, const RlzIndexView &ix, uint32_t records, uint32_t n, const uint32_t *d_seeds,
                                 const uint32_t *d_len, uint32_t S, const uint32_t *d_rep, const uint32_t *d_first,
                                 uint32_t T);

// ---- maximal repeats of the reference (rlz_repeats.hip; DESIGN.md 5, "Relative-LZ index: maximal repeats") -----------
// A reported repeat is one LCP interval of X: its representative is the leftmost rank r in (lo, hi] with lcp[r] = the
// interval's value.  The rules of the reported set: include/nolzss_hip.h, nolzss_rlz_index_repeats.
struct RepeatRec {  // nolzss_rlz_repeat
    uint64_t position, length, count;
    uint32_t record, palindrome;
};
// Stages 1 and 2 over the n = |X| ranks.  d_left (n + 1 entries): the left-context flags, scanned in place -- entry
// r + 1 = D[r], the ranks up to r whose suffix has another base in front of it than its left neighbour's, or none.
// d_flag[r] = 1 iff rank r represents a reported repeat of at least min_len >= 1 bases with at least min_count
// occurrences, d_slot[r] = the flags in front of r (n entries each); *d_total = their number S (device memory).
void rlz_repeat_flags(Context &ctx, const RlzIndexView &ix, uint32_t min_len, uint32_t min_count, uint32_t *d_left,
                      uint32_t *d_flag, uint32_t *d_slot, uint32_t *d_total);
// The S repeats ascending by keys[j] = (position << 32) | length: first[j] = the first rank of the interval, count[j] =
// its members, rep[j] = count[j] where count[j] <= cap, else 0 (the hits that are reported), pal[j] = 1 for a palindrome.
// Arena memory, 37 bytes per repeat and the sort's histograms.
struct RepeatList {
    const uint64_t *keys = nullptr;
    const uint32_t *first = nullptr, *count = nullptr, *rep = nullptr;
    const uint8_t *pal = nullptr;
    uint32_t S = 0;
};
// The bit offsets of the 8-bit digits the sort of the repeats runs, least significant first, for a block of B bases (host
// only): at most kLocateMaxPasses, none of them across bit 32 of the key.  Returns their number.
int rlz_repeat_sort_shifts(uint64_t B, int *shifts);
RepeatList rlz_repeat_list(Context &ctx, const RlzIndexView &ix, uint32_t min_len, uint32_t min_count, uint32_t cap,
                           const uint32_t *d_left, const uint32_t *d_flag, const uint32_t *d_slot, uint32_t S);
// repeats [first, first + count) of the list as records
void rlz_repeat_records(Context &ctx, const RlzIndexView &ix, const RepeatList &list, size_t first, uint32_t count,
                        RepeatRec *d_out);
// The T = sum(rep) hits of the list expanded and sorted by (repeat, position, strand), laid out as rlz_index_hits lays
// out the hits of patterns (the caller has made sure that T stays below 2^32 and S below 2^31).  Arena memory: 4 bytes
// per repeat, 24 per hit and the sort's histograms.
LocateSorted rlz_repeat_hits(Context &ctx, const RlzIndexView &ix, uint32_t records, const RepeatList &list, uint32_t T);

// ---- colinear seed chains (rlz_seed_chain.hip; DESIGN.md 5, "Relative-LZ index: colinear seed chains") ---------------
// An anchor is one reported hit of one seed: q = the seed's start inside its target, y = its coordinate in X (the hit's
// position on the forward strand, the mirrored block's on the reverse strand), len = the seed's length.  The anchors lie
// in group order: keys[i] = (target << 40) | (group << 32) | y ascending, group = is_rc * records + record, equal keys by
// ascending q.  The rules of the recurrence: include/nolzss_hip.h, nolzss_rlz_index_seed_chains.
constexpr uint32_t kChainLookback = 64;      // NOLZSS_RLZ_CHAIN_LOOKBACK: the ring is one wavefront wide
constexpr uint32_t kChainNoPred = 0xffffffffu;
constexpr uint64_t kChainMaxTargets = 1ull << 24;  // the key keeps target, group and y in 24 + 8 + 32 bits
struct ChainAnchors {
    const uint64_t *keys = nullptr;
    const uint32_t *q = nullptr, *len = nullptr;
    uint32_t n = 0;
};
struct ChainRules {
    uint32_t max_gap = 0, bandwidth = 0;  // (clamped to 2^32 - 1: no coordinate difference is larger)
    uint64_t min_score = 0;
    uint32_t records = 0;  // m: a group >= m is a reverse-strand group of record group - m
    uint32_t B = 0;        // x = 2 B - y - len + 1 on the reverse strand
};
struct ChainRec {  // nolzss_rlz_chain
    uint64_t target, t_start, t_end, r_start, r_end, score;
    uint32_t record, is_rc, num_anchors, primary;
};
struct ChainAnchorRec {  // nolzss_rlz_chain_anchor
    uint64_t t_start, position, length;
};
struct ChainsOut {  // arena memory
    uint32_t num_chains = 0, num_anchors = 0;
    const ChainRec *chains = nullptr;          // num_chains, ascending by (target, is_rc, record)
    const uint64_t *offsets = nullptr;         // num_chains + 1
    const ChainAnchorRec *anchors = nullptr;   // num_anchors
    const uint32_t *f = nullptr, *pred = nullptr;  // per anchor, group-local (pred: kChainNoPred without one)
};
// The bit offsets of the 8-bit digits the sort of the anchors runs, least significant first, for y < y_end, `groups`
// groups and k targets (host only): at most kLocateMaxPasses.  Returns their number.
int rlz_chain_sort_shifts(uint64_t y_end, uint64_t groups, uint64_t k, int *shifts);
// *d_total = rep[0] + .. + rep[S - 1], summed in 64 bits (device memory): the hits a seed query would expand
void rlz_index_rep_total(Context &ctx, const uint32_t *d_rep, uint32_t S, uint64_t *d_total);
// The T sorted hits of rlz_index_seed_hits (S seeds over a batch of n positions) as anchors in group order.  Arena
// memory: 40 bytes per hit and the sort's histograms.
ChainAnchors rlz_seed_chain_anchors(Context &ctx, const RlzIndexView &ix, uint32_t records, const PackedText &batch,
                                    const uint32_t *d_seeds, const uint32_t *d_len, uint32_t S, const LocateSorted &sorted,
                                    uint32_t T);
// Group heads, the recurrence, ends, backtrack and primary flags over anchors in group order (a.n >= 1).  Waits for the
// stream twice (the number of groups, then the totals).  Arena memory: at most 152 bytes per anchor.
ChainsOut rlz_seed_chain_run(Context &ctx, const ChainAnchors &a, const ChainRules &rules);

// ---- base-level alignments of the seed chains (rlz_align.hip; DESIGN.md 5, "Relative-LZ index: base-level alignments") -
// One banded edit-distance job per gap between consecutive anchors of a chain and per flank of a chain, by the rules of
// nolzss_rlz_index_align (include/nolzss_hip.h).  A job reads nq query bases from position qpos of the packed query text
// and ny reference bases from position ypos of the packed reference text, upward (gap, right flank) or downward (left
// flank: the job runs on the reversed strings).  Lane l of the job's wavefront is diagonal lo + l, `width` of them.
constexpr uint32_t kAlignLanes = 64;  // NOLZSS_RLZ_ALIGN_LANES: the diagonals of a job are the lanes of one wavefront
constexpr uint32_t kAlignGap = 0, kAlignRight = 1, kAlignLeft = 2;
constexpr uint32_t kAlignNoAnchor = 0xffffffffu;
constexpr uint32_t kAlignI = 1, kAlignD = 2, kAlignEq = 7, kAlignX = 8;  // BAM's codes
constexpr uint64_t kAlignMaxTarget = 1ull << 28;                          // an op keeps its length in 28 bits
struct AlignJob {
    uint32_t kind = kAlignGap;
    uint32_t dp = 0;              // 1: the wavefront runs the recurrence (nq >= 1 and ny >= 1); 0: cost and endj stand below
    uint32_t qpos = 0, ypos = 0;  // the first base read of either text
    uint32_t nq = 0, ny = 0;      // rows and columns of the rectangle (0 and 0: a clipped or empty flank)
    int32_t lo = 0;               // the lowest allowed diagonal j - i
    uint32_t width = 1;           // allowed diagonals, 1 .. 64
    uint32_t anchor = kAlignNoAnchor;  // the chain anchor whose `=` run follows the job's columns (production)
    uint32_t cost = 0, endj = 0;  // of a job without recurrence
    uint32_t pad = 0;
};
// The gap job between two anchors: gq query bases at qpos, gy reference bases at ypos.
__host__ __device__ inline AlignJob align_gap_job(uint32_t qpos, uint32_t gq, uint32_t ypos, uint32_t gy, uint32_t band) {
    AlignJob j;
    const int64_t delta = (int64_t)gy - (int64_t)gq;
    const int64_t lo = (delta < 0 ? delta : 0) - (int64_t)band, hi = (delta > 0 ? delta : 0) + (int64_t)band;
    j.kind = kAlignGap;
    j.qpos = qpos;
    j.ypos = ypos;
    j.nq = gq;
    j.ny = gy;
    j.lo = (int32_t)lo;
    j.width = (uint32_t)(hi - lo + 1);
    j.dp = (gq && gy) ? 1u : 0u;
    j.cost = j.dp ? 0u : gq + gy;
    j.endj = gy;
    return j;
}
// A flank job of fq query bases with `avail` bases of the record span beside it.  Right flank: the texts are read upward
// from qpos / ypos.  Left flank: qend / yend are the anchor's coordinates and the texts are read downward from qend - 1 /
// yend - 1.  A clipped flank (fq == 0, fq > max_flank, or no end cell inside the band) has nq = ny = 0.
__host__ __device__ inline AlignJob align_flank_job(uint32_t kind, uint32_t qat, uint32_t fq, uint32_t yat, uint32_t avail,
                                                    uint32_t band, uint64_t max_flank) {
    AlignJob j;
    j.kind = kind;
    j.lo = -(int32_t)band;
    j.width = 2u * band + 1u;
    if (fq == 0 || (uint64_t)fq > max_flank) return j;
    const uint64_t reach = (uint64_t)fq + band;
    const uint32_t W = (uint64_t)avail < reach ? avail : (uint32_t)reach;
    if ((uint64_t)W + band < (uint64_t)fq) return j;  // no end cell: [max(0, fq - band), min(W, fq + band)] is empty
    j.qpos = kind == kAlignLeft ? qat - 1u : qat;
    j.ypos = kind == kAlignLeft ? yat - 1u : yat;
    j.nq = fq;
    j.ny = W;
    j.dp = W ? 1u : 0u;
    j.cost = j.dp ? 0u : fq;
    j.endj = 0;
    return j;
}
struct AlignRec {  // nolzss_rlz_alignment
    uint64_t target, t_start, t_end, r_start, r_end, score, edit_distance, columns;
    uint32_t record, is_rc, num_ops, primary;
};
// The jobs of a run and everything the stages leave per job.  Arena memory.
struct AlignJobs {
    uint32_t J = 0, A = 0;  // jobs; chain anchors (0 in the debug hook)
    const AlignJob *jobs = nullptr;
    const uint32_t *alen = nullptr;  // L' per chain anchor (production; nullptr in the debug hook)
    uint32_t *rows = nullptr, *slots = nullptr, *weight = nullptr;  // rlz_align_sizes: DP rows, column slots, max columns
    uint64_t total_rows = 0, total_slots = 0, total_weight = 0;      // their sums in 64 bits
    uint32_t *row_off = nullptr, *col_off = nullptr;                 // rlz_align_layout
    unsigned long long *dirs = nullptr;  // 2 words per DP row: bit l of word 0 / 1 = bit 0 / 1 of lane l's direction
    uint8_t *codes = nullptr;            // one code byte per column slot, 0: unused
    uint32_t *cost = nullptr, *endj = nullptr, *ncols = nullptr;  // per job: rlz_align_dp, rlz_align_traceback
};
struct AlignOut {  // arena memory
    uint32_t num_alignments = 0, num_ops = 0;
    const AlignRec *recs = nullptr;       // one per chain, in chain order
    const uint64_t *op_offsets = nullptr; // num_alignments + 1
    const uint32_t *ops = nullptr;        // (length << 4) | code
};
// One lane per chain anchor writes L' and the gap job behind it, the first and last anchor of a chain its flank jobs:
// chain c with anchors [o, o + d) owns the jobs [o + c, o + c + d] -- left flank, d - 1 gaps, right flank.  Arena memory:
// 48 bytes per job, 4 per anchor.
AlignJobs rlz_align_plan(Context &ctx, const RlzIndexView &ix, const PackedText &batch, const ChainsOut &chains, uint32_t band,
                         uint64_t max_flank);
// rows / slots / weight of every job and their 64-bit totals (waits for the stream once).  12 bytes per job.
void rlz_align_sizes(Context &ctx, AlignJobs &a);
// The offsets of the rows and of the column slots, the direction rows, the code bytes (zeroed) and the per-job results.
// The caller has made sure that the three totals stay below 2^32.  Arena memory: 20 bytes per job, 16 per DP row, 1 per
// slot.
void rlz_align_layout(Context &ctx, AlignJobs &a);
// The recurrence, one wavefront per job: qt / xt are the packed query and reference texts.
void rlz_align_dp(Context &ctx, const AlignJobs &a, const PackedText &qt, const PackedText &xt);
// One lane per job walks the direction bits back and writes the job's code bytes and their number.
void rlz_align_traceback(Context &ctx, const AlignJobs &a);
// Heads, scans, ops and one record per chain.  Waits for the stream once (the number of ops).  Arena memory: 16 bytes
// per slot, 12 per op, 88 per chain.
AlignOut rlz_align_ops(Context &ctx, const AlignJobs &a, const ChainsOut &chains, const ChainRules &rules);

// ---- pileup counts of the alignments (rlz_pileup.hip; DESIGN.md 5, "Relative-LZ index: pileup") ---------------------
// The counters of a pileup handle, by the rules of nolzss_rlz_pileup_add (include/nolzss_hip.h): device memory of the
// handle's own, B + 1 entries per array (xbase: 4 per entry), zeroed at open.  `=` runs and reverse-strand spans are
// difference entries in wrapping u32 -- +1 at the first position, -1 just past the last, so entry B takes the -1 of a
// run that ends the block -- and rlz_pileup_resolve scans them into depths: entry p + 1 of an exclusive scan is the
// depth of p.  X, D, I and BREAK are dense counters.
constexpr uint32_t kPileupChannels = 8;  // A, C, G, T, DEL, INS, REV, BREAK
constexpr uint32_t kPileupArrays = 11;   // u32 arrays of B + 1 entries: 36 bytes of counters and 8 of resolved depths
struct PileupView {
    uint32_t *diff_eq = nullptr, *diff_rev = nullptr;    // difference entries of the `=` depth and of REV
    uint32_t *depth_eq = nullptr, *depth_rev = nullptr;  // their exclusive scans (rlz_pileup_resolve)
    uint32_t *xbase = nullptr;                           // [p][base]: X columns by the oriented target base
    uint32_t *del = nullptr, *ins = nullptr, *brk = nullptr;
    uint32_t B = 0;
};
struct PileupVariantRec {  // nolzss_rlz_variant
    uint64_t position, record_offset;
    uint32_t record, ref_base, allele, count, depth, rev;
};
struct PileupRule {  // of a variants query: count >= min_count and count * den >= num * depth, in 64 bits
    uint32_t min_count = 1;
    uint64_t num = 0, den = 1;
};
// The insertion log of a pileup (device memory of the handle's own): one event per I op of a kept alignment -- where INS
// was counted, the op's length and the first kPileupInsBases bases of the allele as two words of big-endian 2-bit codes.
constexpr uint32_t kPileupNormalize = 1u;    // NOLZSS_RLZ_PILEUP_NORMALIZE
constexpr uint32_t kPileupMaxShift = 1024;   // NOLZSS_RLZ_PILEUP_MAX_SHIFT
constexpr uint32_t kPileupInsBases = 64;     // NOLZSS_RLZ_PILEUP_INS_BASES
constexpr uint32_t kPileupStats = 4;         // words of d_stats: alignments kept, their ops, their columns, events logged
struct PileupEvent {
    uint32_t position, length;
    uint64_t bases[2];
};
struct PileupLog {  // what an accumulate appends to: event j of the add goes to events[base + j] iff base + j < capacity
    PileupEvent *events = nullptr;
    uint64_t base = 0, capacity = 0;
    uint32_t flags = 0;
};
// Bytes of one allocation that holds the arrays of a view (each 256-byte aligned), and the view over such an allocation.
size_t rlz_pileup_footprint(uint32_t B);
PileupView rlz_pileup_view(void *d_base, uint32_t B);
// *d_count (device memory, zeroed here) = the I ops of the kept alignments: the events an accumulate of them appends.
// Writes nothing else.
void rlz_pileup_count_insertions(Context &ctx, const AlignOut &a, const PackedText &batch, uint32_t B, bool primary_only,
                                 unsigned long long *d_count);
// The alignments of rlz_align_ops (arena memory) added to the counters and their I ops to the log: `batch` is the packed
// target batch they were aligned from, `block` the packed index text.  With kPileupNormalize in log.flags every D and I
// op behind an `=` op is shifted to its leftmost block position (the rule: nolzss_rlz_pileup_open_flags).  d_stats
// (kPileupStats words, device memory, zeroed here).  Every arena array is taken before the first kernel that writes a
// counter.  Arena memory: 16 bytes per op and the scans' tile sums.  No position outside [r_start, r_end) of an op's
// alignment is written, and no event outside [0, log.capacity).
void rlz_pileup_accumulate(Context &ctx, const PileupView &v, const AlignOut &a, const PackedText &batch,
                           const PackedText &block, bool primary_only, const PileupLog &log, unsigned long long *d_stats);
// depth_eq / depth_rev from diff_eq / diff_rev: two scans over B + 1 entries
void rlz_pileup_resolve(Context &ctx, const PileupView &v);
// The eight channels of positions [start, start + count) of the block into d_out (count x 8), after a resolve: `block`
// is the packed index text, whose terminator table holds the separators (their counters are written as 0).
void rlz_pileup_compose(Context &ctx, const PileupView &v, const PackedText &block, uint32_t start, uint32_t count,
                        uint32_t *d_out);
// d_n[p] = the records (0 .. 5) a variants query writes for position p < B, after a resolve
void rlz_pileup_variant_flags(Context &ctx, const PileupView &v, const PackedText &block, const PileupRule &rule, uint32_t *d_n);
// The records [first, first + count) of the query, d_off = the exclusive scan of d_n, into d_out[0 .. count)
void rlz_pileup_variant_records(Context &ctx, const PileupView &v, const PackedText &block, const PileupRule &rule,
                                const uint32_t *d_off, uint64_t first, uint32_t count, PileupVariantRec *d_out);

// ---- insertion alleles and the consensus (rlz_consensus.hip; DESIGN.md 5, "Relative-LZ index: consensus") ------------
// The allele table of a log: its distinct events ascending by (position, length, bases[0], bases[1]), each with the
// number of events that equal it.
struct PileupAllele {
    uint32_t position, length, count, pad;
    uint64_t bases[2];
};
struct PileupInsertionRec {  // nolzss_rlz_insertion
    uint64_t position, record_offset;
    uint32_t record, length, count, depth, ins_total, truncated;
    uint64_t bases[2];
};
struct ConsensusRule {  // nolzss_rlz_consensus_params
    uint32_t min_depth = 1, low = 0;
    uint64_t num = 0, den = 1;
};
constexpr uint32_t kConsensusStats = 7;  // called, low_positions, substitutions, deleted, insertions, inserted_bases, truncated_skipped
// E >= 1 events -> the table in arena memory (E entries allocated, *count of them written).  Waits for the stream once.
// Arena memory: 56 bytes per event and the sorts' histograms.
const PileupAllele *rlz_pileup_alleles(Context &ctx, const PileupEvent *d_events, uint32_t E, uint32_t *count);
// d_n[g] = 1 where allele g < G passes the rule against the depth of its position, else 0 (after a resolve)
void rlz_pileup_insertion_flags(Context &ctx, const PileupView &v, const PackedText &block, const PileupAllele *d_alleles,
                                uint32_t G, const PileupRule &rule, uint32_t *d_n);
// The records [first, first + count) of the query, d_off = the exclusive scan of d_n, into d_out[0 .. count)
void rlz_pileup_insertion_records(Context &ctx, const PileupView &v, const PackedText &block, const PileupAllele *d_alleles,
                                  uint32_t G, const uint32_t *d_n, const uint32_t *d_off, uint64_t first, uint32_t count,
                                  PileupInsertionRec *d_out);
// d_len[p] = the bytes position p < B emits, d_len[B] = 0; d_stats (kConsensusStats words, zeroed here) summed over
// the positions (after a resolve)
void rlz_consensus_lengths(Context &ctx, const PileupView &v, const PackedText &block, const PileupAllele *d_alleles, uint32_t G,
                           const ConsensusRule &rule, uint32_t *d_len, unsigned long long *d_stats);
// The bytes [first, first + count) of the text, d_off = the exclusive scan of d_len, into d_out[0 .. count)
void rlz_consensus_text(Context &ctx, const PileupView &v, const PackedText &block, const PileupAllele *d_alleles, uint32_t G,
                        const ConsensusRule &rule, const uint32_t *d_off, uint64_t first, uint32_t count, uint8_t *d_out);
// d_out[i] = d_off[first + i] in 64 bits, i < count
void rlz_consensus_starts(Context &ctx, const uint32_t *d_off, uint64_t first, uint32_t count, uint64_t *d_out);
// d_out[r] = the offset in the text where record r < records begins, d_out[records] = total + 1
void rlz_consensus_record_offsets(Context &ctx, const PackedText &block, const uint32_t *d_off, uint32_t B, uint32_t records,
                                  uint64_t total, uint64_t *d_out);

// ---- cohort of samples (rlz_cohort.hip; DESIGN.md 5, "Relative-LZ index: cohort") ----------------------------------
// A sample of a cohort is three bit planes of W = ceil(B / 64) words each, `ok`, `lo`, `hi` in this order (the rules:
// include/nolzss_hip.h, nolzss_rlz_cohort_*): bit p & 63 of word p >> 6 belongs to block position p.  The planes of all
// samples lie sample-major in ONE device allocation of the handle: sample s begins at word 3 W s.  The two invariants
// every reader relies on: lo and hi are 0 wherever ok is 0, and every bit at or beyond B is 0.
constexpr uint32_t kCohortStats = 4;        // words of d_stats: called, low, deleted, differs
constexpr uint32_t kCohortTile = 64;        // samples per side of a pair tile
constexpr uint32_t kCohortMaxSlice = 4096;  // words of a slice at the most: a workgroup counts below 2^18 per pair
constexpr uint64_t kCohortLaunchWordPairs = 1ull << 34;  // the work of one launch of the pair kernel, where a row allows it
struct CohortSiteRec {  // nolzss_rlz_cohort_site
    uint64_t position, record_offset;
    uint32_t record, present, counts[4], reference, pad;
};
inline size_t cohort_words(uint32_t B) { return ((size_t)B + 63) / 64; }
// The planes of one sample (3 W words at d_sample) from the resolved counters of a pileup under the consensus' call
// rule (base_call_of, rlz_pileup_device.hpp); d_stats (kCohortStats words, device memory, zeroed here) summed over the
// positions.  Writes the 3 W words and the statistics, nothing else.
void rlz_cohort_pack_counts(Context &ctx, const PileupView &v, const PackedText &block, const ConsensusRule &rule,
                            uint64_t *d_sample, unsigned long long *d_stats);
// ... from one byte per block position (d_bytes, B of them): ACGT in either case is a call
void rlz_cohort_pack_bytes(Context &ctx, const uint8_t *d_bytes, uint32_t B, const PackedText &block, uint64_t *d_sample,
                           unsigned long long *d_stats);
// The slice length in words a launch of the pair kernel over `row_tiles` tiles of planes of W words takes when no knob
// names one
uint32_t rlz_cohort_default_slice(uint32_t row_tiles, size_t W);
// d_diff / d_cmp (N x N each, zeroed here): the pair counts over all words, both triangles.  slice_knob: the words of a
// slice (clamped to kCohortMaxSlice), 0: rlz_cohort_default_slice per row.  One launch per row of tiles and per
// kCohortLaunchWordPairs of it; a row of more than one slice adds its partial sums by integer atomics.
void rlz_cohort_pairs(Context &ctx, const uint64_t *d_planes, uint32_t N, uint32_t B, uint32_t slice_knob, uint32_t *d_diff,
                      uint32_t *d_cmp);
// d_n[p] = 1 where position p < B is a site of the query, else 0
void rlz_cohort_site_flags(Context &ctx, const uint64_t *d_planes, uint32_t N, uint32_t B, const PackedText &block,
                           uint32_t min_present, bool with_reference, uint32_t *d_n);
// The records [first, first + count) of the query, d_off = the exclusive scan of d_n, into d_out[0 .. count)
void rlz_cohort_site_records(Context &ctx, const uint64_t *d_planes, uint32_t N, uint32_t B, const PackedText &block,
                             const uint32_t *d_n, const uint32_t *d_off, uint64_t first, uint32_t count, CohortSiteRec *d_out);
// Bytes [first, first + count) of the N x S letters (sample-major) at the S positions d_pos, each below B
void rlz_cohort_columns(Context &ctx, const uint64_t *d_planes, uint32_t N, uint32_t B, const uint32_t *d_pos, uint64_t S,
                        uint64_t first, uint32_t count, uint8_t *d_out);
// The letters of positions [start, start + count) of one sample
void rlz_cohort_calls(Context &ctx, const uint64_t *d_sample, uint32_t B, uint32_t start, uint32_t count, uint8_t *d_out);

constexpr int kCrossWords = 4;  // words compared per step of cross_suffix_less (at most 7: the pad words)

// Three-way comparison across two packed 2-bit texts (the counterpart of suffix_compare, text.hpp): the suffix of X at
// `a` against the target suffix at `p` of the batch, which has `rem` symbols before its target's end.  The caller
// guarantees that the first h0 symbols agree.  lcp = the common prefix, capped by the target's end and by the
// terminator of the X suffix.  Returns true if the X suffix is the smaller one: the order of text.hpp, with the end of
// the target as the smallest terminator of all (the target suffix is the smaller one when it ends first or together
// with the X suffix).  At most min(rem, segment rest) / 32 + kCrossWords words are compared.
__device__ __forceinline__ bool cross_suffix_less(const uint64_t *__restrict__ xw, const TermTable &xterms, uint32_t a,
                                                  const uint64_t *__restrict__ tw, uint32_t p, uint32_t rem, uint32_t h0,
                                                  uint32_t &lcp) {
    uint32_t k;
    const uint32_t lx = term_limit(xterms, a, k);
    const uint32_t limit = lx < rem ? lx : rem;
    // kCrossWords words of each text per step: their loads are independent of each other, and a match between similar
    // genomes runs over hundreds of bases (the windows may read up to kCrossWords words past the nearer end: the packed
    // texts carry 8 zero pad words, text_pack.hip)
    uint32_t h = h0;
    while (h < limit) {
        const uint64_t xbit = ((uint64_t)a + h) * 2, ybit = ((uint64_t)p + h) * 2;
        const uint64_t *__restrict__ xp = xw + (xbit >> 6), *__restrict__ yp = tw + (ybit >> 6);
        const int xo = (int)(xbit & 63), yo = (int)(ybit & 63);
        uint64_t xs[kCrossWords + 1], ys[kCrossWords + 1];
#pragma unroll
        for (int j = 0; j <= kCrossWords; ++j) {
            xs[j] = xp[j];
            ys[j] = yp[j];
        }
#pragma unroll
        for (int j = 0; j < kCrossWords; ++j) {
            const uint64_t x = xo ? ((xs[j] << xo) | (xs[j + 1] >> (64 - xo))) : xs[j];
            const uint64_t y = yo ? ((ys[j] << yo) | (ys[j + 1] >> (64 - yo))) : ys[j];
            if (x != y) {
                const uint32_t d = h + 32u * j + (uint32_t)__clzll((long long)(x ^ y)) / 2;
                if (d < limit) {
                    lcp = d;
                    return x < y;
                }
                lcp = limit;  // the first difference lies behind the nearer end
                return lx < rem;
            }
        }
        h += 32u * kCrossWords;
    }
    lcp = limit;
    return lx < rem;
}

}  // namespace nolzss
