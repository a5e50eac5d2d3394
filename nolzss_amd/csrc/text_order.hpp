// text_order.hpp -- the permutation into text order: (position, value) pairs in list order written to out[position],
// by partition passes of the radix sort and windows assembled in LDS (text_order.hip).  Its callers are the stages
// that bring ranks and factor-length codes from suffix-array order into text order: lpnf.hip, rc.hip, sa_regroup.hip
// and, with a RecordScatterPlan, batch.hip.
#pragma once
#include "code16.hpp"
#include "radix_sort.hpp"

#include <vector>

namespace nolzss {

// out[idx[k]] = val[k] for k < count, idx[k] < n_out (entries with idx >= n_out are dropped).
// A random 4-byte scatter over an array much larger than the caches costs a read-modify-write
// of a whole line per element at HBM.  For large targets the pairs are therefore first
// partitioned by the top 8 bits of idx (one radix pass, coalesced), then written bucket by
// bucket so that all writes in flight fall into a window of n_out/256 entries that L2 /
// Infinity Cache can merge into full lines (a permutation of the whole target is assembled
// window by window in LDS instead).  idx[0]/val[0] hold the input, idx[1]/val[1] are scratch of
// the same size.  With keep_input the input arrays survive (a third pair of buffers is taken
// from the arena); otherwise they are used as scratch too.  The pointer arrays may be updated.
// keep_val = false (with keep_input): only idx[0] survives, val[0] is used as a ping-pong buffer too.
//
// plan (optional): the target is a text of independent RECORDS and the pairs are (position, value) in suffix-
// array order of such a text -- a block-diagonal permutation: the ranks of a record hold the positions of that
// record (record_scatter_plan).  Then ONE segmented radix pass (the record is the bucket, the digit the window
// inside the record) and the window scatter do it, 28 instead of 48 bytes per pair; idx[0] / val[0] survive,
// idx[1] / val[1] are the only scratch.
struct RecordScatterPlan {
    SegView seg;                    // the base positions of every record as one bucket (ranks = positions)
    const uint32_t *win = nullptr;  // per window: first list element, first target element, elements
    uint32_t num_windows = 0;
    const uint32_t *sep = nullptr;  // per separator: its rank (the first of its record) and its position
    uint32_t num_seps = 0;
    uint32_t n = 0;
    int window_bits = 0;
};
// What bucketed_scatter / permute_packed did with a call (filled on the host only; no kernel knows of it).
enum class TextOrderForm : int {
    kNone = 0,          // nothing ran (count == 0), or nothing usable was written (narrow, and the packed form did not finish)
    kPlain,             // plain_scatter_kernel alone (out2: plain_rank_scatter_kernel beside it)
    kPartialThenPlain,  // one or two partition passes by the bits above a 2^19 window, then the plain scatter
    kWindowPerm,        // one value: partition passes and the windows assembled in LDS
    kTwoValueHist,      // two values in one 64-bit word, passes with histograms
    kPacked,            // two values and the low index bits in one word, look-back passes (packed_text_order)
    kRecordPlan,        // RecordScatterPlan: one segmented pass, the record windows, the separators; one value
    kRecordPlan2,       // ... two values
    kPermutePlain,      // permute_packed: plain_packed_scatter_kernel
    kPermuteWindows,    // permute_packed: two passes and the windows
};
struct TextOrderReport {
    TextOrderForm form = TextOrderForm::kNone;  // the form whose result stands
    bool packed_tried = false;                  // packed_text_order ran (its result stands only with form == kPacked)
    uint32_t escaped = 0;                       // codes at or above the escape threshold (may exceed the list's capacity)
    bool list_overflow = false;                 // ... did exceed it
    bool lookback_gave_up = false;              // a look-back of either pass gave up
    int partition_passes = 0;                   // kPartialThenPlain: 1 or 2
    int nbits = 0, wb = 0;                      // index_bits(n_out) and the window bits of the permutation forms
};
// out2 (optional): a second target, out2[idx[k]] = k + 1 -- for the pairs (sa[r], code[r]) of the pipeline that is
// the inverse suffix array in its 1-based form, delivered by the same permutation.  val[1] must then hold
// 2 * count words (the pairs travel with 64-bit values).  A permutation of up to 2^30 targets then goes without
// histograms, each pair in ONE 8-byte word whose code field holds 72 - 2 * nb bits (21 at nb = 25, where the windows keep 2^10 entries); larger codes take an
// exception list (and, should it overflow, the histogram form runs after all).  short_codes = false keeps the
// histogram form: codes that are mostly large (a flag in bit 31) would only overflow the list.
// narrow (optional, with out2; out is then not used): the values are factor-length codes and leave in their 16-bit form
// (code16.hpp), which only the packed form writes -- false, with nothing usable written, when that form does not take
// this permutation (packed_text_order_applies) or gave up.  Without narrow the result is always true.
// report (optional, for the test hook nolzss_debug_text_order): what the chooser did.
bool bucketed_scatter(uint32_t *idx[2], uint32_t *val[2], size_t count, uint32_t *out, uint32_t n_out,
                      Arena &arena, hipStream_t stream, Profiler *prof, bool keep_input, bool keep_val = true,
                      const RecordScatterPlan *plan = nullptr, uint32_t *out2 = nullptr, bool short_codes = true,
                      const LstarCodes *narrow = nullptr, TextOrderReport *report = nullptr);
// does bucketed_scatter take the packed form for a two-value permutation of `count` targets?
bool packed_text_order_applies(size_t count, bool has_plan);
// The same permutation for pairs that already carry both values in one 64-bit word (low half -> out, high half ->
// out2) and are a permutation of [0, count): out[idx[k]] = (uint32_t)packed[k], out2[idx[k]] = packed[k] >> 32.
// Both inputs are overwritten (they serve as buffers of the later passes).
void permute_packed(uint32_t *idx, uint64_t *packed, size_t count, uint32_t *out, uint32_t *out2, Arena &arena,
                    hipStream_t stream, Profiler *prof, TextOrderReport *report = nullptr);
// The plan for a text of n symbols whose records end at h_terms[k] (separator positions, the last entry = n);
// false when the shape does not allow it (a record longer than 2^22 bases, or too many short ones).  The
// tables live in the arena (not released here).
bool record_scatter_plan(const std::vector<uint32_t> &h_terms, uint32_t n, Arena &arena, hipStream_t stream,
                         RecordScatterPlan &plan);

}  // namespace nolzss
