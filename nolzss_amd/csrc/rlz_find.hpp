// rlz_find.hpp -- locate through the parse of a relative-LZ archive: the source table of the records, the kernel text K
// around the record starts, and the two kinds of occurrences of a pattern in the targets -- secondary ones, carried from
// a block occurrence through every copy record whose source covers it, and primary ones, found in K (rlz_find.hip;
// DESIGN.md 5, "Relative-LZ archive: locate through the parse"; the handle and its entry points: rlz_find_api.hip,
// include/nolzss_hip.h, nolzss_rlz_finder_*).
#pragma once
#include "rlz_archive.hpp"

namespace nolzss {

// What a query reads of a finder besides the two indexes.  Every pointer is device memory of the handle's own, 256-byte
// aligned and padded as the pyramid queries expect.
struct FinderView {
    // the source table: the z records ordered by the block position lo of their source interval [lo, hi), stable by
    // record index; a literal has lo = 0 and hi = 0, so nothing ever covers it
    const uint32_t *lo = nullptr, *hi = nullptr, *rec = nullptr;
    Pyramid Phi{};  // max pyramid over hi[]
    // the intervals of K: interval i holds decoded positions [dstart[i], dstart[i] + kstart[i + 1] - kstart[i]) at
    // K[kstart[i] ..); nI + 1 entries each, kstart[nI] = |K|, dstart[nI] = the decoded length
    const uint32_t *kstart = nullptr, *dstart = nullptr;
    const uint32_t *bases = nullptr;  // k + 1: the decoded position of each target, then the decoded length
    uint32_t z = 0, nI = 0, k = 0;
};

// ---- open ------------------------------------------------------------------------------------------------------------
// The windows [max(tb, b - W), min(te, b + W)) of the record starts b, merged into intervals that never span two targets.
// d_kstart and d_dstart: z + 1 words each, of which nI + 1 are written.  Returns nI; *K_len = kstart[nI].  Waits for the
// stream.  Temporaries come from the arena and are released on return.
uint32_t find_intervals(Context &ctx, const ArchiveView &v, const uint32_t *d_bases, uint32_t k, uint32_t W,
                        uint32_t *d_kstart, uint32_t *d_dstart, uint32_t *K_len);
// X = K s0 [rc(K) s1] in d_X (K_len + 1, with_rc: 2 K_len + 2 bytes): K through archive_extract over the intervals, the
// mirror from K.  Throws if a reverse-complement copy of the archive read a byte that is not a nucleotide.
void find_kernel_text(Context &ctx, const ArchiveView &v, const uint32_t *d_kstart, const uint32_t *d_dstart, uint32_t nI,
                      uint32_t K_len, bool with_rc, uint8_t s0, uint8_t s1, uint8_t *d_X);
// The source table in arena memory: lo, hi, rec (z words each, ordered) and the max pyramid over hi.
struct SourceTable {
    uint32_t *lo = nullptr, *hi = nullptr, *rec = nullptr;
    Pyramid Phi{};
};
SourceTable find_source_table(Context &ctx, const ArchiveView &v, uint32_t block_len);

// ---- query -----------------------------------------------------------------------------------------------------------
// hits: keys (j << 33) | (position << 1) | strand of the T occurrences of the batch's patterns in the block (secondary
// walk) or in K (primary filter), as rlz_index_hits lays them out; tpos: the terminator table of the packed batch.
// Count pass: cnt[t] = the records whose source covers block hit t (the decoded occurrences it is carried to).
void find_secondary_count(Context &ctx, const FinderView &f, const uint64_t *d_hits, uint32_t T, const uint32_t *d_tpos,
                          uint32_t *d_cnt);
// cnt[t] = 1 where kernel hit t is a primary occurrence of the collection, else 0
void find_primary_count(Context &ctx, const FinderView &f, const ArchiveView &v, const uint64_t *d_hits, uint32_t T,
                        const uint32_t *d_tpos, uint32_t *d_cnt);
// out[i] = in[0] + .. + in[i - 1] in 64 bits, i in [0, n]: n + 1 entries
void find_scan_u64(Context &ctx, const uint32_t *d_in, uint32_t n, uint64_t *d_out);
// counts[j] = the occurrences of pattern j of both classes, from the scans of the two count passes and the offsets of the
// patterns' hits (q + 1 entries each)
void find_pattern_counts(Context &ctx, const uint64_t *d_scanS, const uint32_t *d_offS, const uint64_t *d_scanP,
                         const uint32_t *d_offP, uint32_t q, uint64_t *d_counts);
// Emit passes: the occurrences of the patterns that are reported (out_off[j + 1] > out_off[j]; q + 1 entries) as keys
// (j << 33) | (decoded position << 1) | is_rc with value = the primary flag, pattern j at [out_off[j], out_off[j + 1]):
// its secondary occurrences first, in the order of the block hits, then its primary ones.
struct FindEmit {
    const uint64_t *scanS, *scanP;  // the scans of the count passes (T + 1 entries each)
    const uint32_t *offS, *offP;    // the offsets of the patterns' block hits and kernel hits (q + 1 entries each)
    const uint32_t *out_off;        // q + 1
    uint64_t *keys;
    uint32_t *vals;
    uint32_t total;                 // out_off[q]: no store goes to or behind it
};
void find_secondary_emit(Context &ctx, const FinderView &f, const ArchiveView &v, const uint64_t *d_hits, uint32_t T,
                         const uint32_t *d_tpos, const FindEmit &e);
void find_primary_emit(Context &ctx, const FinderView &f, const ArchiveView &v, const uint64_t *d_hits, uint32_t T,
                       const uint32_t *d_tpos, const FindEmit &e);

struct TargetHit {  // nolzss_rlz_target_hit
    uint64_t target, position;
    uint32_t is_rc, primary;
};
// sorted pairs [0, count) -> records: the target of a decoded position and the position inside it from bases[]
void find_hit_records(Context &ctx, const FinderView &f, const uint64_t *d_keys, const uint32_t *d_vals, uint32_t count,
                      TargetHit *d_out);

}  // namespace nolzss
