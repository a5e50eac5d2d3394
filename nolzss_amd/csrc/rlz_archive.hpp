// rlz_archive.hpp -- the relative-LZ archive on the device: the check of the records at open, the resident form and its
// position sample, the range extraction (rlz_archive.hip; DESIGN.md 5, "Relative-LZ archive: ranges from resident
// records"; C ABI: rlz_archive_api.hip, include/nolzss_hip.h, nolzss_rlz_archive_*).
#pragma once
#include "decode.hpp"
#include "rlz_index.hpp"

namespace nolzss {

// Resident form of one record, 16 bytes, read with one 16-byte load.  Positions are relative to the end of the block
// ("decoded" coordinates, below 2^32 as n <= kMaxText).
struct ArchiveRec {
    uint32_t start;   // first decoded position of the record
    uint32_t length;
    uint32_t src;     // block position of the source of byte 0: ref (forward), ref + length - 1 (reverse complement)
    uint32_t meta;    // bits 1..0: kind; bits 15..8: the symbol of a literal
};
enum : uint32_t { kArchiveForward = 0, kArchiveRc = 1, kArchiveLiteral = 2 };
constexpr uint32_t kSampleShift = 8;  // one sample per 256 decoded positions

inline size_t archive_samples(size_t decoded) { return (decoded + ((size_t(1) << kSampleShift) - 1)) >> kSampleShift; }

struct ArchiveCheck {
    uint64_t bad = ~0ull;   // (record index << 3 | DecodeRule) of the first offending record, ~0: none
    uint64_t literals = 0;  // literal records
};

// All pointers are device memory; temporaries come from the arena and are released on return.
// d_bounds: k + 1 ascending positions, bounds[0] = block_len, bounds[j + 1] = bounds[j] + length of target j.
// Rules: tiling and literal length as the decoder, source inside the block, target boundary.  lit_flags[k] = 1 for a
// literal record (z words).
ArchiveCheck archive_check(Context &ctx, const Rec *d_recs, size_t z, uint64_t block_len, uint64_t n,
                           const uint64_t *d_bounds, size_t k, uint32_t *lit_flags);
// Checked records -> the resident form and the position sample (archive_samples(n - block_len) words: the index of the
// record that covers decoded position 256 * s).  lit_flags is overwritten with its exclusive scan.
void archive_pack(Context &ctx, const Rec *d_recs, size_t z, uint64_t block_len, uint64_t n, uint32_t *lit_flags,
                  const uint8_t *d_literals, ArchiveRec *d_packed, uint32_t *d_sample);

struct ArchiveView {
    const uint8_t *block;
    const ArchiveRec *recs;
    const uint32_t *sample;
    uint32_t z, samples;
};
// q ranges, total >= 1 output bytes.  d_offsets: q + 1 prefix sums of the range lengths (d_offsets[q] = total);
// d_first[i]: the decoded position of the first byte of range i; every range lies inside [0, decoded).  d_err: one
// word preset to ~0, receives the smallest (range index << 32 | byte of the range) whose reverse-complement copy reads a
// byte that is not a nucleotide.  One launch on ctx.stream; does not wait.
void archive_extract(Context &ctx, const ArchiveView &v, const uint32_t *d_offsets, const uint32_t *d_first, uint32_t q,
                     uint32_t total, uint8_t *d_out, unsigned long long *d_err);

// the record that covers decoded position p (p below the decoded length)
__device__ __forceinline__ uint32_t archive_find_record(const ArchiveView &v, uint32_t p) {
    const uint32_t s = p >> kSampleShift;
    uint32_t lo = v.sample[s];
    // the record that covers the next sample position starts behind 256 * s, at p or before it or behind it; every
    // record behind that one starts behind p
    uint32_t hi = s + 1 < v.samples ? v.sample[s + 1] + 1u : v.z;
    while (hi - lo > 1) {  // hi - lo <= 257
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (v.recs[mid].start <= p) lo = mid;
        else hi = mid;
    }
    return lo;
}

__device__ __forceinline__ ArchiveRec archive_load_record(const ArchiveView &v, uint32_t k) {
    const uint4 w = reinterpret_cast<const uint4 *>(v.recs)[k];
    return ArchiveRec{w.x, w.y, w.z, w.w};
}

const char *archive_rule_text(uint32_t rule);

// ---- batches appended from the index, and the way back to host records ("Relative-LZ archive: batches
// appended from the index") ------------------------------------------------------------------------------------------
// Rblk, bytes [0, B) of the segmented 2-bit index text x: A/C/G/T from the codes, 0x01 at each terminator below B.
void archive_unpack_block(Context &ctx, const PackedText &x, uint32_t B, uint8_t *d_block);

// One batch T1 s T2 s .. Tk s (n bytes, upper case, in device memory) behind z_old records and decoded_old bytes.
struct AppendBatch {
    const uint8_t *text;
    const uint32_t *seps;  // k ascending separator positions (device)
    uint32_t n, k;
    uint32_t z_old, decoded_old;
    uint32_t z_new;        // z_old + (factor starts of the batch) - k: no record is written at or behind it
};
// cnt look-ups of the batch's factor starts d_fpos[0 .. cnt) (batch positions; global start index `first` + t) -> their
// resident records at d_recs[z_old + first + t - j], j = the separators below the position; a separator's own literal
// is dropped.  `base` = B + 1, the absolute position of batch position 0.  d_lit_counts: archive_append_counts(cnt)
// words, all written; their sum is the number of literal records among those the launch wrote.
size_t archive_append_counts(size_t cnt);
void archive_append_records(Context &ctx, const IndexRec *d_chunk, const uint32_t *d_fpos, uint32_t first, uint32_t cnt,
                            uint64_t base, const AppendBatch &b, ArchiveRec *d_recs, uint32_t *d_lit_counts);
// sample[s] for s in [s_lo, s_hi): the last record of [z_old, z_new) with start <= 256 s (256 s >= start[z_old])
void archive_extend_sample(Context &ctx, const ArchiveRec *d_recs, uint32_t z_old, uint32_t z_new, uint32_t s_lo,
                           uint32_t s_hi, uint32_t *d_sample);
// d_index[t] = the literal records among d_recs[0 .. t), t < cnt (cnt words); returns the literals among all cnt.
// Waits for the stream.  (Export lays the literal stream out with it.)
uint64_t archive_literal_index(Context &ctx, const ArchiveRec *d_recs, size_t cnt, uint32_t *d_index);
// Resident records [first, first + cnt) -> 24-byte records at d_out[0 .. cnt) (start absolute, ref with kRcMask, a
// literal has ref == start) and the symbols of their literals at d_literals[d_index[first + t]].
void archive_export_records(Context &ctx, const ArchiveRec *d_recs, size_t first, size_t cnt, uint64_t block_len,
                            const uint32_t *d_index, Rec *d_out, uint8_t *d_literals);

}  // namespace nolzss
