// factor_pack.hpp -- the compact container of the factor records of every mode but relative LZ, on the device: 24-byte
// (start, length, ref) records -> control nibbles, data bytes and 2-bit literals, and the way back with every rule of
// the format checked (factor_pack.hip; DESIGN.md 5, "Factor records: the compact container"; the format and the C ABI:
// include/nolzss_hip.h, nolzss_factors_pack / nolzss_factorize_packed / nolzss_factors_unpack / nolzss_decode_packed;
// factor_pack_api.hip).
#pragma once
#include "decode.hpp"

namespace nolzss {

// What a pack or an unpack refuses.  Error words hold (index << 4 | rule), the smallest wins (one 64-bit atomicMin).
enum FactorPackRule : uint32_t {
    kFacOk = 0,
    // the records a pack is given, in nolzss_decode's words
    kFacTiling = 1,          // start[k + 1] != start[k] + length[k], length == 0, or an end beyond the pipeline
    kFacLiteralLength = 2,   // a literal (ref == start) whose length is not 1
    kFacSourceRange = 3,     // pack: ref + length > start; unpack: the recovered x + L > p
    // the sections an unpack is given
    kFacSpareNibble = 4,     // the unused high nibble of an odd z is not 0 (index z)
    kFacLiteralNibble = 5,   // a literal nibble with b != 0
    kFacLength = 6,          // L == 0
    kFacDiagonalCode = 7,    // v beyond 33 bits
    kFacLiteralCount = 8,    // more literal records than n_literals (index z: fewer)
    kFacDataSize = 9,        // the nibbles ask for another number of data bytes than the section holds (index z)
    kFacDecoded = 10,        // the lengths do not sum to `decoded` (index z)
};
const char *factor_pack_rule_text(uint32_t rule);

inline size_t factor_quarter(size_t n) { return (n + 3) / 4; }  // bytes of n symbols at 2 bits

// ---- pack: all pointers are device memory, temporaries come from the arena and STAY there (the caller rewinds) ------
// The rules of the format over z host-made records (those of a pipeline run need no check): tiling from start[0],
// length >= 1, every end at or below `limit`, literal length, source range.  Returns ~0 or (index << 4 | rule) of the
// smallest offending record.  Waits for the stream.
uint64_t factor_check_records(Context &ctx, const Rec *d_recs, size_t z, uint64_t limit);
struct FactorPackPlan {
    uint32_t *rank;       // z: the copies among records [0, i)
    uint2 *diag;          // (g, r) of each copy, by rank (room for z)
    uint32_t *offset;     // z: the first data byte of record i
    uint64_t data_bytes;  // exact in 64 bits: the caller refuses 2^32 or more before anything is written
    uint64_t copies;      // copy records
};
// Waits for the stream (the byte total and the copy count come back).  z >= 1.
FactorPackPlan factor_pack_plan(Context &ctx, const Rec *d_recs, size_t z);
// d_control: (z + 1) / 2 bytes, d_data: plan.data_bytes; every byte of both is written by exactly one lane
void factor_pack_write(Context &ctx, const Rec *d_recs, size_t z, const FactorPackPlan &plan, uint8_t *d_control, uint8_t *d_data);
// n_literals symbols at d_raw -> four to a byte at d_two (factor_quarter bytes); returns 1 when every one is A, C, G or
// T (d_two is then the section, else d_raw).  Waits for the stream.
uint32_t factor_pack_literals(Context &ctx, const uint8_t *d_raw, size_t n_literals, uint8_t *d_two);

// ---- unpack ---------------------------------------------------------------------------------------------------------
struct FactorUnpackIn {
    const uint8_t *control, *data;  // (z + 1) / 2 and data_bytes bytes
    uint64_t data_bytes, n_literals, decoded;
    uint32_t first_start;
};
struct FactorUnpackOut {
    uint64_t bad = ~0ull;  // (index << 4 | FactorPackRule) of the smallest offending record, ~0: none
    uint64_t copies = 0;   // copy records
    uint64_t covered = 0;  // the exact sum of the lengths (set once the data bytes have been read)
};
// Control and data streams -> z records at d_recs.  Every read of a section is bounded by its size; the data size is
// compared with what the nibbles ask for before a data byte is read, the sum of the lengths with `decoded` before a
// position is formed.  first_start + decoded <= kMaxText is the caller's to establish.  Waits for the stream.  z >= 1.
FactorUnpackOut factor_unpack_records(Context &ctx, const FactorUnpackIn &in, size_t z, Rec *d_recs);

}  // namespace nolzss
