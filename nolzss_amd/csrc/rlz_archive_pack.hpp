// rlz_archive_pack.hpp -- the compact container of a relative-LZ archive on the device: resident records -> control
// nibbles, data bytes, 2-bit literals and a 2-bit block, and the way back with every rule of the format checked
// (rlz_archive_pack.hip; DESIGN.md 5, "Relative-LZ archive: the compact container"; the format and the C ABI:
// include/nolzss_hip.h, nolzss_rlz_archive_pack / _open_packed; rlz_archive_pack_api.hip).
#pragma once
#include "rlz_archive.hpp"

namespace nolzss {

// What an unpack refuses.  Error words hold (index << 4 | rule), the smallest wins (one 64-bit atomicMin).
enum PackRule : uint32_t {
    kPackOk = 0,
    kPackSpareNibble = 1,    // the unused high nibble of an odd z is not 0 (index z)
    kPackLiteralNibble = 2,  // a literal nibble with b != 0
    kPackLength = 3,         // L == 0
    kPackDiagonalCode = 4,   // v beyond 33 bits
    kPackSourceInBlock = 5,  // x + L > B
    kPackTargetBoundary = 6, // a record straddles the end of a target or lies behind the last one
    kPackLiteralCount = 7,   // more literal records than n_literals (index z: fewer)
    kPackDataSize = 8,       // the nibbles ask for another number of data bytes than the section holds (index z)
    kPackSeparatorList = 9,  // a separator position at or beyond B, or not above the one before (index: in the list)
};
const char *packed_rule_text(uint32_t rule);

inline size_t packed_quarter(size_t n) { return (n + 3) / 4; }  // bytes of n symbols at 2 bits

// ---- pack: all pointers are device memory, temporaries come from the arena and STAY there (the caller rewinds) ------
struct PackPlan {
    uint32_t *rank;       // z: the copies among records [0, i)
    uint2 *diag;          // (g, r) of each copy, by rank (room for z)
    uint32_t *offset;     // z: the first data byte of record i
    uint64_t data_bytes;  // exact in 64 bits: the caller refuses 2^32 or more before anything is written
};
// copies = z - n_literals.  Waits for the stream (the byte total comes back).
PackPlan packed_plan(Context &ctx, const ArchiveRec *d_recs, size_t z, uint32_t B, size_t copies);
// d_control: (z + 1) / 2 bytes, d_data: plan.data_bytes; every byte of both is written by exactly one lane
void packed_write(Context &ctx, const ArchiveRec *d_recs, size_t z, const PackPlan &plan, uint8_t *d_control, uint8_t *d_data);
// The literal symbols in record order at d_raw (n_literals bytes) and four to a byte at d_two (packed_quarter bytes);
// returns 1 when every one is A, C, G or T (d_two is then the section, else d_raw).  Waits for the stream.
uint32_t packed_literals(Context &ctx, const ArchiveRec *d_recs, size_t z, size_t n_literals, uint8_t *d_raw, uint8_t *d_two);
// The block at 2 bits at d_two (packed_quarter(B) bytes, 0x01 as base 0) and the ascending positions of its 0x01 bytes
// at *d_seps (arena, *num_seps words); returns 1 for mode 1, 0 when a byte is none of A, C, G, T, 0x01 (nothing else
// is then meaningful: the section is the raw block).  Waits for the stream.
uint32_t packed_block(Context &ctx, const uint8_t *d_block, size_t B, uint8_t *d_two, uint32_t **d_seps, uint32_t *num_seps);

// ---- unpack ---------------------------------------------------------------------------------------------------------
// The block section -> B bytes at d_block.  mode 1: d_section holds packed_quarter(B) bytes and then num_seps
// little-endian 32-bit positions (at any alignment).  Returns ~0 or (list index << 4 | kPackSeparatorList).  Waits.
uint64_t unpack_block(Context &ctx, const uint8_t *d_section, size_t B, uint32_t num_seps, uint8_t *d_block);
struct UnpackIn {
    const uint8_t *control, *data, *literals;  // (z + 1) / 2, data_bytes, packed_quarter(n_literals) or n_literals bytes
    uint64_t data_bytes, n_literals;
    uint32_t literal_mode, B;
    const uint64_t *bounds;  // k + 1 ascending decoded positions, bounds[0] = 0; saturated at ~0
    uint32_t k;
};
struct UnpackOut {
    uint64_t bad = ~0ull;  // (index << 4 | PackRule) of the smallest offending record, ~0: none
    uint64_t copies = 0;   // copy records
    uint64_t covered = 0;  // sum of the lengths (meaningful when bad == ~0: no wrap-around then)
};
// Control, data and literal streams -> z resident records at d_recs.  Every read of a section is bounded by its size;
// the data size is compared with what the nibbles ask for before a data byte is read.  Waits for the stream.
UnpackOut unpack_records(Context &ctx, const UnpackIn &in, size_t z, ArchiveRec *d_recs);

// ---- shared with the container of the factor records of the other modes (factor_pack.hip) ---------------------------
// *d_out (one 64-bit word in device memory) = the sum of d_in[0 .. n), exact in 64 bits, on the stream
void packed_sum_u32(Context &ctx, const uint32_t *d_in, size_t n, unsigned long long *d_out);
// n symbols <-> packed_quarter(n) bytes at 2 bits (A, C, G, T = 0 .. 3, anything else packs as 0); n == 0 launches nothing
void packed_quarter_pack(Context &ctx, const uint8_t *d_in, size_t n, uint8_t *d_out);
void packed_quarter_unpack(Context &ctx, const uint8_t *d_in, size_t n, uint8_t *d_out);

}  // namespace nolzss
