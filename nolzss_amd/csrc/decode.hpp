// decode.hpp -- factors and literals back to text on the device (decode.hip; DESIGN.md 5, "Decoding: factors and
// literals back to text"; C ABI: decode_api.hip, include/nolzss_hip.h, nolzss_decode / nolzss_roundtrip).
#pragma once
#include "factor_records.hpp"

namespace nolzss {

// rule of include/nolzss_hip.h that a refused input breaks
enum DecodeRule : uint32_t {
    kDecodeOk = 0,
    kDecodeTiling = 1,
    kDecodeLiteralLength = 2,
    kDecodeSourceRange = 3,
    kDecodeLiteralCount = 4,
    kDecodeComplement = 5,
    // the relative-LZ archive only (rlz_archive.hpp)
    kDecodeSourceInBlock = 6,
    kDecodeTargetBoundary = 7,
};

struct DecodeRefusal : std::invalid_argument {
    DecodeRule rule;
    uint64_t record;    // first offending record (kDecodeComplement: unknown here, see position)
    uint64_t position;  // kDecodeComplement: the first output position whose chain complements a non-nucleotide
    DecodeRefusal(DecodeRule r, uint64_t rec, uint64_t pos, const std::string &msg)
        : std::invalid_argument(msg), rule(r), record(rec), position(pos) {}
};

struct DecodeStats {
    uint64_t n_literals = 0;          // literal records found
    uint64_t resolved_at_expand = 0;  // of the n - prefix_len decoded positions
    uint64_t rounds = 0;
    uint64_t max_active = 0;
};

// All pointers are device memory.  d_out: n bytes whose first prefix_len hold the prefix; [prefix_len, n) is written.
// The records are checked first (DecodeRefusal, nothing launched behind the check); n = start + length of the last
// record, n <= kMaxText and z >= 1 are the caller's to establish.  Work arrays come from the arena and are released on
// return; tile_skip = false launches every jump round over every tile (A/B measurements).
DecodeStats decode_on_device(Context &ctx, const Rec *d_recs, size_t z, const uint8_t *d_literals, size_t n_literals,
                             uint8_t *d_out, size_t prefix_len, size_t n, bool tile_skip = true);
// arena bytes decode_on_device takes for z records and n - prefix_len decoded positions
size_t decode_arena_bytes(size_t z, size_t decoded);

// d_literals[j] = d_text[start of the j-th literal record], for the records of a pipeline run (every start inside
// d_text); d_literals holds z bytes, enough for any z records.  Returns the number of literal records.
size_t gather_literals(Context &ctx, const Rec *d_recs, size_t z, const uint8_t *d_text, uint8_t *d_literals);

// positions i < n with a[i] != b[i], and the smallest one (~0ull if none)
void count_mismatches(Context &ctx, const uint8_t *d_a, const uint8_t *d_b, size_t n, uint64_t *count, uint64_t *first);

}  // namespace nolzss
