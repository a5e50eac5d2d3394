// radix_sort.hpp -- LSD radix sort of (u64 or u32 key, u32 value) pairs, 8-bit digits: the bucketed view of segmented
// passes (SegView), the sorts of radix_sort.hip and their knobs.  (One pass and its kernels: radix_pass.hpp, internal;
// the permutation into text order, built on the same pass: text_order.hpp.)
#pragma once
#include "common.hpp"
#include "text.hpp"

#include <vector>

namespace nolzss {

constexpr int kRadixBits = 8;
// elements per tile of the radix kernels: 16 per thread, 256 or 512 threads.  8192 doubles the length of the 256
// bin runs a tile writes (32 elements = one full 128-byte line per array on average instead of half a line).
#ifndef NOLZSS_SORT_TILE
#define NOLZSS_SORT_TILE 4096
#endif
constexpr int kSortTile = NOLZSS_SORT_TILE;
static_assert(kSortTile == 4096 || kSortTile == 8192, "16 keys per thread on 256 or 512 threads");

// A sorted-by-bucket view of an array for SEGMENTED passes: 256 buckets (the values of a leading
// digit that an earlier pass partitioned by), each cut into tiles that never straddle a bucket.
// desc holds kSegDescWords words per tile (device memory): first element, element count, bucket,
// index of (bin 0, tile) in the bin-major histogram table, distance between the tile's bins there,
// first / end element of the bucket, nearest non-empty bucket below / above.
constexpr int kSegDescWords = 12;
struct SegView {
    const uint32_t *desc = nullptr;
    uint32_t num_tiles = 0;
};

struct TileExtent {
    size_t first;      // first element
    uint32_t count;    // elements (<= kSortTile)
    uint32_t bucket;   // 0 without segmentation
    size_t hist0;      // index of (bin 0, this tile) in the bin-major histogram table
    uint32_t hstride;  // distance between the bins of this tile in that table
    uint32_t bkt_first, bkt_end, prev_ne, next_ne;  // (segmented only)
    uint32_t aux;      // (segmented only) one word per bucket for the source of the pass
};

// tile -> elements; without a SegView tiles are the consecutive kSortTile-element blocks of [0, n)
__device__ __forceinline__ TileExtent tile_extent(uint32_t tile, size_t n, uint32_t num_tiles, const SegView &seg) {
    TileExtent e;
    if (seg.desc == nullptr) {
        e.first = (size_t)tile * kSortTile;
        e.count = (uint32_t)((n - e.first < (size_t)kSortTile) ? (n - e.first) : (size_t)kSortTile);
        e.bucket = 0;
        e.hist0 = tile;
        e.hstride = num_tiles;
        e.bkt_first = 0;
        e.bkt_end = (uint32_t)n;
        e.prev_ne = e.next_ne = 0;
        e.aux = 0;
        return e;
    }
    const uint4 *d = reinterpret_cast<const uint4 *>(seg.desc + (size_t)tile * kSegDescWords);  // uniform: scalar loads
    const uint4 a = d[0], b = d[1], c = d[2];
    e.first = a.x;
    e.count = a.y;
    e.bucket = a.z;
    e.hist0 = a.w;
    e.hstride = b.x;
    e.bkt_first = b.y;
    e.bkt_end = b.z;
    e.prev_ne = b.w;
    e.next_ne = c.x;
    e.aux = c.y;
    return e;
}

// ---- knobs: every NOLZSS_* environment variable of radix_sort.hip, local_sort.hpp and text_order.hip, read once at
// first use and frozen (as SaKnobs, sa_internal.hpp; the tests and tools set them on child processes only)
struct SortKnobs {
    SortKnobs();
    bool trace;                // NOLZSS_TRACE: what the text-order permutation did, to stderr
    bool scatter_phases;       // NOLZSS_SCATTER_PHASES: (diagnostics) cycles per phase of rs_scatter_kernel, large array passes
    bool no_local_sort;        // NOLZSS_NO_LOCAL_SORT: A/B switch, segmented passes instead of local_sort_kernel
    bool local_sort_min_set;   // NOLZSS_LOCAL_SORT_MIN: smallest text / average record whose sub-buckets are sorted in LDS;
    size_t local_sort_min;     // not set: the two defaults below
    static constexpr size_t kLocalSortMinText = size_t(1) << 28;
    static constexpr size_t kLocalSortMinRecord = size_t(1) << 20;
    size_t local_min(size_t dflt) const { return local_sort_min_set ? local_sort_min : dflt; }
    bool no_local_regroup;     // NOLZSS_NO_LOCAL_REGROUP: A/B switch, local_sort_kernel without the regroup of round 0 on the way
    size_t local_regroup_min;  // NOLZSS_LOCAL_REGROUP_MIN: smallest text that takes the regroup on the way
    bool no_key35;             // NOLZSS_NO_KEY35: A/B switch, the 16-base key where the 35-bit key would be taken
    bool test_local_order_fails;     // NOLZSS_TEST_LOCAL_ORDER_FAILS: (test hook) the redo path of a failed lane-order check
    bool test_local_lookback_fails;  // NOLZSS_TEST_LOCAL_LOOKBACK_FAILS: (test hook) the look-back's flag is up before the kernel starts
    uint64_t rec_bucket_min;   // NOLZSS_REC_BUCKET_MIN: smallest average record for the record sort and scatter plan (tiles cost 4096 / that)
    bool text_order_hist;      // NOLZSS_TEXT_ORDER_HIST: A/B switch (and tests), the two-value permutation with histograms
    long long text_order_esc;  // NOLZSS_TEXT_ORDER_ESC: (tests) lower escape threshold of the packed form (-1: not set)
    bool no_code16;            // NOLZSS_NO_CODE16: A/B switch, 32-bit codes in text order throughout (code16.hpp)
    uint32_t code16_max;       // NOLZSS_CODE16_MAX: (tests) lower saturation value of the 16-bit codes, 1 .. 0xffff
};
const SortKnobs &sort_knobs();

// Sorts n pairs by the key digits at the given bit offsets (least significant first;
// each digit is kRadixBits wide).  keys[0]/vals[0] hold the input; the two buffers
// ping-pong.  Returns the index (0 or 1) of the buffer pair that holds the sorted output.
// Stable.  Temporaries come from the arena and are released on return.
// prof (optional) receives per-kernel HIP-event timings: "rs_hist", "rs_scan", "rs_scatter".
int radix_sort_pairs(uint64_t *keys[2], uint32_t *vals[2], size_t n, const int *shifts,
                     int npasses, Arena &arena, hipStream_t stream, Profiler *prof = nullptr);
int radix_sort_pairs(uint32_t *keys[2], uint32_t *vals[2], size_t n, const int *shifts,
                     int npasses, Arena &arena, hipStream_t stream, Profiler *prof = nullptr);

// ONE pass by the digit at `shift` that keeps only the low 16 bits of every key: the last pass of a window permutation
// (text_order.hip).  It lives with the sorts because its histogram kernel is the one every u32 sort uses.
void radix_pass_low16(const uint32_t *keys, const uint32_t *vals, uint16_t *keys16_out, uint32_t *vals_out, size_t n, int shift,
                      Arena &arena, hipStream_t stream, Profiler *prof = nullptr);

// The round-0 sort of the suffix array: pairs (initial_key(i), i) for i < text.n, sorted by the given
// digits.  The first pass computes the keys from the packed text on the fly (histogram and scatter
// kernels read 2 bits per base instead of 12 bytes per suffix, and no kernel writes the unsorted
// pairs); keys[0] / vals[0] are only used as ping-pong space from the second pass on.
int radix_sort_initial_keys(const PackedText &text, uint64_t *keys[2], uint32_t *vals[2], const int *shifts,
                            int npasses, Arena &arena, hipStream_t stream, Profiler *prof = nullptr);

// Plain 2-bit DNA (40-bit keys): the same sort with 8-byte records.  One most-significant-digit pass
// computes the keys from the text, partitions the suffixes by their first four bases (the top 8 key
// bits) and keeps only the LOW 32 key bits; four segmented passes then sort every bucket by those.
// The top byte of an element is implied by the bucket it lies in (seg_out, whose tile descriptors live
// in seg_mem: device memory for kSegDescWords * (n / kSortTile + 257) words that must outlive the call).  The sorted low halves end
// in keys32[1], the suffixes in vals[1].  12 + 4 * 24 bytes of traffic per suffix instead of
// 12 + 4 * 32 (hist + scatter, keys + values).
void radix_sort_dna_keys(const PackedText &text, uint32_t *keys32[2], uint32_t *vals[2], uint32_t *seg_mem,
                         SegView &seg_out, Arena &arena, hipStream_t stream, Profiler *prof = nullptr);

// Plain one-segment 2-bit DNA, 16-base key (text.hpp, kP16Syms): the most-significant-digit pass from the text
// and THREE segmented passes over the 24 key bits above the tag byte of the stored word [24 key bits][8-bit tag].
// The sorted words end in keys32[0], the suffixes in vals[0].  8 + 3 * 16 bytes of scatter traffic per suffix.
// Texts of 2^28 .. 1.13 * 10^9 suffixes: ONE segmented pass, then the 65 536 sub-buckets sorted in LDS (local_sort.hpp:
// local_sort_kernel) -- 8 + 16 + 16 bytes per suffix; from 3 * 2^28 suffixes up that kernel can do the regroup of round 0
// on the way (Round0Regroup below: the keys are then not written at all).
// (also segmented texts with a terminator table of at most kTermFew entries and segments of at least 16 symbols -- a
// prepared reverse-complement string --: key16_applicable says whether a text takes this sort)
bool key16_applicable(const PackedText &text);
// What the regroup kernel of round 0 produces from the sorted keys (sa_regroup.hip: regroup_kernel<true, 3>), asked of the
// sort itself: where the sub-buckets are finished in LDS the sorted keys are at hand -- LCP of every boundary the keys
// decide (0xffffffff = pending elsewhere), the elements that stay tied (slot and slot of their group's head, in slot
// order) and their number.  `done` says whether the sort did it (the keys are then NOT written).
// (with the 35-bit key, key35 below, its layout is 4)
struct Round0Regroup {
    uint32_t *lcp = nullptr;
    uint32_t *new_slot = nullptr, *new_grp = nullptr;
    uint32_t *d_total = nullptr;  // device: [0] survivors, [1] look-back error flag
    bool done = false;
};
void radix_sort_dna_keys16(const PackedText &text, uint32_t *keys32[2], uint32_t *vals[2], uint32_t *seg_mem,
                           SegView &seg_out, Arena &arena, hipStream_t stream, Profiler *prof = nullptr,
                           Round0Regroup *regroup = nullptr, bool key35 = false);
// The 35-bit key (text.hpp, kP35Syms; stored word [27 key bits][5-bit tag]): taken by plain one-segment texts exactly
// where radix_sort_dna_keys16 finishes the sub-buckets in LDS, whose two digits then have 10 and 9 bits -- the same
// passes and records, 17 1/2 bases sorted instead of 16 (NOLZSS_NO_KEY35 keeps the 16-base key).  The caller asks here
// and passes the answer on as key35: the regroup and the direct round behind the sort must know the layout.
bool key35_applicable(const PackedText &text);

// What local_sort_sub_buckets (local_sort.hpp) did, for the debug hook below.  regroup_any_size is an INPUT: the regroup on
// the way is taken whatever the size of the input (NOLZSS_LOCAL_REGROUP_MIN is a choice of speed, not of correctness).
struct LocalSortReport {
    bool regroup_any_size = false;
    bool fused_done = false;         // the form with the regroup of round 0 on the way ran and its checks held
    bool lookback_gave_up = false;   // ... ran, and a look-back gave up (or NOLZSS_TEST_LOCAL_LOOKBACK_FAILS said so)
    bool lane_order_failed = false;  // ctl[2] of local_sort_kernel: a lane-order check failed
    uint32_t listed = 0;             // sub-buckets beyond a workgroup's capacity, sent to the list
};
// Test hook (nolzss_debug_local_sort): what the key sorts do behind their most-significant-digit pass, on the caller's
// pairs.  keys[0] / vals[0] hold n pairs that lie in nb buckets [h_start[k], h_start[k + 1]); seg_view_of, ONE segmented
// pass by the digit at bit 24, then local_sort_sub_buckets(shift0, npass, key35, rg) with the table of that pass: the
// sorted pairs end in keys[0] / vals[0] (the keys are not written where rg->done).  The switch that a failed lane-order
// check throws is put back: report.lane_order_failed says it happened, later sorts of the process are not changed.
void debug_local_sort(uint32_t *keys[2], uint32_t *vals[2], size_t n, const uint32_t *h_start, uint32_t nb, int shift0, int npass,
                      bool key35, Round0Regroup *rg, LocalSortReport &report, Arena &arena, hipStream_t stream);

// The same sort on FUSED records [stored key word : 32 | suffix : 32] (round 4, A/B: NOLZSS_FUSED_SORT): rec[0] and rec[1]
// hold n 64-bit words each; the last pass writes the suffixes to sa_out and the key words to rec[0] (as 32-bit words).
void radix_sort_dna_keys16_fused(const PackedText &text, uint64_t *rec[2], uint32_t *sa_out, uint32_t *seg_mem,
                                 SegView &seg_out, Arena &arena, hipStream_t stream, Profiler *prof = nullptr);

// Independent records of 2-bit DNA (text.terms.seq_shift != 0), at most n / 2^16 of them: the records are
// the buckets -- the text is "partitioned" as it lies -- and every bucket is sorted on 8-byte records by the
// 32-bit key [kRecSyms bases][4-bit length tag], least significant digit first, the first pass making its
// pairs from the packed text: FOUR passes (8 + 3 * 16 bytes per suffix) where the general sort of the merged
// batch takes five on 12-byte records.  h_terms = host copy of the terminator table.  seg_mem: kSegDescWords *
// (n / kSortTile + records + 1) words.  The sorted keys end in keys32[0], the suffixes in vals[0].
void radix_sort_record_keys(const PackedText &text, const std::vector<uint32_t> &h_terms, uint32_t *keys32[2],
                            uint32_t *vals[2], uint32_t *seg_mem, SegView &seg_out, Arena &arena, hipStream_t stream,
                            Profiler *prof = nullptr);

// (u32 key, u32 value) pairs that lie in SEGMENTS [h_start[k], h_start[k + 1]) (h_start[0] = 0, the last entry = n), each
// segment sorted for itself by the low 8 * npasses key bits: the segments are the buckets of bucket-segmented passes on
// 8-byte records -- what the doubling rounds need for the members of their LARGE groups, whose group is known from where
// they lie (round 4: they used to sort 12-byte records by (group, key), eight passes instead of four).  Returns the
// index of the buffer pair that holds the result.
int radix_sort_segments_u32(uint32_t *keys[2], uint32_t *vals[2], size_t n, const std::vector<uint32_t> &h_start, int npasses,
                            Arena &arena, hipStream_t stream, Profiler *prof = nullptr);

}  // namespace nolzss
