// factor_records.hpp -- what the kernels that read the factor records in HBM share (factor_maps.hip, dotplot.hip):
// the record, the kept-factor rule of the reference's plots (src/noLZSS/genomics/plots.py:451-458, :2149-2157) and the
// one-pass statistics over the kept records.
#pragma once
#include "api_internal.hpp"

namespace nolzss {

constexpr int kRecThreads = 256;
constexpr uint64_t kRcMask = 1ull << 63;

struct Rec {
    uint64_t start, length, ref;
};

// min_length starts at ~0; the rest at 0
struct MapStats {
    unsigned long long x_max, y_max, min_length, max_length, max_start, kept_fwd, kept_rc;
};

// length >= min_len, or a sentinel factor: key = the factor's index (records source) or its start (sentinel
// positions of the prepared string), looked up in the ascending list
struct KeepRule {
    uint64_t min_len;
    const uint64_t *sentinels;
    uint32_t n_sentinels;
    uint32_t by_index;
    uint64_t base_index;  // index of the first record of this chunk
};

__device__ __forceinline__ bool is_kept(const KeepRule &k, uint64_t i, uint64_t start, uint64_t length) {
    if (length >= k.min_len) return true;
    const uint64_t key = k.by_index ? k.base_index + i : start;
    uint32_t lo = 0, hi = k.n_sentinels;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (k.sentinels[mid] < key) lo = mid + 1;
        else hi = mid;
    }
    return lo < k.n_sentinels && k.sentinels[lo] == key;
}

__device__ __forceinline__ uint64_t sat_add(uint64_t a, uint64_t b) { return a + b < a ? ~0ull : a + b; }

// extents, length range, largest start and the kept counts per strand
static __global__ __launch_bounds__(kRecThreads) void map_stats_kernel(const Rec *__restrict__ recs, uint64_t z,
                                                                       KeepRule keep, MapStats *__restrict__ out) {
    __shared__ MapStats sh;
    if (threadIdx.x == 0) sh = MapStats{0, 0, ~0ull, 0, 0, 0, 0};
    __syncthreads();
    MapStats m{0, 0, ~0ull, 0, 0, 0, 0};
    const uint64_t stride = (uint64_t)gridDim.x * kRecThreads;
    for (uint64_t i = (uint64_t)blockIdx.x * kRecThreads + threadIdx.x; i < z; i += stride) {
        const Rec f = recs[i];
        if (!is_kept(keep, i, f.start, f.length)) continue;
        const uint64_t r = f.ref & ~kRcMask;
        const uint64_t xe = sat_add(f.start, f.length), ye = sat_add(r, f.length);
        m.x_max = xe > m.x_max ? xe : m.x_max;
        m.y_max = ye > m.y_max ? ye : m.y_max;
        m.min_length = f.length < m.min_length ? f.length : m.min_length;
        m.max_length = f.length > m.max_length ? f.length : m.max_length;
        m.max_start = f.start > m.max_start ? f.start : m.max_start;
        if (f.ref & kRcMask) ++m.kept_rc;
        else ++m.kept_fwd;
    }
    if (m.kept_fwd | m.kept_rc) {
        atomicMax(&sh.x_max, m.x_max);
        atomicMax(&sh.y_max, m.y_max);
        atomicMin(&sh.min_length, m.min_length);
        atomicMax(&sh.max_length, m.max_length);
        atomicMax(&sh.max_start, m.max_start);
        if (m.kept_fwd) atomicAdd(&sh.kept_fwd, m.kept_fwd);
        if (m.kept_rc) atomicAdd(&sh.kept_rc, m.kept_rc);
    }
    __syncthreads();
    if (threadIdx.x == 0 && (sh.kept_fwd | sh.kept_rc)) {
        atomicMax(&out->x_max, sh.x_max);
        atomicMax(&out->y_max, sh.y_max);
        atomicMin(&out->min_length, sh.min_length);
        atomicMax(&out->max_length, sh.max_length);
        atomicMax(&out->max_start, sh.max_start);
        if (sh.kept_fwd) atomicAdd(&out->kept_fwd, sh.kept_fwd);
        if (sh.kept_rc) atomicAdd(&out->kept_rc, sh.kept_rc);
    }
}

// workgroups of kRecThreads for a grid-stride pass over `items` records
inline unsigned record_grid(uint64_t items) {
    uint64_t g = div_up(items, (uint64_t)kRecThreads);
    if (g < 1) g = 1;
    return (unsigned)(g > 1024 ? 1024 : g);
}

namespace api {

// ---- the pipeline runs that leave their records in the arena (factor_maps.hip; also dotplot.hip) ----------------
// The refusals of nolzss_count_factors / nolzss_count_factors_dna_w_rc; false: nothing to factorize.
bool check_text_source(const uint8_t *text, size_t n, bool with_rc);
// Plain mode over the bytes, rc mode over T s0 rc(T) s1 prepared on the device; `extra`: arena bytes the caller
// takes afterwards.  Returns z and the records in the arena (ChainRequest, pipeline.hpp; the caller's Session owns the mark).
ChainRequest text_records(Context &ctx, const uint8_t *text, size_t n, bool with_rc, size_t extra);
// The prepared string of read_fasta_text; sentinels: the byte behind every forward record but the end of the string.
ChainRequest fasta_records(Context &ctx, const FastaText &ft, bool with_rc, size_t extra,
                           std::vector<uint64_t> &sentinels);

}  // namespace api
}  // namespace nolzss
