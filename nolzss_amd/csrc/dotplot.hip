// dotplot.hip -- self dot-plot rasters rendered on the device from resident factor records ("Self
// dot-plot rasters"; C ABI: include/nolzss_hip.h, nolzss_dotplot_*).
//
// reference: plot_multiple_seq_self_lz_factor_plot_from_file, src/noLZSS/genomics/plots.py:352-900 (the segments of
// :477-504, datashade with ds.max('length') per strand :559-595, the hover overlay :600-666, the length slider
// :669-675), recomputed at every zoom.  Here a handle keeps the records of one factorisation in a device allocation of
// its own and a render turns a viewport into per-strand max-length rasters, optional count rasters and a hover table.
//
// Exact form.  Base pair t of factor (start, length, ref) lies at x = start + t, y = ref + t (forward) or
// ref + length - 1 - t (reverse complement); px = floor((x - x_lo) * W / Xs), py = floor((y - y_lo) * H / Ys) with
// Xs = x_hi - x_lo >= W and Ys = y_hi - y_lo >= H.  The t range clipped to the view is one interval [t0, t1).  Pixel
// column px holds t in [max(t0, ceil(px * Xs / W) + x_lo - start), min(t1, ceil((px + 1) * Xs / W) + x_lo - start)),
// and since y is monotonic in t, its rows are the contiguous range between the rows of the interval's two ends: the
// walk visits every column once and every row of the column once, so a factor counts once per pixel.  Widths: the
// coordinates of a factor that survives the cull are below 2^34, W, H, B <= 2^12: every product stays below 2^47 in
// signed 64-bit integers.  There is no floating point.
#include "factor_records.hpp"

namespace nolzss {
namespace {

constexpr int kThreads = kRecThreads;
constexpr uint32_t kMaxPixels = 4096;         // per axis, and hover bins
constexpr int64_t kMaxExtent = 1ll << 33;     // x_hi, y_hi
constexpr size_t kLdsBudget = 64 * 1024 - 64;  // as factor_maps.hip, what HIP grants without opting in, less the kernel's few static words
constexpr uint32_t kMaxStripCols = 4;
constexpr uint32_t kNoStrip = 0x80000000u;    // strip base before the first target: no column is inside
constexpr uint32_t kChunkRecords = 4096;      // contiguous records a workgroup takes at a time
constexpr uint32_t kSmallSpan = 4;            // a lane finishes a factor of fewer columns and rows than this alone

struct DotView {
    int64_t x_lo, x_hi, y_lo, y_hi;
    uint64_t len_lo, len_hi;  // len_hi = ~0: no upper bound
    uint32_t W, H, B;
    uint32_t want_counts;
    uint32_t strip_cols;      // pixel columns of the LDS strip; 0: every pixel goes to global memory
    uint32_t hover_lds;       // the hover keys are reduced in LDS first
};

// The sentinel search of the kept rule, out of line: it runs only for a factor below min_factor_length, and as a call
// its loop shares no register allocation with the cull around it ("Self dot-plot rasters").
__device__ __noinline__ bool kept_as_sentinel(KeepRule k, uint64_t i, uint64_t start) { return is_kept(k, i, start, 0); }

__device__ __forceinline__ int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }  // a >= 0, b > 0

// the accumulators a lane writes to: the workgroup's strip in LDS and the rasters in global memory
struct Planes {
    uint32_t *strip;     // [(column * planes + plane) * H + row], plane = strand (+ 2 for the counts)
    uint32_t *dirty;     // LDS flag: the strip holds something
    uint32_t *out;       // max forward, max rc, (count forward, count rc): W * H each
    uint32_t c0;         // first pixel column of the strip
    uint32_t n_planes;
};

// The max planes only grow, so a cell is read with a plain load first and the atomic skipped when it already holds
// at least `length`: a stale value from another XCD's L2 can only be smaller than the truth, which costs a redundant
// atomic and never a wrong result.
__device__ __forceinline__ void raise_global(uint32_t *cell, uint32_t length) {
    if (__atomic_load_n(cell, __ATOMIC_RELAXED) < length) atomicMax(cell, length);
}

__device__ __forceinline__ void put(const DotView &v, const Planes &p, uint32_t px, uint32_t row, uint32_t rc,
                                    uint32_t length) {
    const uint32_t col = px - p.c0;
    if (col < v.strip_cols) {
        uint32_t *cell = p.strip + ((size_t)col * p.n_planes + rc) * v.H + row;
        if (*cell < length) atomicMax(cell, length);
        if (v.want_counts) atomicAdd(cell + 2 * (size_t)v.H, 1u);
        *p.dirty = 1u;
        return;
    }
    const size_t wh = (size_t)v.W * v.H, at = (size_t)row * v.W + px;
    raise_global(p.out + rc * wh + at, length);
    if (v.want_counts) atomicAdd(p.out + (2 + rc) * wh + at, 1u);
}

// pixel columns px_begin, px_begin + step, .. <= px_last of one factor: rows of each column in the inner loop
__device__ __forceinline__ void walk_columns(const DotView &v, const Planes &p, int64_t start, int64_t y_base,
                                             uint32_t rc, uint32_t length, int64_t t0, int64_t t1, uint32_t px_begin,
                                             uint32_t px_last, uint32_t step) {
    const int64_t Xs = v.x_hi - v.x_lo, Ys = v.y_hi - v.y_lo, shift = v.x_lo - start;
    for (uint32_t px = px_begin; px <= px_last; px += step) {
        const int64_t ca = ceil_div((int64_t)px * Xs, v.W) + shift, cb = ceil_div((int64_t)(px + 1) * Xs, v.W) + shift;
        const int64_t ta = ca > t0 ? ca : t0, tb = cb < t1 ? cb : t1;
        if (ta >= tb) continue;
        const int64_t ya = rc ? y_base - ta : y_base + ta, yb = rc ? y_base - (tb - 1) : y_base + (tb - 1);
        const uint32_t ra = (uint32_t)(((ya - v.y_lo) * v.H) / Ys), rb = (uint32_t)(((yb - v.y_lo) * v.H) / Ys);
        const uint32_t lo = ra < rb ? ra : rb, hi = ra < rb ? rb : ra;
        for (uint32_t row = lo; row <= hi; ++row) put(v, p, px, row, rc, length);
    }
}

// strip -> rasters: one atomic per non-zero cell; leaves the strip zero
__device__ __forceinline__ void flush_strip(const DotView &v, const Planes &p) {
    const uint32_t per_col = p.n_planes * v.H, cells = v.strip_cols * per_col;
    const size_t wh = (size_t)v.W * v.H;
    for (uint32_t c = threadIdx.x; c < cells; c += kThreads) {
        const uint32_t val = p.strip[c];
        if (!val) continue;
        p.strip[c] = 0;
        const uint32_t px = p.c0 + c / per_col, plane = (c % per_col) / v.H, row = c % v.H;
        if (px >= v.W) continue;
        uint32_t *cell = p.out + plane * wh + (size_t)row * v.W + px;
        if (plane < 2) raise_global(cell, val);
        else atomicAdd(cell, val);
    }
}

// Workgroups take chunks of kChunkRecords contiguous records, grid-stride over the chunks, 256 records per step.
// Records from the pipeline are sorted by start, so the records of a step begin in one or a few adjacent pixel
// columns: the strip is aimed at the column of the step's first record and flushed when a step begins outside it.
// Per step: cull (length window, view, kept rule), clip to [t0, t1), hover key, then by size: one pixel -- the lane
// writes it (count increments to global memory combined across the wave first); fewer than kSmallSpan columns and
// rows -- the lane walks it; otherwise the wave takes the factors one by one, a pixel column per lane.
// Integer max and add only: the rasters do not depend on the order.
__global__ __launch_bounds__(kThreads) void dotplot_raster_kernel(const Rec *__restrict__ recs, uint64_t z,
                                                                  KeepRule keep, DotView v, uint32_t *out,
                                                                  unsigned long long *hover_keys,
                                                                  unsigned long long *visible) {
    extern __shared__ unsigned long long lds_dyn[];
    __shared__ uint32_t dirty;
    __shared__ unsigned long long vis_sh[2];
    unsigned long long *hover_lds = lds_dyn;
    Planes p;
    p.strip = reinterpret_cast<uint32_t *>(lds_dyn + (v.hover_lds ? v.B : 0u));
    p.dirty = &dirty;
    p.out = out;
    p.c0 = kNoStrip;
    p.n_planes = v.want_counts ? 4u : 2u;
    const uint32_t strip_cells = v.strip_cols * p.n_planes * v.H;
    for (uint32_t c = threadIdx.x; c < strip_cells; c += kThreads) p.strip[c] = 0;
    if (v.hover_lds)
        for (uint32_t c = threadIdx.x; c < v.B; c += kThreads) hover_lds[c] = 0;
    if (threadIdx.x == 0) {
        dirty = 0;
        vis_sh[0] = vis_sh[1] = 0;
    }
    __syncthreads();

    const int64_t Xs = v.x_hi - v.x_lo, Ys = v.y_hi - v.y_lo;
    const uint32_t lane = (uint32_t)lane_id();
    const size_t wh = (size_t)v.W * v.H;
    unsigned long long n_vis[2] = {0, 0};
    const uint64_t chunks = (z + kChunkRecords - 1) / kChunkRecords;
    for (uint64_t chunk = blockIdx.x; chunk < chunks; chunk += gridDim.x) {
        const uint64_t chunk_begin = chunk * kChunkRecords;
        const uint64_t chunk_end = chunk_begin + kChunkRecords < z ? chunk_begin + kChunkRecords : z;
        for (uint64_t base = chunk_begin; base < chunk_end; base += kThreads) {  // (the same trips for every lane)
            if (v.strip_cols) {
                // aim the strip: every lane reads the same record, so the branch and its barriers are uniform
                const uint64_t s0 = recs[base].start;
                if (s0 < (uint64_t)v.x_hi) {
                    const uint32_t col = (int64_t)s0 <= v.x_lo ? 0u : (uint32_t)((((int64_t)s0 - v.x_lo) * v.W) / Xs);
                    if (col - p.c0 >= v.strip_cols) {
                        __syncthreads();
                        const uint32_t d = dirty;
                        __syncthreads();
                        if (d) {
                            flush_strip(v, p);
                            if (threadIdx.x == 0) dirty = 0;
                            __syncthreads();
                        }
                        p.c0 = col;
                    }
                }
            }
            const uint64_t i = base + threadIdx.x;
            bool vis = false;
            uint32_t rc = 0, length = 0, px_a = 0, px_b = 0, row_a = 0, row_b = 0;
            int64_t start = 0, y_base = 0, t0 = 0, t1 = 0;
            if (i < chunk_end) {
                const Rec f = recs[i];
                const uint64_t r = f.ref & ~kRcMask;
                // cull before any arithmetic: the kept rule, the length window, the view (both strands cover y in
                // [ref, ref + length)).  What passes has start, ref < 2^33 and length < 2^32.
                const bool kept = f.length >= keep.min_len || kept_as_sentinel(keep, i, f.start);
                if (kept && f.length >= v.len_lo && f.length <= v.len_hi && f.length != 0 &&
                    f.start < (uint64_t)v.x_hi && sat_add(f.start, f.length) > (uint64_t)v.x_lo &&
                    r < (uint64_t)v.y_hi && sat_add(r, f.length) > (uint64_t)v.y_lo) {
                    rc = (f.ref & kRcMask) ? 1u : 0u;
                    length = (uint32_t)f.length;
                    start = (int64_t)f.start;
                    const int64_t ref = (int64_t)r, len = (int64_t)f.length;
                    y_base = rc ? ref + len - 1 : ref;  // y of t = 0
                    // y in [y_lo, y_hi): forward t in [y_lo - ref, y_hi - ref), rc t in [ref + len - y_hi, ref + len - y_lo)
                    const int64_t ty0 = rc ? ref + len - v.y_hi : v.y_lo - ref, ty1 = rc ? ref + len - v.y_lo : v.y_hi - ref;
                    t0 = v.x_lo - start;
                    t0 = t0 > ty0 ? t0 : ty0;
                    t0 = t0 > 0 ? t0 : 0;
                    t1 = v.x_hi - start;
                    t1 = t1 < ty1 ? t1 : ty1;
                    t1 = t1 < len ? t1 : len;
                    vis = t0 < t1;
                }
                if (vis) {
                    ++n_vis[rc];
                    px_a = (uint32_t)(((start + t0 - v.x_lo) * v.W) / Xs);
                    px_b = (uint32_t)(((start + t1 - 1 - v.x_lo) * v.W) / Xs);
                    const int64_t ya = rc ? y_base - t0 : y_base + t0, yb = rc ? y_base - (t1 - 1) : y_base + (t1 - 1);
                    row_a = (uint32_t)(((ya - v.y_lo) * v.H) / Ys);
                    row_b = (uint32_t)(((yb - v.y_lo) * v.H) / Ys);
                    const int64_t mid2 = 2 * start + (int64_t)length;
                    if (v.B && mid2 >= 2 * v.x_lo && mid2 < 2 * v.x_hi) {
                        // greatest length, then smallest index
                        const unsigned long long key = ((unsigned long long)length << 32) | (0xffffffffu - (uint32_t)i);
                        const uint32_t c = (uint32_t)(((mid2 - 2 * v.x_lo) * v.B) / (2 * Xs));
                        if (v.hover_lds) {
                            if (hover_lds[c] < key) atomicMax(&hover_lds[c], key);
                        } else if (__atomic_load_n(&hover_keys[c], __ATOMIC_RELAXED) < key) {
                            atomicMax(&hover_keys[c], key);
                        }
                    }
                }
            }
            const uint32_t rows = row_a < row_b ? row_b - row_a : row_a - row_b;
            const bool single = vis && px_a == px_b && rows == 0;
            const bool small = vis && !single && px_b - px_a < kSmallSpan && rows < kSmallSpan;
            const bool shared = vis && !single && !small;

            // one pixel
            bool add_global = false;
            size_t count_cell = 0;
            if (single) {
                const uint32_t col = px_a - p.c0;
                if (col < v.strip_cols) {
                    uint32_t *cell = p.strip + ((size_t)col * p.n_planes + rc) * v.H + row_a;
                    if (*cell < length) atomicMax(cell, length);
                    if (v.want_counts) atomicAdd(cell + 2 * (size_t)v.H, 1u);
                    dirty = 1u;
                } else {
                    const size_t at = (size_t)row_a * v.W + px_a;
                    raise_global(out + rc * wh + at, length);
                    add_global = v.want_counts != 0;
                    count_cell = (2 + rc) * wh + at;
                }
            }
            if (v.want_counts) {
                // equal pixels inside the wave: one atomic with their number
                unsigned long long todo = __ballot(add_global);
                while (todo) {
                    const int leader = __ffsll((long long)todo) - 1;
                    const size_t cell = (size_t)__shfl((unsigned long long)count_cell, leader);
                    const unsigned long long same = __ballot(add_global && count_cell == cell);
                    if ((int)lane == leader) atomicAdd(out + cell, (uint32_t)__popcll(same));
                    todo &= ~same;
                }
            }
            // a few pixels: the lane's own walk
            if (small) walk_columns(v, p, start, y_base, rc, length, t0, t1, px_a, px_b, 1);
            // many pixels: the wave walks them together, one pixel column per lane
            unsigned long long queue = __ballot(shared);
            while (queue) {
                const int src = __ffsll((long long)queue) - 1;
                queue &= queue - 1;
                const int64_t q_start = __shfl((long long)start, src), q_y = __shfl((long long)y_base, src);
                const int64_t q_t0 = __shfl((long long)t0, src), q_t1 = __shfl((long long)t1, src);
                const uint32_t q_rc = __shfl(rc, src), q_len = __shfl(length, src);
                const uint32_t q_a = __shfl(px_a, src), q_b = __shfl(px_b, src);
                walk_columns(v, p, q_start, q_y, q_rc, q_len, q_t0, q_t1, q_a + lane, q_b, 64);
            }
        }
    }
    if (n_vis[0]) atomicAdd(&vis_sh[0], n_vis[0]);
    if (n_vis[1]) atomicAdd(&vis_sh[1], n_vis[1]);
    __syncthreads();
    if (v.strip_cols && dirty) flush_strip(v, p);
    if (v.hover_lds)
        for (uint32_t c = threadIdx.x; c < v.B; c += kThreads) {
            const unsigned long long key = hover_lds[c];
            if (key && __atomic_load_n(&hover_keys[c], __ATOMIC_RELAXED) < key) atomicMax(&hover_keys[c], key);
        }
    if (threadIdx.x < 2 && vis_sh[threadIdx.x]) atomicAdd(&visible[threadIdx.x], vis_sh[threadIdx.x]);
}

// the winning record of every hover column (start, length, ref: B entries each, zero where the column is empty)
__global__ void hover_gather_kernel(const Rec *__restrict__ recs, const unsigned long long *__restrict__ keys,
                                    uint32_t B, unsigned long long *__restrict__ table) {
    const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= B) return;
    const unsigned long long key = keys[c];
    if (!key) return;
    const Rec f = recs[0xffffffffu - (uint32_t)key];
    table[c] = f.start;
    table[B + c] = f.length;
    table[2 * (size_t)B + c] = f.ref;
}

// found[k] = 1 when a record starts at positions[k] (records sorted by start, as the pipeline leaves them)
__global__ void sentinel_hits_kernel(const Rec *__restrict__ recs, uint64_t z, const uint64_t *__restrict__ positions,
                                     uint32_t n, uint32_t *__restrict__ found) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const uint64_t pos = positions[k];
    uint64_t lo = 0, hi = z;
    while (lo < hi) {
        const uint64_t mid = (lo + hi) >> 1;
        if (recs[mid].start < pos) lo = mid + 1;
        else hi = mid;
    }
    found[k] = lo < z && recs[lo].start == pos ? 1u : 0u;
}

bool force_global() {  // every pixel and hover key straight to global memory, for A/B runs and tests
    const char *e = getenv("NOLZSS_DOTPLOT_GLOBAL");
    return e && *e && *e != '0';
}

}  // namespace
}  // namespace nolzss

using namespace nolzss;
using namespace nolzss::api;

// The handle: the records and the sorted sentinel keys in DeviceBufs (device_buf.hpp), and the statistics at
// min_factor_length = 1.
struct nolzss_dotplot {
    int device = 0;
    uint64_t z = 0;
    DeviceBuf recs, sentinel_keys;
    std::vector<uint64_t> sentinels;  // ascending: factor indices (by_index) or start positions
    bool by_index = false;
    MapStats st{0, 0, 0, 0, 0, 0, 0};
    std::vector<uint64_t> sentinel_starts;
    const Rec *d_recs() const { return recs.as<Rec>(); }
    const uint64_t *d_sentinels() const { return sentinel_keys.as<uint64_t>(); }
};

namespace {

// Takes z records (device memory of the arena, or host memory) into the handle and computes its statistics.
void adopt_records(Context &ctx, nolzss_dotplot &h, const void *recs, bool on_device, uint64_t z) {
    hipStream_t s = ctx.stream;
    ProfScope whole(ctx.profiler(), "dotplot_open", s);
    if (z > 0xffffffffull) throw std::invalid_argument("z: the hover table indexes factors in 32 bits, 2^32 or more are refused");
    h.z = z;
    h.device = ctx.device;
    if (z == 0) return;
    h.recs.alloc(ctx, sizeof(Rec) * z);
    if (on_device) {
        HIP_CHECK(hipMemcpyAsync(h.recs.get(), recs, sizeof(Rec) * z, hipMemcpyDeviceToDevice, s));
    } else {
        ProfScope ps(ctx.profiler(), "records_h2d", s, 24.0 * (double)z);
        upload_bytes(ctx, h.recs.get(), recs, sizeof(Rec) * z);
    }
    if (!h.sentinels.empty()) {
        h.sentinel_keys.alloc(ctx, sizeof(uint64_t) * h.sentinels.size());
        HIP_CHECK(hipMemcpyAsync(h.sentinel_keys.get(), h.sentinels.data(), sizeof(uint64_t) * h.sentinels.size(),
                                 hipMemcpyHostToDevice, s));
    }
    MapStats *d_st = ctx.arena.alloc<MapStats>(1);
    const MapStats init{0, 0, ~0ull, 0, 0, 0, 0};
    HIP_CHECK(hipMemcpyAsync(d_st, &init, sizeof init, hipMemcpyHostToDevice, s));
    const KeepRule keep{1, h.d_sentinels(), (uint32_t)h.sentinels.size(), h.by_index ? 1u : 0u, 0};
    {
        ProfScope ps(ctx.profiler(), "map_stats", s, 24.0 * (double)z);
        map_stats_kernel<<<record_grid(z), kRecThreads, 0, s>>>(h.d_recs(), z, keep, d_st);
        KERNEL_CHECK();
    }
    HIP_CHECK(hipMemcpyAsync(&h.st, d_st, sizeof h.st, hipMemcpyDeviceToHost, s));
    std::vector<uint32_t> found;
    if (!h.by_index && !h.sentinels.empty()) {  // the sentinels that begin a factor
        const uint32_t n = (uint32_t)h.sentinels.size();
        uint32_t *d_found = ctx.arena.alloc<uint32_t>(n);
        sentinel_hits_kernel<<<(unsigned)div_up((size_t)n, (size_t)256), 256, 0, s>>>(h.d_recs(), z, h.d_sentinels(), n, d_found);
        KERNEL_CHECK();
        found.resize(n);
        HIP_CHECK(hipMemcpyAsync(found.data(), d_found, sizeof(uint32_t) * n, hipMemcpyDeviceToHost, s));
    }
    HIP_CHECK(hipStreamSynchronize(s));
    for (size_t k = 0; k < found.size(); ++k)
        if (found[k]) h.sentinel_starts.push_back(h.sentinels[k]);
    if (h.st.kept_fwd + h.st.kept_rc == 0) h.st.min_length = 0;
    if (h.st.max_length > 0xffffffffull)
        throw std::invalid_argument("length: a record of 2^32 bases or more (the rasters hold lengths in 32 bits)");
}

void check_handle_out(nolzss_dotplot **h) {
    if (!h) throw std::invalid_argument("output pointer is null");
    *h = nullptr;
}

void check_view(const nolzss_dotplot_view &v) {
    if (v.width < 1 || v.width > kMaxPixels) throw std::invalid_argument("width must be between 1 and 4096");
    if (v.height < 1 || v.height > kMaxPixels) throw std::invalid_argument("height must be between 1 and 4096");
    if (v.hover_bins > kMaxPixels) throw std::invalid_argument("hover_bins must be at most 4096");
    if (v.x_lo >= v.x_hi) throw std::invalid_argument("x_lo must be below x_hi");
    if (v.y_lo >= v.y_hi) throw std::invalid_argument("y_lo must be below y_hi");
    if (v.x_hi > (uint64_t)kMaxExtent) throw std::invalid_argument("x_hi beyond 2^33");
    if (v.y_hi > (uint64_t)kMaxExtent) throw std::invalid_argument("y_hi beyond 2^33");
    if (v.x_hi - v.x_lo < v.width)
        throw std::invalid_argument("x_hi - x_lo is below width: fewer bases than pixels, shrink the raster");
    if (v.y_hi - v.y_lo < v.height)
        throw std::invalid_argument("y_hi - y_lo is below height: fewer bases than pixels, shrink the raster");
    if (v.len_hi && v.len_lo > v.len_hi) throw std::invalid_argument("len_lo must not exceed len_hi");
}

template <typename T> T *calloc_array(size_t count) {
    T *p = static_cast<T *>(std::calloc(count ? count : 1, sizeof(T)));
    if (!p) throw std::bad_alloc();
    return p;
}

void render(const nolzss_dotplot &h, const nolzss_dotplot_view &v, nolzss_dotplot_raster *out) {
    const size_t wh = (size_t)v.width * v.height;
    const uint32_t B = v.hover_bins, n_planes = v.want_counts ? 4u : 2u;
    out->width = v.width;
    out->height = v.height;
    out->hover_bins = B;
    out->max_forward = calloc_array<uint32_t>(wh);
    out->max_rc = calloc_array<uint32_t>(wh);
    if (v.want_counts) {
        out->count_forward = calloc_array<uint32_t>(wh);
        out->count_rc = calloc_array<uint32_t>(wh);
    }
    if (B) {
        out->hover_start = calloc_array<uint64_t>(B);
        out->hover_length = calloc_array<uint64_t>(B);
        out->hover_ref = calloc_array<uint64_t>(B);
    }
    if (h.z == 0) return;

    Session ses(h.device, nullptr);
    Context &ctx = ses.ctx();
    hipStream_t s = ctx.stream;
    const size_t raster_bytes = sizeof(uint32_t) * n_planes * wh;
    reserve_arena_for(ctx, 0, raster_bytes + 32 * (size_t)B + (size_t(1) << 20));
    uint32_t *d_out = ctx.arena.alloc<uint32_t>(n_planes * wh);
    unsigned long long *d_vis = ctx.arena.alloc<unsigned long long>(2);
    unsigned long long *d_keys = ctx.arena.alloc<unsigned long long>(B ? B : 1);
    unsigned long long *d_table = ctx.arena.alloc<unsigned long long>(B ? 3 * (size_t)B : 1);

    DotView dv;
    dv.x_lo = (int64_t)v.x_lo;
    dv.x_hi = (int64_t)v.x_hi;
    dv.y_lo = (int64_t)v.y_lo;
    dv.y_hi = (int64_t)v.y_hi;
    dv.len_lo = v.len_lo;
    dv.len_hi = v.len_hi ? v.len_hi : ~0ull;
    dv.W = v.width;
    dv.H = v.height;
    dv.B = B;
    dv.want_counts = v.want_counts ? 1u : 0u;
    // LDS: the strip first (as many columns as fit, at most kMaxStripCols), the hover keys if they still fit
    const size_t col_bytes = sizeof(uint32_t) * n_planes * v.height, hover_bytes = sizeof(uint64_t) * B;
    const bool global_form = force_global();
    dv.strip_cols = global_form ? 0u : (uint32_t)std::min<size_t>(kMaxStripCols, kLdsBudget / col_bytes);
    dv.strip_cols = std::min(dv.strip_cols, v.width);
    dv.hover_lds = !global_form && B && dv.strip_cols * col_bytes + hover_bytes <= kLdsBudget ? 1u : 0u;
    const size_t lds_bytes = dv.strip_cols * col_bytes + (dv.hover_lds ? hover_bytes : 0);
    const KeepRule keep{v.min_factor_length, h.d_sentinels(), (uint32_t)h.sentinels.size(), h.by_index ? 1u : 0u, 0};
    {
        ProfScope whole(ctx.profiler(), "dotplot_render", s);
        HIP_CHECK(hipMemsetAsync(d_out, 0, raster_bytes, s));
        HIP_CHECK(hipMemsetAsync(d_vis, 0, 2 * sizeof(unsigned long long), s));
        HIP_CHECK(hipMemsetAsync(d_keys, 0, sizeof(unsigned long long) * (B ? B : 1), s));
        HIP_CHECK(hipMemsetAsync(d_table, 0, sizeof(unsigned long long) * (B ? 3 * (size_t)B : 1), s));
        {
            ProfScope ps(ctx.profiler(), "dotplot_raster", s, 24.0 * (double)h.z);
            const uint64_t chunks = div_up((size_t)h.z, (size_t)kChunkRecords);
            const unsigned grid = (unsigned)std::min<uint64_t>(chunks, 1024);
            dotplot_raster_kernel<<<grid, kThreads, lds_bytes, s>>>(h.d_recs(), h.z, keep, dv, d_out, d_keys, d_vis);
            KERNEL_CHECK();
        }
        if (B) {
            hover_gather_kernel<<<(unsigned)div_up((size_t)B, (size_t)256), 256, 0, s>>>(h.d_recs(), d_keys, B, d_table);
            KERNEL_CHECK();
        }
    }
    unsigned long long vis[2] = {0, 0};
    HIP_CHECK(hipMemcpyAsync(vis, d_vis, sizeof vis, hipMemcpyDeviceToHost, s));
    // the planes through download_bytes: a 4096 x 4096 plane is 64 MB, above its threshold for the staged copy
    uint32_t *const planes[4] = {out->max_forward, out->max_rc, out->count_forward, out->count_rc};
    for (uint32_t k = 0; k < n_planes; ++k) download_bytes(ctx, planes[k], d_out + k * wh, sizeof(uint32_t) * wh);
    if (B) {
        HIP_CHECK(hipMemcpyAsync(out->hover_start, d_table, sizeof(uint64_t) * B, hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipMemcpyAsync(out->hover_length, d_table + B, sizeof(uint64_t) * B, hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipMemcpyAsync(out->hover_ref, d_table + 2 * (size_t)B, sizeof(uint64_t) * B, hipMemcpyDeviceToHost, s));
    }
    HIP_CHECK(hipStreamSynchronize(s));
    out->visible_forward = vis[0];
    out->visible_rc = vis[1];
    ctx.prof.collect();
}

}  // namespace

extern "C" {

int nolzss_dotplot_open_text(const uint8_t *text, size_t n, int with_rc, int device, nolzss_dotplot **h) {
    return guarded([&] {
        check_handle_out(h);
        std::unique_ptr<nolzss_dotplot> dp(new nolzss_dotplot);
        dp->device = device;
        if (check_text_source(text, n, with_rc != 0)) {
            Session ses(device, nullptr);
            Context &ctx = ses.ctx();
            const ChainRequest recs = text_records(ctx, text, n, with_rc != 0, size_t(1) << 20);
            adopt_records(ctx, *dp, recs.d_records, true, recs.z);
            ctx.prof.collect();
        }
        *h = dp.release();
    });
}

int nolzss_dotplot_open_fasta(const char *path, int with_rc, int sanitize_mode, int device, nolzss_dotplot **h) {
    return guarded([&] {
        check_handle_out(h);
        if (!path) throw std::invalid_argument("path is null");
        check_sanitize_mode(sanitize_mode);
        std::unique_ptr<nolzss_dotplot> dp(new nolzss_dotplot);
        dp->device = device;
        FastaText ft;
        read_fasta_text(path, with_rc != 0, sanitize_mode == 1, ft);
        if (!ft.empty) {
            Session ses(device, nullptr);
            Context &ctx = ses.ctx();
            const ChainRequest recs = fasta_records(ctx, ft, with_rc != 0, size_t(1) << 20, dp->sentinels);
            adopt_records(ctx, *dp, recs.d_records, true, recs.z);
            ctx.prof.collect();
        }
        *h = dp.release();
    });
}

int nolzss_dotplot_open_records(const nolzss_factor *factors, size_t z, const uint64_t *sentinel_factor_indices,
                                size_t n_sentinels, int device, nolzss_dotplot **h) {
    return guarded([&] {
        check_handle_out(h);
        if (z && !factors) throw std::invalid_argument("factors pointer is null");
        if (n_sentinels && !sentinel_factor_indices) throw std::invalid_argument("sentinel_factor_indices is null");
        std::unique_ptr<nolzss_dotplot> dp(new nolzss_dotplot);
        dp->device = device;
        dp->by_index = true;
        if (z) {
            dp->sentinels.assign(sentinel_factor_indices, sentinel_factor_indices + n_sentinels);
            std::sort(dp->sentinels.begin(), dp->sentinels.end());
            dp->sentinels.erase(std::unique(dp->sentinels.begin(), dp->sentinels.end()), dp->sentinels.end());
            // The reference (:528-531) keeps the caller's index order; here the starts are ascending and distinct
            // whatever the order of the records, which is what the sequence boundaries are cut from.
            for (uint64_t idx : dp->sentinels)
                if (idx < z) dp->sentinel_starts.push_back(factors[idx].start);
            std::sort(dp->sentinel_starts.begin(), dp->sentinel_starts.end());
            dp->sentinel_starts.erase(std::unique(dp->sentinel_starts.begin(), dp->sentinel_starts.end()),
                                      dp->sentinel_starts.end());
            Session ses(device, nullptr);
            Context &ctx = ses.ctx();
            reserve_arena_for(ctx, 0, size_t(1) << 20);
            adopt_records(ctx, *dp, factors, false, z);
            ctx.prof.collect();
        }
        *h = dp.release();
    });
}

int nolzss_dotplot_info(const nolzss_dotplot *h, nolzss_dotplot_summary *info) {
    return guarded([&] {
        if (!h || !info) throw std::invalid_argument("handle or output pointer is null");
        std::memset(info, 0, sizeof *info);
        info->z = h->z;
        info->x_max = h->st.x_max;
        info->y_max = h->st.y_max;
        info->min_length = h->st.min_length;
        info->max_length = h->st.max_length;
        info->kept_forward = h->st.kept_fwd;
        info->kept_rc = h->st.kept_rc;
        info->device = h->device;
        info->sentinel_starts = h->sentinel_starts.empty() ? nullptr : h->sentinel_starts.data();
        info->n_sentinel_starts = h->sentinel_starts.size();
    });
}

int nolzss_dotplot_render(const nolzss_dotplot *h, const nolzss_dotplot_view *view, nolzss_dotplot_raster *out) {
    return guarded([&] {
        if (!out) throw std::invalid_argument("output pointer is null");
        std::memset(out, 0, sizeof *out);
        if (!h) throw std::invalid_argument("handle is null");
        if (!view) throw std::invalid_argument("view is null");
        check_view(*view);
        try {
            render(*h, *view, out);
        } catch (...) {
            nolzss_free_dotplot_raster(out);
            throw;
        }
    });
}

void nolzss_free_dotplot_raster(nolzss_dotplot_raster *out) {
    if (!out) return;
    std::free(out->max_forward);
    std::free(out->max_rc);
    std::free(out->count_forward);
    std::free(out->count_rc);
    std::free(out->hover_start);
    std::free(out->hover_length);
    std::free(out->hover_ref);
    std::memset(out, 0, sizeof *out);
}

int nolzss_dotplot_close(nolzss_dotplot *h) {
    return guarded([&] { delete h; });
}

}  // extern "C"
