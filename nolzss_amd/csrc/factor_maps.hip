// factor_maps.hip -- the strand-bias grid and the space-scale histogram of the factors, binned on the device
// ("Strand-bias and space-scale maps"; C ABI: include/nolzss_hip.h, nolzss_factor_maps_*).
//
// reference: _compute_strand_bias_grid, src/noLZSS/genomics/plots.py:1961-2075 (the segment of every factor split at
// the cell edges, the covered nucleotides summed per cell and strand) and the numpy.histogram2d of
// plot_space_scale_heatmap, :2559-2614; the kept-factor rule of :2149-2157.
//
// Exact form of the grid.  With unit = x_bins * y_bins and t = (x - start) * unit, the x edge k lies at
// t = k * x_max * y_bins - start * unit and the y edge j at t = j * y_max * x_bins - ref * unit (forward) or
// (ref + length) * unit - j * y_max * x_bins (reverse complement): integers.  A lane walks the merged sequence of
// these crossings from t = 0 to length * unit, carrying the cell indices along (x ascending; y ascending on the
// forward strand, descending from ceil((ref + length) * y_bins / y_max) - 1 on the other), and adds the t-length of
// every part to its cell.  The segment is first clipped to [0, x_max) x [0, y_max) -- the clip points are integers --
// so every part is inside the grid and the walk has at most x_bins + y_bins + 1 parts.  Widths: x_max, y_max <= 2^33
// and unit <= 2^24 keep every product below 2^57.
#include "factor_records.hpp"

#include <cmath>

namespace nolzss {
namespace {

constexpr int kThreads = kRecThreads;
constexpr uint32_t kMaxBins = 4096;                    // per axis of the strand grid: unit <= 2^24
constexpr uint64_t kMaxExtent = 1ull << 33;            // x_max, y_max
constexpr size_t kMaxLengthEdges = 4097;               // staged in LDS (32 KB)
constexpr size_t kMaxPositionEdges = (size_t(1) << 20) + 1;
constexpr size_t kStagedPositionEdges = 2049;          // staged in LDS up to here, searched in global memory above
constexpr size_t kMaxHistCells = size_t(1) << 26;
// LDS a workgroup of these kernels may take: what HIP grants without opting in, and two workgroups per CU of the
// 160 KB.  The default 50 x 50 grid takes 40 KB of it.
constexpr size_t kLdsBudget = 64 * 1024;

struct GridParams {
    uint64_t x_max, y_max;
    uint32_t xb, yb;
};

// One factor per lane, grid-stride.  kLds: both grids (forward cells, then reverse-complement cells) are accumulated
// in a workgroup-private LDS copy and the non-zero cells flushed with one 64-bit global atomic add each; otherwise
// every part goes to global memory directly.  Integer adds: the result does not depend on their order.
template <bool kLds>
__global__ __launch_bounds__(kThreads) void strand_grid_kernel(const Rec *__restrict__ recs, uint64_t z, KeepRule keep,
                                                               GridParams g, unsigned long long *__restrict__ out) {
    extern __shared__ unsigned long long lds_cells[];
    const uint32_t cells = g.xb * g.yb;
    if (kLds) {
        for (uint32_t c = threadIdx.x; c < 2 * cells; c += kThreads) lds_cells[c] = 0;
        __syncthreads();
    }
    unsigned long long *acc = kLds ? lds_cells : out;
    const uint64_t D = cells;
    const uint64_t step_x = g.x_max * g.yb, step_y = g.y_max * g.xb;
    const uint32_t max_parts = g.xb + g.yb + 2;
    const uint64_t stride = (uint64_t)gridDim.x * kThreads;
    for (uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x; i < z; i += stride) {
        const Rec f = recs[i];
        if (!is_kept(keep, i, f.start, f.length)) continue;
        const bool rc = (f.ref & kRcMask) != 0;
        const uint64_t r = f.ref & ~kRcMask;
        uint64_t s = f.start, l = f.length;
        // clip to [0, x_max) x [0, y_max): the tail in x, then the end that leaves the grid in y
        if (s >= g.x_max) continue;
        if (l > g.x_max - s) l = g.x_max - s;
        uint64_t top = 0;  // reverse complement: y just before the first base, ref + length of the whole factor
        if (rc) {
            top = sat_add(r, f.length);
            if (top > g.y_max) {
                const uint64_t c = top - g.y_max;
                if (c >= l) continue;
                s += c;
                l -= c;
                top = g.y_max;
            }
        } else {
            if (r >= g.y_max) continue;
            if (l > g.y_max - r) l = g.y_max - r;
        }
        if (l == 0) continue;
        const uint64_t end = l * D;
        uint32_t xi = (uint32_t)((s * g.xb) / g.x_max);
        uint64_t t_x = (uint64_t)(xi + 1) * step_x - s * D;
        uint32_t yi;
        uint64_t t_y;
        if (rc) {
            yi = (uint32_t)((top * g.yb + g.y_max - 1) / g.y_max) - 1u;
            t_y = top * D - (uint64_t)yi * step_y;
        } else {
            yi = (uint32_t)((r * g.yb) / g.y_max);
            t_y = (uint64_t)(yi + 1) * step_y - r * D;
        }
        unsigned long long *strand = acc + (rc ? cells : 0u);
        uint64_t a = 0;
        for (uint32_t part = 0; a < end && part < max_parts; ++part) {
            uint64_t b = t_x < t_y ? t_x : t_y;
            b = b < end ? b : end;
            if (xi < g.xb && yi < g.yb) atomicAdd(&strand[(size_t)yi * g.xb + xi], (unsigned long long)(b - a));
            if (b == t_x) {
                ++xi;
                t_x += step_x;
            }
            if (b == t_y) {
                yi = rc ? yi - 1u : yi + 1u;  // (wraps below row 0 only at b == end)
                t_y += step_y;
            }
            a = b;
        }
    }
    if (kLds) {
        __syncthreads();
        for (uint32_t c = threadIdx.x; c < 2 * cells; c += kThreads)
            if (lds_cells[c]) atomicAdd(&out[c], lds_cells[c]);
    }
}

struct HistParams {
    const double *len_edges, *pos_edges;
    uint32_t n_le, n_pe;
    uint32_t stage_pos;  // position edges staged in LDS
};

// numpy.histogramdd's bin of v: searchsorted(edges, v, 'right') - 1, v == edges[-1] counted in the last bin
__device__ __forceinline__ bool bin_of(const double *edges, uint32_t n, double v, uint32_t &bin) {
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (edges[mid] <= v) lo = mid + 1;
        else hi = mid;
    }
    if (lo == 0) return false;
    if (lo == n) {
        if (v != edges[n - 1]) return false;
        bin = n - 2;
        return true;
    }
    bin = lo - 1;
    return true;
}

// (length bin, position bin) of every kept factor by binary search of the two edge arrays (staged in LDS).
// kLdsCounts: 32-bit workgroup-private counts in LDS behind the edges (forward cells, then reverse complement),
// flushed as in strand_grid_kernel; otherwise 64-bit global atomics.
template <bool kLdsCounts>
__global__ __launch_bounds__(kThreads) void length_position_hist_kernel(const Rec *__restrict__ recs, uint64_t z,
                                                                        KeepRule keep, HistParams h,
                                                                        unsigned long long *__restrict__ out) {
    extern __shared__ double lds_edges[];
    double *le = lds_edges;
    double *pe = lds_edges + h.n_le;
    const uint32_t staged = h.n_le + (h.stage_pos ? h.n_pe : 0u);
    uint32_t *counts = reinterpret_cast<uint32_t *>(lds_edges + staged);
    const uint32_t nlb = h.n_le - 1, npb = h.n_pe - 1, cells = nlb * npb;
    for (uint32_t k = threadIdx.x; k < h.n_le; k += kThreads) le[k] = h.len_edges[k];
    if (h.stage_pos)
        for (uint32_t k = threadIdx.x; k < h.n_pe; k += kThreads) pe[k] = h.pos_edges[k];
    if (kLdsCounts)
        for (uint32_t c = threadIdx.x; c < 2 * cells; c += kThreads) counts[c] = 0;
    __syncthreads();
    const double *pos = h.stage_pos ? pe : h.pos_edges;
    const uint64_t stride = (uint64_t)gridDim.x * kThreads;
    for (uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x; i < z; i += stride) {
        const Rec f = recs[i];
        if (!is_kept(keep, i, f.start, f.length)) continue;
        uint32_t lb, pb;
        if (!bin_of(le, h.n_le, (double)f.length, lb) || !bin_of(pos, h.n_pe, (double)f.start, pb)) continue;
        const size_t cell = ((f.ref & kRcMask) ? cells : 0u) + (size_t)lb * npb + pb;
        if (kLdsCounts) atomicAdd(&counts[cell], 1u);
        else atomicAdd(&out[cell], 1ull);
    }
    if (kLdsCounts) {
        __syncthreads();
        for (uint32_t c = threadIdx.x; c < 2 * cells; c += kThreads)
            if (counts[c]) atomicAdd(&out[c], (unsigned long long)counts[c]);
    }
}

unsigned grid_of(uint64_t items) { return record_grid(items); }

bool force_global() {  // the form without workgroup-private LDS accumulators, for A/B runs and tests
    const char *e = getenv("NOLZSS_FACTOR_MAPS_GLOBAL");
    return e && *e && *e != '0';
}

size_t records_chunk() {  // records per upload of the records source (tests: a small value)
    const char *e = getenv("NOLZSS_FACTOR_MAPS_CHUNK");
    const long long v = e ? atoll(e) : 0;
    return v > 0 ? (size_t)v : (size_t(1) << 22);
}

std::vector<double> reference_position_edges(uint64_t genome_end, uint32_t min_bins, uint64_t bin_bp) {
    if (genome_end == 0) throw std::invalid_argument("position ladder: genome_end must be positive");
    if (bin_bp == 0) throw std::invalid_argument("position ladder: position_bin_bp must be positive");
    const double q = std::ceil((double)genome_end / (double)bin_bp);
    uint64_t nb = (uint64_t)q;
    if (nb < min_bins) nb = min_bins;
    if (nb == 0) throw std::invalid_argument("position ladder: no bins");
    if (nb + 1 > kMaxPositionEdges) throw std::invalid_argument("position ladder: more than 2^20 bins");
    const double step = (double)genome_end / (double)nb;
    std::vector<double> e(nb + 1);
    for (uint64_t k = 0; k <= nb; ++k) e[k] = (double)k * step;
    e[nb] = (double)genome_end;
    return e;
}

void check_edges(const double *e, size_t n, size_t cap, const char *what) {
    if (n < 2 || n > cap)
        throw std::invalid_argument(std::string(what) + ": between 2 and " + std::to_string(cap) + " edges are supported");
    for (size_t k = 0; k < n; ++k) {
        if (!std::isfinite(e[k])) throw std::invalid_argument(std::string(what) + " must be finite");
        if (k && e[k] < e[k - 1]) throw std::invalid_argument(std::string(what) + " must be ascending");
    }
}

}  // namespace

namespace api {

struct MapsResult {
    uint64_t z = 0;
    MapStats st{0, 0, 0, 0, 0, 0, 0};
    uint64_t x_max = 0, y_max = 0;
    bool want_grid = false, want_hist = false;
    uint32_t xb = 0, yb = 0;
    std::vector<uint64_t> grid;  // forward cells, then reverse complement
    std::vector<double> pos_edges;
    size_t nlb = 0;
    std::vector<uint64_t> hist;  // forward, then reverse complement
};

void check_request(const nolzss_factor_map_request *rq, nolzss_factor_maps *out) {
    if (!out) throw std::invalid_argument("output pointer is null");
    std::memset(out, 0, sizeof *out);
    if (!rq) throw std::invalid_argument("request is null");
    if (rq->x_bins || rq->y_bins) {
        if (rq->x_bins < 1 || rq->y_bins < 1 || rq->x_bins > kMaxBins || rq->y_bins > kMaxBins)
            throw std::invalid_argument("x_bins and y_bins must be between 1 and 4096");
        if (rq->total_length > kMaxExtent) throw std::invalid_argument("total_length beyond 2^33");
    }
    if (rq->n_length_edges) {
        if (!rq->length_edges) throw std::invalid_argument("length_edges is null");
        check_edges(rq->length_edges, rq->n_length_edges, kMaxLengthEdges, "length_edges");
        if (rq->n_position_edges) {
            if (!rq->position_edges) throw std::invalid_argument("position_edges is null");
            check_edges(rq->position_edges, rq->n_position_edges, kMaxPositionEdges, "position_edges");
        } else if (rq->position_bin_bp == 0) {
            throw std::invalid_argument("position ladder: position_bin_bp must be positive");
        }
    }
}

// Bins the records that `each_chunk` delivers into r (already holding z and the request's shape).
// each_chunk(fn): calls fn(device records, count, index of the first) for every chunk, in order; it is run twice
// (statistics, then the maps).
template <typename Chunks>
void bin_records(Context &ctx, const nolzss_factor_map_request &rq, const std::vector<uint64_t> &sentinels,
                 bool by_index, Chunks &&each_chunk, MapsResult &r) {
    hipStream_t s = ctx.stream;
    Arena &arena = ctx.arena;
    ProfScope whole(ctx.profiler(), "factor_maps", s);
    KeepRule keep{rq.min_factor_length, nullptr, (uint32_t)sentinels.size(), by_index ? 1u : 0u, 0};
    if (!sentinels.empty()) {
        uint64_t *d_sent = arena.alloc<uint64_t>(sentinels.size());
        HIP_CHECK(hipMemcpyAsync(d_sent, sentinels.data(), sizeof(uint64_t) * sentinels.size(), hipMemcpyHostToDevice, s));
        keep.sentinels = d_sent;
    }
    MapStats *d_st = arena.alloc<MapStats>(1);
    const MapStats init{0, 0, ~0ull, 0, 0, 0, 0};
    HIP_CHECK(hipMemcpyAsync(d_st, &init, sizeof init, hipMemcpyHostToDevice, s));
    {
        ProfScope ps(ctx.profiler(), "map_stats", s);
        each_chunk([&](const Rec *d, uint64_t count, uint64_t base) {
            KeepRule k = keep;
            k.base_index = base;
            map_stats_kernel<<<grid_of(count), kThreads, 0, s>>>(d, count, k, d_st);
            KERNEL_CHECK();
        });
    }
    HIP_CHECK(hipMemcpyAsync(&r.st, d_st, sizeof r.st, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));  // (init and the sentinel list are locals of the caller's frame)
    const uint64_t kept = r.st.kept_fwd + r.st.kept_rc;
    if (kept == 0) r.st.min_length = 0;

    unsigned long long *d_grid = nullptr, *d_hist = nullptr;
    GridParams gp{0, 0, r.xb, r.yb};
    const size_t cells = (size_t)r.xb * r.yb;
    bool grid_lds = false;
    if (r.want_grid && kept) {
        r.x_max = rq.total_length ? rq.total_length : r.st.x_max;
        r.y_max = rq.total_length ? rq.total_length : r.st.y_max;
        if (r.x_max == 0 || r.y_max == 0) throw std::invalid_argument("Invalid factor coordinates for strand bias grid");
        if (r.x_max > kMaxExtent || r.y_max > kMaxExtent)
            throw std::invalid_argument("factor coordinates beyond 2^33: the strand grid keeps its products in 64 bits");
        gp.x_max = r.x_max;
        gp.y_max = r.y_max;
        d_grid = arena.alloc<unsigned long long>(2 * cells);
        HIP_CHECK(hipMemsetAsync(d_grid, 0, sizeof(uint64_t) * 2 * cells, s));
        grid_lds = !force_global() && 2 * cells * sizeof(uint64_t) <= kLdsBudget;
    }
    HistParams hp{nullptr, nullptr, 0, 0, 0};
    size_t hcells = 0, hist_lds_bytes = 0;
    bool hist_lds = false;
    if (r.want_hist && kept) {
        if (rq.n_position_edges) r.pos_edges.assign(rq.position_edges, rq.position_edges + rq.n_position_edges);
        else if (r.st.max_start > 0)
            r.pos_edges = reference_position_edges(r.st.max_start, rq.position_min_bins, rq.position_bin_bp);
    }
    if (r.want_hist && kept && !r.pos_edges.empty()) {
        hp.n_le = (uint32_t)rq.n_length_edges;
        hp.n_pe = (uint32_t)r.pos_edges.size();
        hcells = (size_t)(hp.n_le - 1) * (hp.n_pe - 1);
        if (hcells > kMaxHistCells) throw std::invalid_argument("space-scale histogram: more than 2^26 cells");
        double *d_le = arena.alloc<double>(hp.n_le), *d_pe = arena.alloc<double>(hp.n_pe);
        HIP_CHECK(hipMemcpyAsync(d_le, rq.length_edges, sizeof(double) * hp.n_le, hipMemcpyHostToDevice, s));
        HIP_CHECK(hipMemcpyAsync(d_pe, r.pos_edges.data(), sizeof(double) * hp.n_pe, hipMemcpyHostToDevice, s));
        hp.len_edges = d_le;
        hp.pos_edges = d_pe;
        hp.stage_pos = hp.n_pe <= kStagedPositionEdges ? 1u : 0u;
        d_hist = arena.alloc<unsigned long long>(2 * hcells);
        HIP_CHECK(hipMemsetAsync(d_hist, 0, sizeof(uint64_t) * 2 * hcells, s));
        const size_t edge_bytes = sizeof(double) * ((size_t)hp.n_le + (hp.stage_pos ? hp.n_pe : 0));
        hist_lds = !force_global() && edge_bytes + 2 * hcells * sizeof(uint32_t) <= kLdsBudget;
        hist_lds_bytes = edge_bytes + (hist_lds ? 2 * hcells * sizeof(uint32_t) : 0);
    }
    if (d_grid || d_hist) {
        each_chunk([&](const Rec *d, uint64_t count, uint64_t base) {
            KeepRule k = keep;
            k.base_index = base;
            if (d_grid) {
                ProfScope ps(ctx.profiler(), "strand_grid", s, 24.0 * (double)count);
                if (grid_lds)
                    strand_grid_kernel<true><<<grid_of(count), kThreads, 2 * cells * sizeof(uint64_t), s>>>(d, count, k, gp,
                                                                                                          d_grid);
                else
                    strand_grid_kernel<false><<<grid_of(count), kThreads, 0, s>>>(d, count, k, gp, d_grid);
                KERNEL_CHECK();
            }
            if (d_hist) {
                ProfScope ps(ctx.profiler(), "length_position_hist", s, 24.0 * (double)count);
                if (hist_lds)
                    length_position_hist_kernel<true><<<grid_of(count), kThreads, hist_lds_bytes, s>>>(d, count, k, hp,
                                                                                                     d_hist);
                else
                    length_position_hist_kernel<false><<<grid_of(count), kThreads, hist_lds_bytes, s>>>(d, count, k, hp,
                                                                                                      d_hist);
                KERNEL_CHECK();
            }
        });
    }
    if (r.want_grid) r.grid.assign(2 * cells, 0);
    if (d_grid) HIP_CHECK(hipMemcpyAsync(r.grid.data(), d_grid, sizeof(uint64_t) * 2 * cells, hipMemcpyDeviceToHost, s));
    if (d_hist) {
        r.nlb = hp.n_le - 1;
        r.hist.resize(2 * hcells);
        HIP_CHECK(hipMemcpyAsync(r.hist.data(), d_hist, sizeof(uint64_t) * 2 * hcells, hipMemcpyDeviceToHost, s));
    }
    HIP_CHECK(hipStreamSynchronize(s));
}

void shape_result(const nolzss_factor_map_request &rq, MapsResult &r) {
    r.want_grid = rq.x_bins != 0;
    r.want_hist = rq.n_length_edges != 0;
    r.xb = rq.x_bins;
    r.yb = rq.y_bins;
    if (r.want_grid) r.grid.assign(2 * (size_t)r.xb * r.yb, 0);
}

// device memory the maps take beside the pipeline (reserve_arena_for's extra)
size_t maps_extra(const nolzss_factor_map_request &rq) {
    size_t b = size_t(1) << 20;
    b += 16 * (size_t)rq.x_bins * rq.y_bins;
    if (rq.n_length_edges) {
        const size_t npe = rq.n_position_edges ? rq.n_position_edges : kMaxPositionEdges;
        const size_t hc = std::min(kMaxHistCells, (rq.n_length_edges - 1) * (npe - 1));
        b += 16 * hc + 8 * (rq.n_length_edges + npe);
    }
    return b;
}

// records left in the arena by a pipeline run: one chunk
void bin_device_records(Context &ctx, const nolzss_factor_map_request &rq, const std::vector<uint64_t> &sentinels,
                        const void *d_recs, MapsResult &r) {
    if (r.z && d_recs) {
        const Rec *d = static_cast<const Rec *>(d_recs);
        bin_records(ctx, rq, sentinels, false, [&](auto &&fn) { fn(d, r.z, 0); }, r);
    }
    ctx.prof.collect();
}

// plain mode over the bytes, rc mode over T s0 rc(T) s1 prepared on the device: text_lengths of significance.hip
// with the records kept (the refusals of nolzss_count_factors / nolzss_count_factors_dna_w_rc)
bool check_text_source(const uint8_t *text, size_t n, bool with_rc) {
    if (n && !text) throw std::invalid_argument("text pointer is null");
    if (with_rc) {
        if (n == 0) return false;  // as dna_w_rc_common
        const size_t m = 2 * n + 2;
        if (m > kMaxText) throw std::invalid_argument("text too long: the device pipeline uses 32-bit indices");
        return rc_guards(m, 0);
    }
    check_text_args(text, n, 0);
    return n != 0;
}

ChainRequest text_records(Context &ctx, const uint8_t *text, size_t n, bool with_rc, size_t extra) {
    const size_t m = with_rc ? 2 * n + 2 : n;
    reserve_arena_for(ctx, m, m + n + extra);
    uint8_t *d_T = ctx.arena.alloc<uint8_t>(n);
    {
        ProfScope ps(ctx.profiler(), "text_h2d", ctx.stream);
        upload_bytes(ctx, d_T, text, n);
    }
    ChainRequest rq;
    rq.records = true;
    if (!with_rc) {
        run_plain(ctx, d_T, n, 0, rq);
        return rq;
    }
    uint8_t *d_S = ctx.arena.alloc<uint8_t>(m);
    const uint32_t bad = prepare_single_rc_on_device(ctx, d_T, (uint32_t)n, d_S);
    if (bad != 0xffffffffu)
        throw std::runtime_error("Invalid nucleotide '" + std::string(1, (char)text[bad]) + "' found in sequence 0");
    run_rc_pipeline(ctx, d_S, m, 0, rq);
    return rq;
}

ChainRequest fasta_records(Context &ctx, const FastaText &ft, bool with_rc, size_t extra,
                           std::vector<uint64_t> &sentinels) {
    const size_t m = ft.S.size();
    sentinels.clear();  // ascending: the byte behind every forward record but the end of the string
    for (const auto &rec : ft.recs)
        if (rec.second < m) sentinels.push_back(rec.second);
    reserve_arena_for(ctx, m, m + extra);
    uint8_t *d_S = ctx.arena.alloc<uint8_t>(m);
    {
        ProfScope ps(ctx.profiler(), "text_h2d", ctx.stream);
        upload_bytes(ctx, d_S, ft.S.data(), m);
    }
    ChainRequest rq;
    rq.records = true;
    if (with_rc) run_rc_pipeline(ctx, d_S, m, 0, rq);
    else run_plain(ctx, d_S, m, 0, rq);
    return rq;
}

void text_maps(const uint8_t *text, size_t n, bool with_rc, int device, const nolzss_factor_map_request &rq,
               MapsResult &r) {
    shape_result(rq, r);
    if (!check_text_source(text, n, with_rc)) return;
    Session ses(device, nullptr);
    Context &ctx = ses.ctx();
    const ChainRequest recs = text_records(ctx, text, n, with_rc, maps_extra(rq));
    r.z = recs.z;
    bin_device_records(ctx, rq, {}, recs.d_records, r);
}

void fasta_maps(const char *path, bool with_rc, bool strict, int device, const nolzss_factor_map_request &rq,
                MapsResult &r) {
    shape_result(rq, r);
    FastaText ft;
    read_fasta_text(path, with_rc, strict, ft);
    if (ft.empty) return;
    std::vector<uint64_t> sentinels;
    Session ses(device, nullptr);
    Context &ctx = ses.ctx();
    const ChainRequest recs = fasta_records(ctx, ft, with_rc, maps_extra(rq), sentinels);
    r.z = recs.z;
    bin_device_records(ctx, rq, sentinels, recs.d_records, r);
}

void records_maps(const nolzss_factor *f, size_t z, const uint64_t *sent_idx, size_t n_sent, int device,
                  const nolzss_factor_map_request &rq, MapsResult &r) {
    shape_result(rq, r);
    if (z && !f) throw std::invalid_argument("factors pointer is null");
    if (n_sent && !sent_idx) throw std::invalid_argument("sentinel_factor_indices is null");
    r.z = z;
    if (z == 0) return;
    std::vector<uint64_t> sentinels(sent_idx, sent_idx + n_sent);
    std::sort(sentinels.begin(), sentinels.end());
    Session ses(device, nullptr);
    Context &ctx = ses.ctx();
    const size_t chunk = std::min(records_chunk(), z);
    reserve_arena_for(ctx, 0, sizeof(Rec) * chunk + 8 * n_sent + maps_extra(rq));
    Rec *d = ctx.arena.alloc<Rec>(chunk);
    bool resident = false;  // a single chunk is uploaded once
    bin_records(ctx, rq, sentinels, true,
                [&](auto &&fn) {
                    for (size_t at = 0; at < z; at += chunk) {
                        const size_t count = std::min(chunk, z - at);
                        if (!resident) {
                            ProfScope ps(ctx.profiler(), "records_h2d", ctx.stream, 24.0 * (double)count);
                            upload_bytes(ctx, d, f + at, sizeof(Rec) * count);
                        }
                        resident = chunk == z;
                        fn(d, count, at);
                    }
                },
                r);
    ctx.prof.collect();
}

template <typename T> T *malloc_copy(const T *src, size_t count) {
    T *p = static_cast<T *>(std::malloc(sizeof(T) * (count ? count : 1)));
    if (!p) throw std::bad_alloc();
    if (count) std::memcpy(p, src, sizeof(T) * count);
    return p;
}

void fill_maps(const MapsResult &r, nolzss_factor_maps *out) {
    try {
        out->z = r.z;
        out->z_used = r.st.kept_fwd + r.st.kept_rc;
        out->kept_forward = r.st.kept_fwd;
        out->kept_rc = r.st.kept_rc;
        out->min_length = r.st.min_length;
        out->max_length = r.st.max_length;
        out->max_start = r.st.max_start;
        if (r.want_grid) {
            const size_t cells = (size_t)r.xb * r.yb;
            out->x_bins = r.xb;
            out->y_bins = r.yb;
            out->unit = cells;
            out->x_max = r.x_max;
            out->y_max = r.y_max;
            out->forward_units = malloc_copy(r.grid.data(), cells);
            out->rc_units = malloc_copy(r.grid.data() + cells, cells);
        }
        if (!r.hist.empty()) {
            const size_t npb = r.pos_edges.size() - 1, hc = r.nlb * npb;
            out->n_length_bins = r.nlb;
            out->n_position_bins = npb;
            out->hist_forward = malloc_copy(r.hist.data(), hc);
            out->hist_rc = malloc_copy(r.hist.data() + hc, hc);
            out->position_edges = malloc_copy(r.pos_edges.data(), npb + 1);
        }
    } catch (...) {
        nolzss_free_factor_maps(out);
        throw;
    }
}

}  // namespace api
}  // namespace nolzss

using namespace nolzss;
using namespace nolzss::api;

extern "C" {

void nolzss_free_factor_maps(nolzss_factor_maps *m) {
    if (!m) return;
    std::free(m->forward_units);
    std::free(m->rc_units);
    std::free(m->hist_forward);
    std::free(m->hist_rc);
    std::free(m->position_edges);
    std::memset(m, 0, sizeof *m);
}

int nolzss_factor_maps_text(const uint8_t *text, size_t n, int with_rc, int device,
                            const nolzss_factor_map_request *request, nolzss_factor_maps *out) {
    return guarded([&] {
        check_request(request, out);
        MapsResult r;
        text_maps(text, n, with_rc != 0, device, *request, r);
        fill_maps(r, out);
    });
}

int nolzss_factor_maps_fasta(const char *path, int with_rc, int sanitize_mode, int device,
                             const nolzss_factor_map_request *request, nolzss_factor_maps *out) {
    return guarded([&] {
        check_request(request, out);
        if (!path) throw std::invalid_argument("path is null");
        check_sanitize_mode(sanitize_mode);
        MapsResult r;
        fasta_maps(path, with_rc != 0, sanitize_mode == 1, device, *request, r);
        fill_maps(r, out);
    });
}

int nolzss_factor_maps_records(const nolzss_factor *factors, size_t z, const uint64_t *sentinel_factor_indices,
                               size_t n_sentinels, int device, const nolzss_factor_map_request *request,
                               nolzss_factor_maps *out) {
    return guarded([&] {
        check_request(request, out);
        MapsResult r;
        records_maps(factors, z, sentinel_factor_indices, n_sentinels, device, *request, r);
        fill_maps(r, out);
    });
}

int nolzss_debug_position_edges(uint64_t genome_end, uint32_t min_bins, uint64_t bin_bp, double **edges, size_t *n) {
    return guarded([&] {
        if (!edges || !n) throw std::invalid_argument("output pointer is null");
        *edges = nullptr;
        *n = 0;
        const std::vector<double> e = reference_position_edges(genome_end, min_bins, bin_bp);
        *edges = malloc_copy(e.data(), e.size());
        *n = e.size();
    });
}

}  // extern "C"
