// significance.hip -- factor lengths for the shuffled-control significance analysis ("Factor-length
// histograms and the keyed shuffle"): the length histogram and the lengths in factor order straight from the chain
// (chain_lengths, chain.hip), and the keyed shuffle of the text that gives the control.
//
// Keyed shuffle: out[s + i] = in[s + pi(i)] for every record [s, s + len).  pi is a balanced 4-round Feistel network
// on 2k bits, k = the smallest k >= 1 with 4^k >= len, walked in cycles until it lands inside [0, len):
//   mix64(x)   = splitmix64's finaliser (x ^= x >> 30; x *= 0xbf58476d1ce4e5b9; x ^= x >> 27;
//                x *= 0x94d049bb133111eb; x ^= x >> 31), all arithmetic mod 2^64
//   key        = mix64(seed + 0x9e3779b97f4a7c15 * (record + 1))
//   F_r(x)     = mix64(key ^ ((r + 1) << 32 | x)) & (2^k - 1)            r = 0..3, x < 2^k <= 2^16
//   E(x)       = four rounds of (hi, lo) -> (lo, hi ^ F_r(lo)) on hi = x >> k, lo = x & (2^k - 1); E = hi << k | lo
//   pi(i)      = E(i), then E again while the value is >= len
// Every output index is computed on its own: no sort, no sequential random number generator.
#include "api_internal.hpp"

namespace nolzss {
namespace {

constexpr int kThreads = 256;

__host__ __device__ __forceinline__ uint64_t mix64(uint64_t x) {
    x ^= x >> 30;
    x *= 0xbf58476d1ce4e5b9ull;
    x ^= x >> 27;
    x *= 0x94d049bb133111ebull;
    x ^= x >> 31;
    return x;
}

struct Feistel {
    uint64_t key;
    uint32_t k;     // half width in bits
    uint32_t mask;  // 2^k - 1
    uint32_t len;
};

Feistel make_feistel(uint64_t seed, uint64_t record, uint32_t len) {
    Feistel f;
    f.key = mix64(seed + 0x9e3779b97f4a7c15ull * (record + 1));
    f.k = 1;
    while ((1ull << (2 * f.k)) < len) ++f.k;
    f.mask = (1u << f.k) - 1u;
    f.len = len;
    return f;
}

__device__ __forceinline__ uint32_t feistel_index(const Feistel &f, uint32_t i) {
    uint64_t x = i;
    do {
        uint32_t hi = (uint32_t)(x >> f.k), lo = (uint32_t)x & f.mask;
#pragma unroll
        for (uint32_t r = 0; r < 4; ++r) {
            const uint32_t t = hi ^ ((uint32_t)mix64(f.key ^ (((uint64_t)(r + 1) << 32) | lo)) & f.mask);
            hi = lo;
            lo = t;
        }
        x = ((uint64_t)hi << f.k) | lo;
    } while (x >= f.len);  // cycle walk: the cycle of i < len returns to [0, len)
    return (uint32_t)x;
}

__global__ __launch_bounds__(kThreads) void shuffle_kernel(const uint8_t *__restrict__ in, uint8_t *__restrict__ out,
                                                           Feistel f) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < f.len; i += stride)
        out[i] = in[feistel_index(f, (uint32_t)i)];
}

// S = F $ rc-half of the concatenated form (m = |S|): the reverse-complement half mirrors the bases of the forward
// half, S[m - 2 - i] = complement(S[i]), and keeps its own sentinels
__global__ __launch_bounds__(kThreads) void mirror_rc_half_kernel(uint8_t *__restrict__ S, uint32_t N, uint32_t m) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < N; i += stride) {
        const uint8_t c = S[i];
        uint8_t comp;
        switch (c) {
        case 'A': comp = 'T'; break;
        case 'C': comp = 'G'; break;
        case 'G': comp = 'C'; break;
        case 'T': comp = 'A'; break;
        default: continue;  // a sentinel
        }
        S[m - 2 - i] = comp;
    }
}

unsigned grid_of(size_t items) {
    size_t g = div_up(items, (size_t)kThreads);
    if (g < 1) g = 1;
    return (unsigned)(g > 8192 ? 8192 : g);
}

void shuffle_record(Context &ctx, const uint8_t *d_in, uint8_t *d_out, uint32_t len, uint64_t seed, uint64_t record) {
    if (len == 0) return;
    const Feistel f = make_feistel(seed, record, len);
    shuffle_kernel<<<grid_of(len), kThreads, 0, ctx.stream>>>(d_in, d_out, f);
    KERNEL_CHECK();
}

// the forward records [begin, end) of a concatenated text, shuffled in place (through a copy of the forward half)
void shuffle_records_in_place(Context &ctx, uint8_t *d_S, uint32_t N, const std::vector<std::pair<uint32_t, uint32_t>> &recs,
                              uint64_t seed) {
    ProfScope ps(ctx.profiler(), "shuffle", ctx.stream);
    const size_t mark = ctx.arena.mark();
    uint8_t *copy = ctx.arena.alloc<uint8_t>(N);
    HIP_CHECK(hipMemcpyAsync(copy, d_S, N, hipMemcpyDeviceToDevice, ctx.stream));
    for (size_t r = 0; r < recs.size(); ++r)
        shuffle_record(ctx, copy + recs[r].first, d_S + recs[r].first, recs[r].second - recs[r].first, seed, r);
    HIP_CHECK(hipStreamSynchronize(ctx.stream));  // (the copy is released below)
    ctx.arena.rewind(mark);
}

}  // namespace

namespace api {

// Host copy of what ChainLengthsOut leaves on the device.  The lengths in factor order go straight into a malloc'ed
// block that the C entry point hands to its caller (one host copy of up to 4 GiB, not two).
struct LengthResult {
    std::vector<uint32_t> hist;  // 2 x T
    std::vector<uint64_t> tail;  // sorted
    std::unique_ptr<uint32_t, void (*)(void *)> order{nullptr, &std::free};
    uint64_t z = 0;
};

// runs the pipeline over d_text (plain) or the prepared d_S (rc) with the factor-length outputs
void run_lengths(Context &ctx, const uint8_t *d_text, size_t n, bool rc, bool want_hist, bool want_order,
                 LengthResult &out) {
    hipStream_t s = ctx.stream;
    Arena &arena = ctx.arena;
    const size_t mark = arena.mark();
    const uint32_t chain_n = rc ? (uint32_t)(n / 2 - 1) : (uint32_t)n;
    ChainLengthsOut lo;
    uint32_t *order = nullptr;
    if (want_hist) {
        lo.hist = arena.alloc<uint32_t>(2 * kLengthHistBins + 1);
        lo.tail_count = lo.hist + 2 * kLengthHistBins;
        lo.tail_cap = length_tail_cap(chain_n);
        lo.tail = arena.alloc<uint64_t>(lo.tail_cap);
        HIP_CHECK(hipMemsetAsync(lo.hist, 0, sizeof(uint32_t) * (2 * kLengthHistBins + 1), s));
    }
    if (want_order) lo.order = &order;
    uint32_t z = 0;
    {
        ProfScope ps(ctx.profiler(), "length_pipeline", s);
        ChainRequest rq;
        rq.lengths = &lo;
        if (rc) run_rc_pipeline(ctx, d_text, n, 0, rq);
        else run_plain(ctx, d_text, n, 0, rq);
        z = rq.z;
    }
    out.z = z;
    {  // (closed before collect(): the downloads are timed too)
        ProfScope ps(ctx.profiler(), "lengths_d2h", s);
        if (want_hist) {
            download_bytes(ctx, out.hist.data(), lo.hist, sizeof(uint32_t) * 2 * kLengthHistBins);
            uint32_t tc = 0;
            ctx.read_back(lo.tail_count, &tc, 1);
            if (tc > lo.tail_cap) throw HipError("length histogram: tail list overflow");
            out.tail.resize(tc);
            if (tc) download_bytes(ctx, out.tail.data(), lo.tail, sizeof(uint64_t) * tc);
            std::sort(out.tail.begin(), out.tail.end());
        }
        if (want_order) {
            out.order.reset(static_cast<uint32_t *>(std::malloc(sizeof(uint32_t) * (z ? z : 1))));
            if (!out.order) throw std::bad_alloc();
            if (z) download_bytes(ctx, out.order.get(), order, sizeof(uint32_t) * z);
        }
        HIP_CHECK(hipStreamSynchronize(s));
    }
    ctx.prof.collect();
    arena.rewind(mark);
}

// an empty result (no factors): both histograms zero and, if asked for, an empty order block
void empty_lengths(bool want_order, LengthResult &out) {
    out.hist.assign(2 * kLengthHistBins, 0);
    if (want_order) {
        out.order.reset(static_cast<uint32_t *>(std::malloc(sizeof(uint32_t))));
        if (!out.order) throw std::bad_alloc();
    }
}

// one text: plain mode over the bytes, rc mode over T s0 rc(T) s1 prepared on the device (the refusals of
// nolzss_count_factors_dna_w_rc).  shuffle: the text is shuffled (one record, index 0) before anything else.
void text_lengths(const uint8_t *text, size_t n, bool with_rc, bool shuffle, uint64_t seed, int device, bool want_hist,
                  bool want_order, LengthResult &out) {
    empty_lengths(want_order, out);
    if (n && !text) throw std::invalid_argument("text pointer is null");
    if (with_rc) {
        if (n == 0) return;  // as dna_w_rc_common
        const size_t m = 2 * n + 2;
        if (m > kMaxText) throw std::invalid_argument("text too long: the device pipeline uses 32-bit indices");
        if (!rc_guards(m, 0)) return;
    } else {
        check_text_args(text, n, 0);
        if (n == 0) return;
    }
    Session ses(device, nullptr);
    Context &ctx = ses.ctx();
    const size_t m = with_rc ? 2 * n + 2 : n;
    reserve_arena_for(ctx, m, m + 2 * n + 8 * (size_t)length_tail_cap((uint32_t)n) + 4 * (size_t)kLengthHistBins * 4);
    uint8_t *d_T = ctx.arena.alloc<uint8_t>(n);
    {
        ProfScope ps(ctx.profiler(), "text_h2d", ctx.stream);
        upload_bytes(ctx, d_T, text, n);
    }
    uint8_t *d_S = with_rc ? ctx.arena.alloc<uint8_t>(m) : nullptr;
    if (with_rc) {  // validate the text as given: the refusal names its first invalid byte
        const uint32_t bad = prepare_single_rc_on_device(ctx, d_T, (uint32_t)n, d_S);
        if (bad != 0xffffffffu)
            throw std::runtime_error("Invalid nucleotide '" + std::string(1, (char)text[bad]) + "' found in sequence 0");
    }
    const uint8_t *d_in = d_T;
    if (shuffle) {
        uint8_t *d_shuf = ctx.arena.alloc<uint8_t>(n);
        {
            ProfScope ps(ctx.profiler(), "shuffle", ctx.stream);
            shuffle_record(ctx, d_T, d_shuf, (uint32_t)n, seed, 0);
        }
        d_in = d_shuf;
        if (with_rc) prepare_single_rc_on_device(ctx, d_shuf, (uint32_t)n, d_S);
    }
    run_lengths(ctx, with_rc ? d_S : d_in, m, with_rc, want_hist, want_order, out);
}

// the concatenated multiple-DNA form of nolzss_factorize_fasta_multiple_dna: same reader, sanitizing and limits.
// S = the prepared string; recs = its forward records [begin, end); N = length of the forward half (rc) or m.
// (FastaText: api_internal.hpp)
void read_fasta_text(const char *path, bool with_rc, bool strict, FastaText &ft) {
    FastaParse parse = parse_fasta(path, strict);
    std::vector<const char *> ptrs;
    std::vector<size_t> lens;
    for (const auto &q : parse.sequences) {
        ptrs.push_back(q.data());
        lens.push_back(q.size());
    }
    std::vector<uint64_t> sent;
    size_t orig = 0;
    if (with_rc) {
        prepare_w_rc(ptrs.data(), lens.data(), ptrs.size(), ft.S, orig, sent);  // fasta_processor.cpp:308
        if (ft.S.size() > kMaxText) throw std::invalid_argument("text too long: the device pipeline uses 32-bit indices");
        if (!rc_guards(ft.S.size(), 0)) return;
    } else {
        prepare_no_rc(ptrs.data(), lens.data(), ptrs.size(), ft.S, orig, sent);  // :331
        check_text_args(ft.S.data(), ft.S.size(), 0);
        if (ft.S.size() == 0) return;
    }
    const size_t m = ft.S.size();
    ft.N = with_rc ? (uint32_t)orig : (uint32_t)m;
    // forward records lie between the sentinels of the forward half (no-rc: no sentinel after the last record)
    const size_t k = with_rc ? sent.size() / 2 : sent.size() + 1;
    size_t at = 0;
    for (size_t r = 0; r < k; ++r) {
        const size_t end = r < sent.size() ? (size_t)sent[r] : m;
        ft.recs.emplace_back((uint32_t)at, (uint32_t)end);
        at = end + 1;
    }
    ft.empty = false;
}

// uploads S and, with shuffle, shuffles its forward records on the device; the reverse-complement half is then
// rewritten from the shuffled forward half (= prepare(shuffled records))
uint8_t *upload_fasta_text(Context &ctx, const FastaText &ft, bool with_rc, bool shuffle, uint64_t seed) {
    const size_t m = ft.S.size();
    uint8_t *d_S = ctx.arena.alloc<uint8_t>(m);
    {
        ProfScope ps(ctx.profiler(), "text_h2d", ctx.stream);
        upload_bytes(ctx, d_S, ft.S.data(), m);
    }
    if (shuffle) {
        shuffle_records_in_place(ctx, d_S, ft.N, ft.recs, seed);
        if (with_rc) {
            mirror_rc_half_kernel<<<grid_of(ft.N), kThreads, 0, ctx.stream>>>(d_S, ft.N, (uint32_t)m);
            KERNEL_CHECK();
        }
    }
    return d_S;
}

void fasta_lengths(const char *path, bool with_rc, bool strict, bool shuffle, uint64_t seed, int device, bool want_hist,
                   bool want_order, LengthResult &out) {
    empty_lengths(want_order, out);
    FastaText ft;
    read_fasta_text(path, with_rc, strict, ft);
    if (ft.empty) return;
    const size_t m = ft.S.size();
    Session ses(device, nullptr);
    Context &ctx = ses.ctx();
    reserve_arena_for(ctx, m, 2 * m + 8 * (size_t)length_tail_cap((uint32_t)m) + 4 * (size_t)kLengthHistBins * 4);
    uint8_t *d_S = upload_fasta_text(ctx, ft, with_rc, shuffle, seed);
    run_lengths(ctx, d_S, m, with_rc, want_hist, want_order, out);
}

// the shuffled prepared string itself (tests, control FASTA files)
void fasta_shuffled_text(const char *path, bool with_rc, bool strict, uint64_t seed, int device, HostBytes &S) {
    FastaText ft;
    read_fasta_text(path, with_rc, strict, ft);
    S.clear();
    if (ft.empty) return;
    const size_t m = ft.S.size();
    Session ses(device, nullptr);
    Context &ctx = ses.ctx();
    reserve_arena_for(ctx, 0, 2 * m);  // (no pipeline: the two byte buffers only)
    const uint8_t *d_S = upload_fasta_text(ctx, ft, with_rc, true, seed);
    S.resize(m);
    download_bytes(ctx, S.data(), d_S, m);
    HIP_CHECK(hipStreamSynchronize(ctx.stream));
}

void shuffle_text(const uint8_t *text, size_t n, uint64_t seed, int device, uint8_t *h_out) {
    check_text_args(text, n, 0);
    if (n == 0) return;
    Session ses(device, nullptr);
    Context &ctx = ses.ctx();
    reserve_arena_for(ctx, 0, 2 * n);  // (no pipeline: the two byte buffers only)
    uint8_t *d_in = ctx.arena.alloc<uint8_t>(n);
    uint8_t *d_out = ctx.arena.alloc<uint8_t>(n);
    upload_bytes(ctx, d_in, text, n);
    {
        ProfScope ps(ctx.profiler(), "shuffle", ctx.stream);
        shuffle_record(ctx, d_in, d_out, (uint32_t)n, seed, 0);
    }
    download_bytes(ctx, h_out, d_out, n);
    HIP_CHECK(hipStreamSynchronize(ctx.stream));
    ctx.prof.collect();
}

// LengthResult -> nolzss_length_hist (malloc'ed arrays; the order block, if any, is handed over)
void fill_length_hist(LengthResult &r, nolzss_length_hist *out) {
    const uint32_t T = kLengthHistBins;
    out->threshold = T;
    out->z = r.z;
    out->fwd = static_cast<uint64_t *>(std::calloc(T, sizeof(uint64_t)));
    out->rc = static_cast<uint64_t *>(std::calloc(T, sizeof(uint64_t)));
    const size_t tc = r.tail.size();
    out->tail_count = tc;
    out->tail_lengths = static_cast<uint64_t *>(std::malloc(sizeof(uint64_t) * (tc ? tc : 1)));
    out->tail_rc = static_cast<uint8_t *>(std::malloc(tc ? tc : 1));
    if (!out->fwd || !out->rc || !out->tail_lengths || !out->tail_rc) {
        nolzss_free_length_hist(out);
        throw std::bad_alloc();
    }
    for (uint32_t L = 0; L < T; ++L) {
        out->fwd[L] = r.hist[L];
        out->rc[L] = r.hist[T + L];
    }
    for (size_t j = 0; j < tc; ++j) {
        out->tail_lengths[j] = r.tail[j] & 0xffffffffull;
        out->tail_rc[j] = (uint8_t)(r.tail[j] >> 32);
    }
    if (r.order) {
        out->lengths = r.order.release();
        out->lengths_count = r.z;
    }
}

void check_sanitize_mode(int sanitize_mode) {  // as nolzss_factorize_fasta_multiple_dna
    if (sanitize_mode != 0 && sanitize_mode != 1) throw std::invalid_argument("sanitize_mode must be 0 or 1");
}

void check_hist_out(nolzss_length_hist *out) {
    if (!out) throw std::invalid_argument("output pointer is null");
    std::memset(out, 0, sizeof *out);
}

}  // namespace api
}  // namespace nolzss

using namespace nolzss;
using namespace nolzss::api;

extern "C" {

void nolzss_free_length_hist(nolzss_length_hist *h) {
    if (!h) return;
    std::free(h->fwd);
    std::free(h->rc);
    std::free(h->tail_lengths);
    std::free(h->tail_rc);
    std::free(h->lengths);
    std::memset(h, 0, sizeof *h);
}

int nolzss_factor_length_histogram(const uint8_t *text, size_t n, int with_rc, int shuffle, uint64_t seed, int device,
                                   nolzss_length_hist *out) {
    return guarded([&] {
        check_hist_out(out);
        LengthResult r;
        text_lengths(text, n, with_rc != 0, shuffle != 0, seed, device, true, false, r);
        fill_length_hist(r, out);
    });
}

int nolzss_factor_length_histogram_with_lengths(const uint8_t *text, size_t n, int with_rc, int device,
                                                nolzss_length_hist *out) {
    return guarded([&] {
        check_hist_out(out);
        LengthResult r;
        text_lengths(text, n, with_rc != 0, false, 0, device, true, true, r);
        fill_length_hist(r, out);
    });
}

int nolzss_fasta_factor_length_histogram(const char *path, int with_rc, int sanitize_mode, int shuffle, uint64_t seed,
                                         int device, nolzss_length_hist *out) {
    return guarded([&] {
        check_hist_out(out);
        if (!path) throw std::invalid_argument("path is null");
        check_sanitize_mode(sanitize_mode);
        LengthResult r;
        fasta_lengths(path, with_rc != 0, sanitize_mode == 1, shuffle != 0, seed, device, true, false, r);
        fill_length_hist(r, out);
    });
}

int nolzss_fasta_factor_length_histogram_with_lengths(const char *path, int with_rc, int sanitize_mode, int device,
                                                      nolzss_length_hist *out) {
    return guarded([&] {
        check_hist_out(out);
        if (!path) throw std::invalid_argument("path is null");
        check_sanitize_mode(sanitize_mode);
        LengthResult r;
        fasta_lengths(path, with_rc != 0, sanitize_mode == 1, false, 0, device, true, true, r);
        fill_length_hist(r, out);
    });
}

int nolzss_fasta_shuffled_text(const char *path, int with_rc, int sanitize_mode, uint64_t seed, int device,
                               uint8_t **S_out, size_t *S_len) {
    return guarded([&] {
        if (!S_out || !S_len) throw std::invalid_argument("output pointer is null");
        *S_out = nullptr;
        *S_len = 0;
        if (!path) throw std::invalid_argument("path is null");
        check_sanitize_mode(sanitize_mode);
        HostBytes S;
        fasta_shuffled_text(path, with_rc != 0, sanitize_mode == 1, seed, device, S);
        uint8_t *h = static_cast<uint8_t *>(std::malloc(S.size() ? S.size() : 1));
        if (!h) throw std::bad_alloc();
        if (S.size()) std::memcpy(h, S.data(), S.size());
        *S_out = h;
        *S_len = S.size();
    });
}

int nolzss_factor_lengths(const uint8_t *text, size_t n, int with_rc, int device, uint32_t **out, size_t *z) {
    return guarded([&] {
        if (!out || !z) throw std::invalid_argument("output pointer is null");
        *out = nullptr;
        *z = 0;
        LengthResult r;
        text_lengths(text, n, with_rc != 0, false, 0, device, false, true, r);
        *z = r.z;
        *out = r.order.release();
    });
}

int nolzss_shuffle_dna(const uint8_t *text, size_t n, uint64_t seed, int device, uint8_t **out) {
    return guarded([&] {
        if (!out) throw std::invalid_argument("output pointer is null");
        *out = nullptr;
        uint8_t *h = static_cast<uint8_t *>(std::malloc(n ? n : 1));
        if (!h) throw std::bad_alloc();
        try {
            shuffle_text(text, n, seed, device, h);
        } catch (...) {
            std::free(h);
            throw;
        }
        *out = h;
    });
}

}  // extern "C"
