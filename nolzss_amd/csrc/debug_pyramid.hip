// debug_pyramid.hip -- test hooks for the 16-ary pyramids (pyramid.hpp, pyramid.hip) and the searches built on them
// (nearest.hpp): the caller's arrays go into arena memory whose padding holds a poison byte, the pyramids are built the
// way the pipelines build them, and one lane per query runs the device functions themselves.  No product path calls
// these (part of the C ABI layer of libnolzss_hip.so, include/nolzss_hip.h).
// nolzss_debug_lds_search does the same for the LDS tile searches of nearest_lds.hpp, in the two forms the candidate
// kernels instantiate them (lpnf.hip, rc.hip).
#include "api_internal.hpp"
#include "nearest.hpp"
#include "nearest_lds.hpp"

using namespace nolzss;
using namespace nolzss::api;

namespace {

constexpr int kQueryThreads = 256;
constexpr size_t kSpare = 16;  // poisoned entries behind the last one of an uploaded array

template <bool kMax>
__global__ __launch_bounds__(kQueryThreads) void debug_pyramid_query_kernel(Pyramid P, const uint32_t *__restrict__ q,
                                                                            size_t nq, uint32_t *__restrict__ out) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x; k < nq; k += stride) {
        const uint32_t op = q[3 * k], a = q[3 * k + 1], b = q[3 * k + 2];
        uint32_t res;
        if (op == NOLZSS_PYR_NEAREST_LEFT)
            res = (uint32_t)pyr_nearest_left<kMax>(P, a, b);  // -1 -> 0xffffffff
        else if (op == NOLZSS_PYR_NEAREST_RIGHT)
            res = pyr_nearest_right<kMax>(P, a, b);
        else
            res = pyr_range<kMax>(P, a, b);
        out[k] = res;
    }
}

__global__ __launch_bounds__(kQueryThreads) void debug_nearest_query_kernel(const uint32_t *__restrict__ sa,
                                                                            const uint32_t *__restrict__ lcp, uint32_t n,
                                                                            Pyramid Pmin, Pyramid Pmax, Pyramid Plcp,
                                                                            const uint32_t *__restrict__ q, size_t nq,
                                                                            uint32_t *__restrict__ out) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x; k < nq; k += stride) {
        const uint32_t op = q[5 * k], r = q[5 * k + 1], a = q[5 * k + 2], b = q[5 * k + 3], c = q[5 * k + 4];
        uint32_t o0 = 0, o1 = 0;
        switch (op) {  // the greater-than searches walk the max pyramid (as rc.hip passes it)
        case NOLZSS_NEAR_UP_LESS: nearest_up<false>(sa, lcp, Pmin, Plcp, r, a, b, o0, o1); break;
        case NOLZSS_NEAR_UP_GREATER: nearest_up<true>(sa, lcp, Pmax, Plcp, r, a, b, o0, o1); break;
        case NOLZSS_NEAR_DOWN_LESS: nearest_down<false>(sa, lcp, n, Pmin, Plcp, r, a, b, o0, o1); break;
        case NOLZSS_NEAR_DOWN_GREATER: nearest_down<true>(sa, lcp, n, Pmax, Plcp, r, a, b, o0, o1); break;
        case NOLZSS_NEAR_FAR_UP_LESS: far_up<false>(sa, Pmin, Plcp, r, a, b, o0, o1); break;
        case NOLZSS_NEAR_FAR_UP_GREATER: far_up<true>(sa, Pmax, Plcp, r, a, b, o0, o1); break;
        case NOLZSS_NEAR_FAR_DOWN_LESS: far_down<false>(sa, n, Pmin, Plcp, r, a, b, o0, o1); break;
        case NOLZSS_NEAR_FAR_DOWN_GREATER: far_down<true>(sa, n, Pmax, Plcp, r, a, b, o0, o1); break;
        case NOLZSS_NEAR_LCP_INTERVAL: lcp_interval(Plcp, r, a, o0, o1); break;
        case NOLZSS_NEAR_LPNF_LEFTMOST: o0 = lpnf_leftmost(Pmin, Plcp, r, a); break;
        default: o0 = lpnf_search(Pmin, Plcp, r, a, b, c); break;
        }
        out[2 * k] = o0;
        out[2 * k + 1] = o1;
    }
}

// The searches of one tile as lpf_tile_kernel (kRc = false) and rc_tile_kernel (kRc = true) run them: same staging,
// same block tables, same template arguments and list sizes; every wavefront then writes out what its own ranks found.
template <bool kRc>
__global__ __launch_bounds__(kLdsThreads) void debug_lds_search_kernel(const uint32_t *__restrict__ sa,
                                                                       const uint32_t *__restrict__ lcp, uint32_t n,
                                                                       uint32_t N, uint32_t *__restrict__ out_len,
                                                                       uint32_t *__restrict__ out_pos) {
    constexpr int NS = kRc ? 4 : 2, NP = 2;
    constexpr int kListCap = kRc ? 128 : kLdsPerWave;
    constexpr int kListCapB = 64;
    __shared__ __align__(16) uint32_t s_sa[kLdsSpan];
    __shared__ __align__(16) uint32_t s_lcp[kLdsSpan + 4];
    __shared__ uint32_t s_len[NS * kLdsTile];
    __shared__ uint16_t s_pos[NP * kLdsTile];
    __shared__ uint16_t s_list0[kLdsWaves][NS * kListCap];
    __shared__ uint16_t s_list1[kLdsWaves][NS * kListCapB];
    __shared__ uint32_t s_blk[(kRc ? 4 : 3) * kBlkTableLen];
    const uint32_t base = blockIdx.x * (uint32_t)kLdsTile;
    stage_tile(sa, lcp, n, base, s_sa, s_lcp);
    __syncthreads();
    const BlockTables T = block_tables<kRc>(s_blk);
    build_block_tables<kRc>(s_sa, s_lcp, T);
    __syncthreads();
    const int w = threadIdx.x >> 6;
    const uint32_t far_bit = n <= 0x80000000u ? 0x80000000u : 0u;
    if constexpr (kRc)
        lds_search_wave_blocks<NS, NP, true, kListCap, kListCapB>(s_sa, s_lcp, T, n, base, s_len, s_pos, s_list0[w], s_list1[w],
                                       [N](uint32_t i) { return i < N; }, [N](uint32_t i) { return 2u * N - i; }, far_bit);
    else
        lds_search_wave_blocks<NS, NP, false, kListCap, kListCapB>(s_sa, s_lcp, T, n, base, s_len, s_pos, s_list0[w], s_list1[w],
                                       [](uint32_t) { return true; }, [](uint32_t) { return 0u; }, far_bit);
    for (int row = 0; row < kLdsPerWave / 64; ++row) {
        const int t = w * kLdsPerWave + row * 64 + lane_id();
        const uint64_t rr = (uint64_t)base + t;
        if (rr >= n) continue;
        const bool searched = !kRc || s_sa[t + kLdsReach] < N;
#pragma unroll
        for (int k = 0; k < NS; ++k) {
            out_len[(size_t)k * n + rr] = searched ? s_len[k * kLdsTile + t] : 0u;
            if (k < NP) out_pos[(size_t)k * n + rr] = searched ? match_pos(s_sa, s_pos[k * kLdsTile + t]) : kNoPos;
        }
    }
}

size_t padded_bytes(size_t entries) { return (entries * sizeof(uint32_t) + 255) & ~size_t(255); }

// the level lengths alloc_pyramid will choose for a base array of len entries
int level_lengths(uint32_t len, uint32_t *lens) {
    int nlev = 1;
    lens[0] = len;
    while (lens[nlev - 1] > 1 && nlev < kPyrMaxLevels) {
        lens[nlev] = (lens[nlev - 1] + kPyrFan - 1) >> kPyrShift;
        ++nlev;
    }
    return nlev;
}

// the arena bytes alloc_pyramid takes for the upper levels
size_t upper_level_bytes(uint32_t len) {
    uint32_t lens[kPyrMaxLevels];
    const int nlev = level_lengths(len, lens);
    size_t bytes = 0;
    for (int l = 1; l < nlev; ++l) bytes += padded_bytes(lens[l]);
    return bytes;
}

// h[0 .. len) into a fresh arena array; the kSpare entries behind it and the rest of the allocation hold the poison
uint32_t *upload_poisoned(Context &ctx, const uint32_t *h, size_t len, int poison) {
    uint32_t *d = ctx.arena.alloc<uint32_t>(len + kSpare);
    HIP_CHECK(hipMemsetAsync(d, poison, padded_bytes(len + kSpare), ctx.stream));
    HIP_CHECK(hipMemcpyAsync(d, h, len * sizeof(uint32_t), hipMemcpyHostToDevice, ctx.stream));
    return d;
}

// the arena span the next `bytes` of allocations will occupy, filled with the poison (the level arrays are not cleared
// by anybody: what their padding holds is otherwise what an earlier kernel left there)
void poison_ahead(Context &ctx, size_t bytes, int poison) {
    if (bytes == 0) return;
    const size_t mark = ctx.arena.mark();
    uint8_t *scratch = ctx.arena.alloc<uint8_t>(bytes);
    HIP_CHECK(hipMemsetAsync(scratch, poison, bytes, ctx.stream));
    ctx.arena.rewind(mark);
}

unsigned query_grid(size_t nq) {
    const size_t g = div_up(nq, (size_t)kQueryThreads);
    return (unsigned)(g > 1024 ? 1024 : g);
}

void check_poison(int poison) {
    if (poison != 0x00 && poison != 0xFF) throw std::invalid_argument("poison must be 0x00 or 0xFF");
}

}  // namespace

extern "C" {

int nolzss_debug_pyramid(const uint32_t *base, size_t len, int is_max, int mode, const uint32_t *level1,
                         size_t first_entry, uint32_t flag_min, int poison, const uint32_t *queries, size_t nq,
                         int device, int *nlev, uint32_t *level_lens, uint32_t *levels, size_t levels_cap,
                         uint32_t *flag, uint32_t *results) {
    return guarded([&] {
        if (!base || !nlev || !level_lens) throw std::invalid_argument("null argument");
        if (len == 0) throw std::invalid_argument("the base array is empty");
        if (len >= (size_t(1) << 32)) throw std::invalid_argument("the base array has 2^32 entries or more");
        if (mode != 0 && mode != 1) throw std::invalid_argument("build mode must be 0 or 1");
        check_poison(poison);
        if (nq && (!queries || !results)) throw std::invalid_argument("null query or result array");
        if (flag_min != 0 && (is_max || mode != 0 || !flag || len < 2))  // (the kernel of level 1 sets the flag)
            throw std::invalid_argument("flag_min is for a min pyramid with a level 1, built in mode 0, with a flag word to return");
        uint32_t lens[kPyrMaxLevels];
        const int levels_n = level_lengths((uint32_t)len, lens);
        size_t total = 0;
        for (int l = 0; l < levels_n; ++l) total += lens[l];
        if (levels && levels_cap < total) throw std::invalid_argument("the level buffer is too small");
        if (mode == 1) {
            if (len < 2) throw std::invalid_argument("mode 1 needs a level 1: at least 2 entries");
            if (first_entry > lens[1]) throw std::invalid_argument("first_entry lies beyond level 1");
            if (first_entry && !level1) throw std::invalid_argument("null level-1 array");
        }
        for (size_t k = 0; k < nq; ++k) {
            const uint32_t op = queries[3 * k], a = queries[3 * k + 1], b = queries[3 * k + 2];
            if (op == NOLZSS_PYR_NEAREST_LEFT) {
                if (a >= len) throw std::invalid_argument("nearest_left: r is not below len");
            } else if (op == NOLZSS_PYR_RANGE) {
                if (a > b || b >= len) throw std::invalid_argument("range: needs a <= b < len");
            } else if (op != NOLZSS_PYR_NEAREST_RIGHT) {
                throw std::invalid_argument("unknown pyramid query");
            }
        }

        Session ses(device, nullptr);
        Context &ctx = ses.ctx();
        ctx.arena.reserve(padded_bytes(len + kSpare) + upper_level_bytes((uint32_t)len) + nq * 16 + (size_t(64) << 20));
        const size_t mark = ctx.arena.mark();
        hipStream_t s = ctx.stream;
        uint32_t *d_flag = ctx.arena.alloc<uint32_t>(1);
        HIP_CHECK(hipMemsetAsync(d_flag, 0, sizeof(uint32_t), s));
        uint32_t *d_q = nq ? ctx.arena.alloc<uint32_t>(3 * nq) : nullptr;
        uint32_t *d_res = nq ? ctx.arena.alloc<uint32_t>(nq) : nullptr;
        const uint32_t *d_base = upload_poisoned(ctx, base, len, poison);
        poison_ahead(ctx, upper_level_bytes((uint32_t)len), poison);
        Pyramid P;
        if (mode == 0) {
            P = build_pyramid(d_base, (uint32_t)len, is_max != 0, ctx.arena, s, flag_min, flag_min ? d_flag : nullptr);
        } else {  // the caller wrote level 1 in front of first_entry itself, as the candidate kernels do
            P = alloc_pyramid(d_base, (uint32_t)len, ctx.arena);
            if (first_entry)
                HIP_CHECK(hipMemcpyAsync(const_cast<uint32_t *>(P.lvl[1]), level1, first_entry * sizeof(uint32_t),
                                         hipMemcpyHostToDevice, s));
            fill_pyramid_tail(P, (uint32_t)first_entry, is_max != 0, s);
            fill_pyramid(P, 2, is_max != 0, s);
        }
        if (P.nlev != levels_n) throw std::logic_error("debug_pyramid: level count differs from alloc_pyramid's");
        if (nq) {
            HIP_CHECK(hipMemcpyAsync(d_q, queries, 3 * nq * sizeof(uint32_t), hipMemcpyHostToDevice, s));
            if (is_max)
                debug_pyramid_query_kernel<true><<<query_grid(nq), kQueryThreads, 0, s>>>(P, d_q, nq, d_res);
            else
                debug_pyramid_query_kernel<false><<<query_grid(nq), kQueryThreads, 0, s>>>(P, d_q, nq, d_res);
            KERNEL_CHECK();
            HIP_CHECK(hipMemcpyAsync(results, d_res, nq * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
        }
        *nlev = P.nlev;
        size_t at = 0;
        for (int l = 0; l < P.nlev; ++l) {
            level_lens[l] = P.len[l];
            if (levels) HIP_CHECK(hipMemcpyAsync(levels + at, P.lvl[l], P.len[l] * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
            at += P.len[l];
        }
        if (flag) HIP_CHECK(hipMemcpyAsync(flag, d_flag, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipStreamSynchronize(s));
        ctx.arena.rewind(mark);
    });
}

int nolzss_debug_nearest(const uint32_t *sa, const uint32_t *lcp, size_t n, int poison, const uint32_t *queries,
                         size_t nq, int device, uint32_t *results) {
    return guarded([&] {
        if (!sa || !lcp) throw std::invalid_argument("null argument");
        if (n == 0) throw std::invalid_argument("the arrays are empty");
        if (n + 1 >= (size_t(1) << 32)) throw std::invalid_argument("the LCP array has 2^32 entries or more");
        check_poison(poison);
        if (lcp[0] != 0 || lcp[n] != 0) throw std::invalid_argument("lcp[0] and lcp[n] must be 0");
        if (nq && (!queries || !results)) throw std::invalid_argument("null query or result array");
        for (size_t k = 0; k < nq; ++k) {
            const uint32_t op = queries[5 * k], r = queries[5 * k + 1], a = queries[5 * k + 2];
            if (op > NOLZSS_NEAR_LPNF_SEARCH) throw std::invalid_argument("unknown search");
            if (r >= n) throw std::invalid_argument("search: r is not below n");
            if ((op == NOLZSS_NEAR_LCP_INTERVAL || op == NOLZSS_NEAR_LPNF_LEFTMOST) && a < 1)
                throw std::invalid_argument("lcp_interval / lpnf_leftmost: d must be at least 1");
            if (op == NOLZSS_NEAR_LPNF_SEARCH && a >= n) throw std::invalid_argument("lpnf_search: i is not below n");
        }
        if (nq == 0) return;

        Session ses(device, nullptr);
        Context &ctx = ses.ctx();
        const size_t upper = 2 * upper_level_bytes((uint32_t)n) + upper_level_bytes((uint32_t)n + 1);
        ctx.arena.reserve(padded_bytes(n + kSpare) + padded_bytes(n + 1 + kSpare) + upper + nq * 32 + (size_t(64) << 20));
        const size_t mark = ctx.arena.mark();
        hipStream_t s = ctx.stream;
        uint32_t *d_q = ctx.arena.alloc<uint32_t>(5 * nq);
        uint32_t *d_res = ctx.arena.alloc<uint32_t>(2 * nq);
        const uint32_t *d_sa = upload_poisoned(ctx, sa, n, poison);
        const uint32_t *d_lcp = upload_poisoned(ctx, lcp, n + 1, poison);
        poison_ahead(ctx, upper, poison);
        const Pyramid Pmin = build_pyramid(d_sa, (uint32_t)n, false, ctx.arena, s);
        const Pyramid Pmax = build_pyramid(d_sa, (uint32_t)n, true, ctx.arena, s);
        const Pyramid Plcp = build_pyramid(d_lcp, (uint32_t)n + 1, false, ctx.arena, s);
        HIP_CHECK(hipMemcpyAsync(d_q, queries, 5 * nq * sizeof(uint32_t), hipMemcpyHostToDevice, s));
        debug_nearest_query_kernel<<<query_grid(nq), kQueryThreads, 0, s>>>(d_sa, d_lcp, (uint32_t)n, Pmin, Pmax, Plcp, d_q,
                                                                           nq, d_res);
        KERNEL_CHECK();
        HIP_CHECK(hipMemcpyAsync(results, d_res, 2 * nq * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipStreamSynchronize(s));
        ctx.arena.rewind(mark);
    });
}

int nolzss_debug_lds_search(const uint32_t *sa, const uint32_t *lcp, size_t n, int form, uint32_t strand, int poison,
                            int device, uint32_t *len, uint32_t *pos) {
    return guarded([&] {
        if (!sa || !lcp || !len || !pos) throw std::invalid_argument("null argument");
        if (n == 0) throw std::invalid_argument("the arrays are empty");
        if (n > (size_t(1) << 31) - 2 * kLdsTile) throw std::invalid_argument("more than 2^31 - 2048 ranks");
        if (form != NOLZSS_LDS_PLAIN && form != NOLZSS_LDS_RC) throw std::invalid_argument("unknown form of the LDS searches");
        check_poison(poison);
        if (lcp[0] != 0 || lcp[n] != 0) throw std::invalid_argument("lcp[0] and lcp[n] must be 0");
        const size_t searches = form == NOLZSS_LDS_RC ? 4 : 2;

        Session ses(device, nullptr);
        Context &ctx = ses.ctx();
        ctx.arena.reserve(padded_bytes(n + kSpare) + padded_bytes(n + 1 + kSpare) + (searches + 2) * padded_bytes(n) +
                          (size_t(64) << 20));
        const size_t mark = ctx.arena.mark();
        hipStream_t s = ctx.stream;
        uint32_t *d_len = ctx.arena.alloc<uint32_t>(searches * n);
        uint32_t *d_pos = ctx.arena.alloc<uint32_t>(2 * n);
        const uint32_t *d_sa = upload_poisoned(ctx, sa, n, poison);
        const uint32_t *d_lcp = upload_poisoned(ctx, lcp, n + 1, poison);
        const unsigned tiles = (unsigned)div_up(n, (size_t)kLdsTile);
        if (form == NOLZSS_LDS_RC)
            debug_lds_search_kernel<true><<<tiles, kLdsThreads, 0, s>>>(d_sa, d_lcp, (uint32_t)n, strand, d_len, d_pos);
        else
            debug_lds_search_kernel<false><<<tiles, kLdsThreads, 0, s>>>(d_sa, d_lcp, (uint32_t)n, strand, d_len, d_pos);
        KERNEL_CHECK();
        HIP_CHECK(hipMemcpyAsync(len, d_len, searches * n * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipMemcpyAsync(pos, d_pos, 2 * n * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipStreamSynchronize(s));
        ctx.arena.rewind(mark);
    });
}

}  // extern "C"
