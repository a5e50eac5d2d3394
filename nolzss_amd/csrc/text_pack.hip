// text_pack.hip -- stage 1 of the pipeline on gfx950: the alphabet of the byte text, its dense codes and the packed
// text (2 / 4 / 8 bits per symbol), with the terminator table of a segmented text (text.hpp).  Entry points: pipeline.hpp.
#include "sa_internal.hpp"

#include <algorithm>

namespace nolzss {

namespace {

// ---------------------------------------------------------------------------------------
// alphabet presence: which byte values occur (256-bit mask, OR-reduced per wavefront)
// ---------------------------------------------------------------------------------------
__device__ __forceinline__ void mark_byte(uint64_t (&m)[4], uint32_t b) {
    const uint64_t bit = 1ull << (b & 63);
    const uint32_t q = b >> 6;
    m[0] |= (q == 0) ? bit : 0;
    m[1] |= (q == 1) ? bit : 0;
    m[2] |= (q == 2) ? bit : 0;
    m[3] |= (q == 3) ? bit : 0;
}

__global__ __launch_bounds__(kThreads) void presence_kernel(const uint8_t *__restrict__ text, size_t n,
                                                            unsigned long long *presence) {
    uint64_t m[4] = {0, 0, 0, 0};
    const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    if (((uintptr_t)text & 15) == 0) {
        const uint4 *v = reinterpret_cast<const uint4 *>(text);
        const size_t nv = n / 16;
        // four loads in flight per thread (a piece past the end reads the last piece again: marking a byte
        // twice changes nothing)
        for (size_t i = tid; i < nv; i += 4 * stride) {
            uint4 x[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const size_t q = i + (size_t)u * stride;
                x[u] = v[q < nv ? q : nv - 1];
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const uint32_t wds[4] = {x[u].x, x[u].y, x[u].z, x[u].w};
#pragma unroll
                for (int k = 0; k < 4; ++k)
#pragma unroll
                    for (int e = 0; e < 4; ++e) mark_byte(m, (wds[k] >> (8 * e)) & 255u);
            }
        }
        for (size_t i = nv * 16 + tid; i < n; i += stride) mark_byte(m, text[i]);
    } else {
        for (size_t i = tid; i < n; i += stride) mark_byte(m, text[i]);
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        uint64_t v = m[k];
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) v |= __shfl_xor(v, d, 64);
        if (lane_id() == 0 && v) atomicOr(&presence[k], (unsigned long long)v);
    }
}

// positions of everything that is not an upper-case nucleotide (at most kMaxTermScan are
// recorded; the count keeps running)
constexpr uint32_t kMaxTermScan = 512;

// kCountOnly: no positions, and ONE atomic per wavefront at the end.  pack_text asks for the count first: a text over
// another alphabet that happens to contain A, C, G and T -- a protein -- has 10^8 bytes that are "not a nucleotide", and
// one returning atomic per such byte on a single counter took 47 ms of the 80 ms of a 2^28-symbol protein text (round 4,
// tools/alphabet_probe.py); the positions are recorded by a second launch only when there are at most 250 of them.
template <bool kCountOnly>
__global__ __launch_bounds__(kThreads) void find_terminators_kernel(const uint8_t *__restrict__ text, uint32_t n,
                                                                    uint32_t *__restrict__ count,
                                                                    uint32_t *__restrict__ pos_out) {
    uint32_t local = 0;
    auto check = [&](uint8_t c, size_t i) {
        if (c != 'A' && c != 'C' && c != 'G' && c != 'T') {
            if (kCountOnly) {
                ++local;
            } else {
                const uint32_t k = atomicAdd(count, 1u);
                if (k < kMaxTermScan) pos_out[k] = (uint32_t)i;
            }
        }
    };
    // 16 bytes per load from the first 16-byte boundary on; a 32-bit word is tested against the four
    // nucleotides at once with exact per-byte equality masks, and only a word that holds something else is
    // looked at byte by byte (1.35 -> 0.35 ms per 2^30-base run of the merged batch)
    const size_t head = (size_t)((16 - (reinterpret_cast<uintptr_t>(text) & 15)) & 15);
    const size_t h = head < n ? head : n;
    const size_t vecs = (n - h) / 16;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (tid < h) check(text[tid], tid);
    const uint4 *v = reinterpret_cast<const uint4 *>(text + h);
    auto all_nucleotides = [](uint32_t w) -> bool {
        // per byte: zero iff the byte equals the pattern; a byte of (x ^ p) is zero <=> haszero
        auto eq = [](uint32_t x, uint32_t p) -> uint32_t {
            const uint32_t y = x ^ p;
            return ~(((y & 0x7f7f7f7fu) + 0x7f7f7f7fu) | y | 0x7f7f7f7fu);  // 0x80 in every byte that matched
        };
        const uint32_t m = eq(w, 0x41414141u) | eq(w, 0x43434343u) | eq(w, 0x47474747u) | eq(w, 0x54545454u);
        return m == 0x80808080u;
    };
    for (size_t k = tid; k < vecs; k += stride) {
        const uint4 q = v[k];
        if (all_nucleotides(q.x) && all_nucleotides(q.y) && all_nucleotides(q.z) && all_nucleotides(q.w)) continue;
        const size_t base = h + k * 16;
        const uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
        for (int j = 0; j < 16; ++j) check((uint8_t)(w[j >> 2] >> (8 * (j & 3))), base + (size_t)j);
    }
    const size_t tail0 = h + vecs * 16;
    if (tail0 + tid < n) check(text[tail0 + tid], tail0 + tid);
    if (kCountOnly) {
        // (saturating: the caller only asks whether the count is one of at most 250, and 2^15 wavefronts x 1024 fits 32 bits)
        local = local < 1024u ? local : 1024u;
        const uint32_t total = wave_reduce(local, OpAdd<uint32_t>());
        if (lane_id() == 0 && total) atomicAdd(count, total < 1024u ? total : 1024u);
    }
}

// ---------------------------------------------------------------------------------------
// packing: one thread per 64-bit output word
// ---------------------------------------------------------------------------------------
template <int BITS>
__global__ __launch_bounds__(kThreads) void pack_kernel(const uint8_t *__restrict__ text, size_t n,
                                                        const unsigned long long *__restrict__ presence,
                                                        uint64_t *__restrict__ words, size_t nwords) {
    constexpr int kSyms = 64 / BITS;
    __shared__ uint8_t lut[256];
    {
        const int b = threadIdx.x;  // kThreads == 256
        int c = 0;
        for (int k = 0; k < (b >> 6); ++k) c += __popcll(presence[k]);
        c += __popcll(presence[b >> 6] & ((1ull << (b & 63)) - 1ull));
        // bytes outside the alphabet (the unique terminators of a segmented text, which may lie above
        // 'T') pack as code 0: their rank would not fit the symbol width and spill into the
        // neighbouring base
        lut[b] = ((presence[b >> 6] >> (b & 63)) & 1ull) ? (uint8_t)c : (uint8_t)0;
    }
    __syncthreads();
    const bool aligned = ((uintptr_t)text & 15) == 0;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t wi = (size_t)blockIdx.x * blockDim.x + threadIdx.x; wi < nwords; wi += stride) {
        const size_t base = wi * kSyms;
        uint64_t acc = 0;
        if (aligned && base + kSyms <= n) {
            if constexpr (kSyms == 8) {
                const uint2 x = *reinterpret_cast<const uint2 *>(text + base);
                const uint32_t wds[2] = {x.x, x.y};
#pragma unroll
                for (int k = 0; k < 2; ++k)
#pragma unroll
                    for (int e = 0; e < 4; ++e) acc = (acc << BITS) | lut[(wds[k] >> (8 * e)) & 255u];
            } else {
#pragma unroll
                for (int c = 0; c < kSyms / 16; ++c) {
                    const uint4 x = *reinterpret_cast<const uint4 *>(text + base + 16 * c);
                    const uint32_t wds[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
                    for (int k = 0; k < 4; ++k)
#pragma unroll
                        for (int e = 0; e < 4; ++e) acc = (acc << BITS) | lut[(wds[k] >> (8 * e)) & 255u];
                }
            }
        } else {
#pragma unroll 4
            for (int e = 0; e < kSyms; ++e) {
                const size_t p = base + e;
                acc = (acc << BITS) | (p < n ? (uint64_t)lut[text[p]] : 0ull);
            }
        }
        words[wi] = acc;
    }
}

// coarse index of a long terminator table (text.hpp): one binary search per 4096-symbol block
__global__ __launch_bounds__(kThreads) void term_coarse_kernel(const uint32_t *__restrict__ pos, uint32_t count,
                                                               uint32_t blocks, uint32_t *__restrict__ coarse) {
    const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= blocks) return;
    const uint64_t p = (uint64_t)b << kTermBlockShift;
    uint32_t lo = 0, hi = count - 1;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if ((uint64_t)pos[mid] >= p)
            hi = mid;
        else
            lo = mid + 1;
    }
    coarse[b] = lo;
}

// terminator table (the given sorted positions and always the end of the text), then the packed words
void finish_packing(Context &ctx, PackedText &t, const uint8_t *d_text, size_t n,
                    const std::vector<uint32_t> &terminators, const unsigned long long *presence) {
    hipStream_t s = ctx.stream;
    std::vector<uint32_t> table = terminators;
    table.push_back((uint32_t)n);
    uint32_t *d_terms = ctx.arena.alloc<uint32_t>(table.size());
    HIP_CHECK(hipMemcpyAsync(d_terms, table.data(), table.size() * sizeof(uint32_t), hipMemcpyHostToDevice, s));
    HIP_CHECK(hipStreamSynchronize(s));  // table is a local vector
    t.terms.pos = d_terms;
    t.terms.count = (uint32_t)table.size();
    t.terms.end = (uint32_t)n;
    if (table.size() <= kTermFew) {  // (a short table travels in the kernel arguments too, text.hpp)
        t.terms.nfew = (uint32_t)table.size();
        for (size_t k = 0; k < table.size(); ++k) t.terms.few[k] = table[k];
    }
    if (table.size() > 256) {
        const uint32_t blocks = (uint32_t)(n >> kTermBlockShift) + 3;
        uint32_t *coarse = ctx.arena.alloc<uint32_t>(blocks);
        term_coarse_kernel<<<(unsigned)div_up(blocks, kThreads), kThreads, 0, s>>>(d_terms, t.terms.count, blocks, coarse);
        KERNEL_CHECK();
        t.terms.coarse = coarse;
    }

    const size_t nwords = div_up(n * (size_t)t.bits, 64) + kRefineWords + 4;  // zero pad: windows read past the end
    uint64_t *words = ctx.arena.alloc<uint64_t>(nwords);
    {
        ProfScope ps(ctx.profiler(), "text_pack", s);
        const unsigned g = grid_for(nwords, kThreads);
        dispatch_bits(t.bits, [&](auto B) { pack_kernel<decltype(B)::value><<<g, kThreads, 0, s>>>(d_text, n, presence, words, nwords); });
        KERNEL_CHECK();
    }
    t.words = words;
}

}  // namespace

PackedText pack_text(Context &ctx, const uint8_t *d_text, size_t n) {
    hipStream_t s = ctx.stream;
    PackedText t;
    t.n = (uint32_t)n;
    unsigned long long *presence = ctx.arena.alloc<unsigned long long>(4);
    HIP_CHECK(hipMemsetAsync(presence, 0, 32, s));
    {
        ProfScope ps(ctx.profiler(), "text_presence", s);
        presence_kernel<<<grid_for(div_up(n, 16), kThreads, 2048), kThreads, 0, s>>>(d_text, n, presence);
        KERNEL_CHECK();
    }
    uint32_t bitsw[8];
    ctx.read_back(reinterpret_cast<const uint32_t *>(presence), bitsw, 8);
    int sigma = 0;
    for (int k = 0; k < 8; ++k) sigma += __builtin_popcount(bitsw[k]);
    t.sigma = sigma;
    t.bits = sigma <= 4 ? 2 : (sigma <= 16 ? 4 : 8);

    // Segmented text?  Upper-case nucleotides plus at most 250 other byte values that occur
    // exactly ONCE each (the shape of the reference's prepared multi-sequence / reverse-
    // complement strings, and of reference + '\\x01' + target): a byte that occurs once can match
    // nothing, so it only terminates matches and the text packs at 2 bits per base.
    std::vector<uint32_t> terminators;
    {
        uint32_t acgt[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        for (unsigned char c : {'A', 'C', 'G', 'T'}) acgt[c >> 5] |= 1u << (c & 31);
        int others = 0, nucleotides = 0;
        for (int k = 0; k < 8; ++k) {
            others += __builtin_popcount(bitsw[k] & ~acgt[k]);
            nucleotides += __builtin_popcount(bitsw[k] & acgt[k]);
        }
        if (others >= 1 && others <= 250 && nucleotides >= 1) {
            uint32_t *count = ctx.arena.alloc<uint32_t>(1);
            uint32_t *pos = ctx.arena.alloc<uint32_t>(kMaxTermScan);
            HIP_CHECK(hipMemsetAsync(count, 0, sizeof(uint32_t), s));
            size_t g = div_up(n, kThreads);
            if (g > 8192) g = 8192;
            find_terminators_kernel<true><<<(unsigned)g, kThreads, 0, s>>>(d_text, (uint32_t)n, count, pos);
            KERNEL_CHECK();
            uint32_t h_count = 0;
            ctx.read_back(count, &h_count, 1);
            if (h_count == (uint32_t)others) {  // every non-nucleotide byte value occurs exactly once
                HIP_CHECK(hipMemsetAsync(count, 0, sizeof(uint32_t), s));
                find_terminators_kernel<false><<<(unsigned)g, kThreads, 0, s>>>(d_text, (uint32_t)n, count, pos);
                KERNEL_CHECK();
                HIP_CHECK(hipStreamSynchronize(s));
                terminators.resize(h_count);
                HIP_CHECK(hipMemcpy(terminators.data(), pos, h_count * sizeof(uint32_t), hipMemcpyDeviceToHost));
                std::sort(terminators.begin(), terminators.end());
                unsigned long long h_presence[4] = {0, 0, 0, 0};
                for (unsigned char c : {'A', 'C', 'G', 'T'}) h_presence[c >> 6] |= 1ull << (c & 63);
                HIP_CHECK(hipMemcpy(presence, h_presence, 32, hipMemcpyHostToDevice));
                t.sigma = 4;
                t.bits = 2;
                t.segmented = true;
            }
        }
    }
    finish_packing(ctx, t, d_text, n, terminators, presence);
    return t;
}

// The merged per-sequence batch: d_text holds upper-case nucleotide records with ONE separator byte
// (any byte that is not a nucleotide) at each of the given sorted positions.  Returns false -- and
// packs nothing -- if the text holds anything else (the caller then takes the records one by one).
bool pack_independent_text(Context &ctx, const uint8_t *d_text, size_t n, const std::vector<uint32_t> &separators,
                           PackedText &t, bool mirror) {
    hipStream_t s = ctx.stream;
    uint32_t *count = ctx.arena.alloc<uint32_t>(1);
    uint32_t *pos = ctx.arena.alloc<uint32_t>(kMaxTermScan);
    HIP_CHECK(hipMemsetAsync(count, 0, sizeof(uint32_t), s));
    size_t g = div_up(n, kThreads);
    if (g > 8192) g = 8192;
    find_terminators_kernel<false><<<(unsigned)g, kThreads, 0, s>>>(d_text, (uint32_t)n, count, pos);
    KERNEL_CHECK();
    uint32_t h_count = 0;
    ctx.read_back(count, &h_count, 1);
    // the separators are not nucleotides, so an equal count means: nothing else is there
    if (h_count != (uint32_t)separators.size()) return false;
    unsigned long long h_presence[4] = {0, 0, 0, 0};
    for (unsigned char c : {'A', 'C', 'G', 'T'}) h_presence[c >> 6] |= 1ull << (c & 63);
    unsigned long long *presence = ctx.arena.alloc<unsigned long long>(4);
    HIP_CHECK(hipMemcpy(presence, h_presence, 32, hipMemcpyHostToDevice));
    t = PackedText{};
    t.n = (uint32_t)n;
    t.sigma = 4;
    t.bits = 2;
    t.segmented = true;
    finish_packing(ctx, t, d_text, n, separators, presence);
    if (!separators.empty()) t.terms.seq_shift = kIndKeyBits;
    t.terms.mirror = mirror ? 1u : 0u;
    return true;
}

}  // namespace nolzss
