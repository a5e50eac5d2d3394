// rlz_cohort.hip -- the kernels of a cohort of samples over the block of a relative-LZ index ("Relative-LZ
// index: cohort"; the entry points: rlz_cohort_api.hip, nolzss_rlz_cohort_*; the rules: include/nolzss_hip.h).
//
// A sample is three bit planes over the block -- ok, lo, hi --, 3 bits per base.  The pack kernels write them: one
// wavefront per word, lane = bit, three ballots.  The pair kernel counts, for every two samples, the positions both call
// and those where the calls differ: XOR / AND / popcount over the planes, a 64 x 64 tile of pairs per workgroup, staged
// through LDS, 4 x 4 pairs per thread in registers.  The site kernels count the bases of every position over the samples;
// the column kernels turn bits back into letters.
//
// No kernel here spins or communicates between workgroups; every loop bound is a count clamped on load to the arrays it
// indexes; the only atomics add integers, so no result depends on their order.
#include "rlz_pileup_device.hpp"

namespace nolzss {
namespace {

constexpr int kThreads = 256;
constexpr uint32_t kWaves = kThreads / 64;
constexpr unsigned kStrideBlocks = 2048;  // workgroups of the word-strided kernels: eight per CU of an MI355X
constexpr uint32_t kChunk = 8;            // words of every staged sample per turn of the pair kernel
constexpr uint32_t kLaunchBlocks = 2048;  // workgroups a launch of the pair kernel is cut into, where the words allow it
constexpr uint32_t kMinSlice = 64;        // words of a slice at the least

// The words a strided grid visits: the wave's first word and the stride, both wave-uniform.
__device__ __forceinline__ uint32_t first_word() {
    return (uint32_t)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * kWaves + (threadIdx.x >> 6)));
}

// One wavefront per word of the sample, lane = bit: the lane's call under the consensus rule, three ballots, the
// statistics as popcounts of four ballots (wave-uniform sums, one atomic per wavefront and statistic at the end: a grid
// of at most kStrideBlocks workgroups, for the reason given at consensus_lengths_kernel).  Lanes at or beyond B and
// separators vote 0.  Loops: the separator search; the five channels; the stride over the words (at most ceil(W / the
// grid's wavefronts) turns).
__global__ __launch_bounds__(kThreads) void cohort_pack_counts_kernel(PileupView v, const uint64_t *__restrict__ xwords,
                                                                      TermTable xt, ConsensusRule rule, uint32_t W,
                                                                      uint64_t *__restrict__ sample,
                                                                      unsigned long long *__restrict__ stats) {
    const uint32_t lane = threadIdx.x & 63u, stride = gridDim.x * kWaves;
    uint32_t st[kCohortStats] = {0, 0, 0, 0};
    for (uint32_t w = first_word(); w < W; w += stride) {
        const uint64_t p64 = (uint64_t)w * 64u + lane;
        bool ok = false, lo = false, hi = false, low = false, del = false, dif = false;
        if (p64 < v.B) {
            const uint32_t p = (uint32_t)p64;
            uint32_t first, ch[kPileupChannels];
            bool separator;
            block_record_of(xt, p, first, separator);
            if (!separator) {
                const uint32_t b = channels_of(v, xwords, false, p, ch);
                uint32_t call;
                uint64_t d;
                low = base_call_of(ch, b, rule, call, d);
                if (!low) {
                    del = call == 4u;
                    ok = call < 4u;
                    lo = ok && (call & 1u);
                    hi = ok && (call & 2u);
                    dif = ok && call != b;
                }
            }
        }
        const uint64_t mok = __ballot(ok), mlo = __ballot(lo), mhi = __ballot(hi);
        const uint64_t mlow = __ballot(low), mdel = __ballot(del), mdif = __ballot(dif);
        if (lane == 0) {
            sample[w] = mok;
            sample[(size_t)W + w] = mlo;
            sample[2 * (size_t)W + w] = mhi;
        }
        st[0] += (uint32_t)__popcll(mok);
        st[1] += (uint32_t)__popcll(mlow);
        st[2] += (uint32_t)__popcll(mdel);
        st[3] += (uint32_t)__popcll(mdif);
    }
    if (lane == 0) {
#pragma unroll
        for (uint32_t k = 0; k < kCohortStats; ++k)
            if (st[k]) atomicAdd(stats + k, (unsigned long long)st[k]);
    }
}

// The same from one byte per position.  Loops: the separator search; the stride over the words.
__global__ __launch_bounds__(kThreads) void cohort_pack_bytes_kernel(const uint8_t *__restrict__ bytes, uint32_t B,
                                                                     const uint64_t *__restrict__ xwords, TermTable xt, uint32_t W,
                                                                     uint64_t *__restrict__ sample,
                                                                     unsigned long long *__restrict__ stats) {
    const uint32_t lane = threadIdx.x & 63u, stride = gridDim.x * kWaves;
    uint32_t st[kCohortStats] = {0, 0, 0, 0};
    for (uint32_t w = first_word(); w < W; w += stride) {
        const uint64_t p64 = (uint64_t)w * 64u + lane;
        bool ok = false, lo = false, hi = false, low = false, dif = false;
        if (p64 < B) {
            const uint32_t p = (uint32_t)p64;
            uint32_t first;
            bool separator;
            block_record_of(xt, p, first, separator);
            if (!separator) {
                const uint32_t c = bytes[p] & 0xdfu;  // (a letter in either case; no other byte becomes one)
                const uint32_t call = c == 'A' ? 0u : c == 'C' ? 1u : c == 'G' ? 2u : c == 'T' ? 3u : 4u;
                ok = call < 4u;
                low = !ok;
                lo = ok && (call & 1u);
                hi = ok && (call & 2u);
                dif = ok && call != base_of(xwords[p >> 5], p);
            }
        }
        const uint64_t mok = __ballot(ok), mlo = __ballot(lo), mhi = __ballot(hi);
        const uint64_t mlow = __ballot(low), mdif = __ballot(dif);
        if (lane == 0) {
            sample[w] = mok;
            sample[(size_t)W + w] = mlo;
            sample[2 * (size_t)W + w] = mhi;
        }
        st[0] += (uint32_t)__popcll(mok);
        st[1] += (uint32_t)__popcll(mlow);
        st[3] += (uint32_t)__popcll(mdif);
    }
    if (lane == 0) {
#pragma unroll
        for (uint32_t k = 0; k < kCohortStats; ++k)
            if (st[k]) atomicAdd(stats + k, (unsigned long long)st[k]);
    }
}

// The pair kernel.  Workgroup (x, y) of a launch owns the tile of the samples [64 ti, 64 ti + 64) x [64 tj, 64 tj + 64),
// tj = ti + x, and the words of slice slice0 + y.  Per turn it stages kChunk words of the three planes of its 128 samples
// in LDS -- sm[side][plane][word][slot], slot = (sample + 2 word) & 63: the rotation spreads the eight words a 16-lane
// group stores over all banks, and a read of one word by consecutive samples stays conflict-free -- and thread (ty, tx)
// counts the pairs (16 a + ty, 16 b + tx), a, b < 4, in 32 registers.  A sample at or beyond N and a word beyond the
// slice are staged as zeros: they count nothing.  Only entries i <= j are written (plain stores when one slice covers
// the words, else atomic adds on the zeroed matrices); cohort_mirror_kernel fills the rest.  Loops: the turns of the
// slice (at most ceil(slice / kChunk), slice <= kCohortMaxSlice); the staging (12 words per thread); the kChunk words
// of a turn, 16 unrolled pairs each.
__global__ __launch_bounds__(kThreads) void cohort_pairs_kernel(const uint64_t *__restrict__ planes, uint32_t N, uint32_t W,
                                                                uint32_t ti, uint32_t slice, uint32_t slice0, int atomic,
                                                                uint32_t *__restrict__ diff, uint32_t *__restrict__ cmp) {
    __shared__ uint64_t sm[2][3][kChunk][kCohortTile];
    const uint32_t tj = ti + blockIdx.x;
    const uint64_t wb = (uint64_t)(slice0 + blockIdx.y) * slice;
    const uint32_t w_begin = wb < W ? (uint32_t)wb : W, w_end = wb + slice < W ? (uint32_t)(wb + slice) : W;
    const uint32_t tx = threadIdx.x & 15u, ty = threadIdx.x >> 4;
    uint32_t c_acc[4][4], d_acc[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) c_acc[a][b] = d_acc[a][b] = 0u;
    for (uint32_t w0 = w_begin; w0 < w_end; w0 += kChunk) {
        __syncthreads();  // (the turn before has been read)
#pragma unroll
        for (uint32_t k = 0; k < 2u * 3u * kCohortTile * kChunk / kThreads; ++k) {
            const uint32_t idx = k * kThreads + threadIdx.x;
            const uint32_t c = idx & (kChunk - 1u), row = idx / kChunk;  // row = (side * 3 + plane) * 64 + sample
            const uint32_t smp = row & (kCohortTile - 1u), pl = (row / kCohortTile) % 3u, side = row / (3u * kCohortTile);
            const uint32_t gs = (side ? tj : ti) * kCohortTile + smp, w = w0 + c;
            uint64_t val = 0;
            if (gs < N && w < w_end) val = planes[(size_t)gs * 3u * W + (size_t)pl * W + w];
            sm[side][pl][c][(smp + 2u * c) & (kCohortTile - 1u)] = val;
        }
        __syncthreads();
#pragma unroll 1  // (unrolled, the 8 x 24 staged words of a turn are all live: 209 registers instead of 137)
        for (uint32_t c = 0; c < kChunk; ++c) {
            uint64_t ro[4], rl[4], rh[4], co[4], cl[4], chi[4];
#pragma unroll
            for (uint32_t a = 0; a < 4u; ++a) {
                const uint32_t r = (a * 16u + ty + 2u * c) & (kCohortTile - 1u), q = (a * 16u + tx + 2u * c) & (kCohortTile - 1u);
                ro[a] = sm[0][0][c][r];
                rl[a] = sm[0][1][c][r];
                rh[a] = sm[0][2][c][r];
                co[a] = sm[1][0][c][q];
                cl[a] = sm[1][1][c][q];
                chi[a] = sm[1][2][c][q];
            }
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int b = 0; b < 4; ++b) {
                    const uint64_t m = ro[a] & co[b];
                    c_acc[a][b] += (uint32_t)__popcll(m);
                    d_acc[a][b] += (uint32_t)__popcll(((rl[a] ^ cl[b]) | (rh[a] ^ chi[b])) & m);
                }
        }
    }
#pragma unroll
    for (uint32_t a = 0; a < 4u; ++a)
#pragma unroll
        for (uint32_t b = 0; b < 4u; ++b) {
            const uint32_t i = ti * kCohortTile + a * 16u + ty, j = tj * kCohortTile + b * 16u + tx;
            if (i >= N || j >= N || i > j) continue;
            const size_t at = (size_t)i * N + j;
            if (atomic) {
                if (c_acc[a][b]) atomicAdd(cmp + at, c_acc[a][b]);
                if (d_acc[a][b]) atomicAdd(diff + at, d_acc[a][b]);
            } else {
                cmp[at] = c_acc[a][b];
                diff[at] = d_acc[a][b];
            }
        }
}

// One lane per entry below the diagonal: the entry mirrored across it.  No loop.
__global__ __launch_bounds__(kThreads) void cohort_mirror_kernel(uint32_t N, uint32_t *__restrict__ diff, uint32_t *__restrict__ cmp) {
    const uint64_t gid = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (gid >= (uint64_t)N * N) return;
    const uint32_t i = (uint32_t)(gid / N), j = (uint32_t)(gid % N);
    if (i <= j) return;
    diff[gid] = diff[(size_t)j * N + i];
    cmp[gid] = cmp[(size_t)j * N + i];
}

// What the samples say at the lane's bit of word w: the samples with a call and those of every base.  The three words
// of a sample are wave-uniform (w is): they come through scalar loads.  Loop: the N samples.
__device__ __forceinline__ void site_counts(const uint64_t *__restrict__ planes, uint32_t N, uint32_t W, uint32_t w, uint32_t lane,
                                            uint32_t &present, uint32_t cnt[4]) {
    present = cnt[0] = cnt[1] = cnt[2] = cnt[3] = 0u;
    for (uint32_t s = 0; s < N; ++s) {
        const uint64_t *__restrict__ sp = planes + (size_t)s * 3u * W + w;
        const uint64_t ok = sp[0], lo = sp[W], hi = sp[2 * (size_t)W];
        const uint32_t o = (uint32_t)(ok >> lane) & 1u, l = (uint32_t)(lo >> lane) & 1u, h = (uint32_t)(hi >> lane) & 1u;
        present += o;
        cnt[0] += o & ~l & ~h;
        cnt[1] += l & ~h;  // (lo and hi are 0 wherever ok is)
        cnt[2] += h & ~l;
        cnt[3] += l & h;
    }
}

__device__ __forceinline__ bool is_site(uint32_t present, const uint32_t cnt[4], uint32_t b, uint32_t min_present, bool with_reference) {
    uint32_t distinct = (cnt[0] ? 1u : 0u) + (cnt[1] ? 1u : 0u) + (cnt[2] ? 1u : 0u) + (cnt[3] ? 1u : 0u);
    if (with_reference && cnt[b] == 0u) ++distinct;
    return distinct >= 2u && present >= min_present;
}

// One wavefront per word, lane = bit: the flag of every position below B.  Loops: the samples; the separator search;
// the stride over the words.
__global__ __launch_bounds__(kThreads) void cohort_site_flags_kernel(const uint64_t *__restrict__ planes, uint32_t N, uint32_t B,
                                                                     uint32_t W, const uint64_t *__restrict__ xwords, TermTable xt,
                                                                     uint32_t min_present, int with_reference,
                                                                     uint32_t *__restrict__ flag) {
    const uint32_t lane = threadIdx.x & 63u, stride = gridDim.x * kWaves;
    for (uint32_t w = first_word(); w < W; w += stride) {
        uint32_t present, cnt[4];
        site_counts(planes, N, W, w, lane, present, cnt);
        const uint64_t p64 = (uint64_t)w * 64u + lane;
        if (p64 >= B) continue;
        const uint32_t p = (uint32_t)p64;
        uint32_t first;
        bool separator;
        block_record_of(xt, p, first, separator);
        flag[p] = (!separator && is_site(present, cnt, base_of(xwords[p >> 5], p), min_present, with_reference != 0)) ? 1u : 0u;
    }
}

// The same walk: a flagged position whose rank falls into [first, first + count) writes its record; a word without one
// is skipped before the samples are read.  Loops: as above.
__global__ __launch_bounds__(kThreads) void cohort_site_records_kernel(const uint64_t *__restrict__ planes, uint32_t N, uint32_t B,
                                                                       uint32_t W, const uint64_t *__restrict__ xwords, TermTable xt,
                                                                       const uint32_t *__restrict__ flag,
                                                                       const uint32_t *__restrict__ off, uint64_t first,
                                                                       uint32_t count, CohortSiteRec *__restrict__ out) {
    const uint32_t lane = threadIdx.x & 63u, stride = gridDim.x * kWaves;
    for (uint32_t w = first_word(); w < W; w += stride) {
        const uint64_t p64 = (uint64_t)w * 64u + lane;
        bool take = false;
        uint64_t at = 0;
        if (p64 < B && flag[p64]) {
            at = off[p64];
            take = at >= first && at < first + count;
        }
        if (!__ballot(take)) continue;
        uint32_t present, cnt[4];
        site_counts(planes, N, W, w, lane, present, cnt);
        if (!take) continue;
        const uint32_t p = (uint32_t)p64;
        uint32_t rec_first;
        bool separator;
        CohortSiteRec r;
        r.record = block_record_of(xt, p, rec_first, separator);
        r.position = p;
        r.record_offset = p - rec_first;
        r.present = present;
        r.counts[0] = cnt[0];
        r.counts[1] = cnt[1];
        r.counts[2] = cnt[2];
        r.counts[3] = cnt[3];
        r.reference = base_of(xwords[p >> 5], p);
        r.pad = 0;
        out[at - first] = r;
    }
}

__device__ __forceinline__ uint8_t letter_of(const uint64_t *__restrict__ sample, uint32_t W, uint32_t p) {
    const uint32_t w = p >> 6, bit = p & 63u;
    if (!((sample[w] >> bit) & 1u)) return (uint8_t)'N';
    return (uint8_t)"ACGT"[((sample[(size_t)W + w] >> bit) & 1u) | (((sample[2 * (size_t)W + w] >> bit) & 1u) << 1)];
}

// One lane per output byte: byte g = s S + k is the letter of sample s at pos[k].  Sample and position are clamped to
// the planes (the entry point has refused a position at or beyond B).  No loop.
__global__ __launch_bounds__(kThreads) void cohort_columns_kernel(const uint64_t *__restrict__ planes, uint32_t N, uint32_t B,
                                                                  uint32_t W, const uint32_t *__restrict__ pos, uint64_t S,
                                                                  uint64_t first, uint32_t count, uint8_t *__restrict__ out) {
    const uint64_t gid = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (gid >= count) return;
    const uint64_t g = first + gid;
    uint64_t s = g / S;
    s = s < N ? s : N - 1u;
    uint32_t p = pos[g % S];
    p = p < B ? p : B - 1u;
    out[gid] = letter_of(planes + (size_t)s * 3u * W, W, p);
}

// One lane per output byte: the letter of position start + gid of one sample.  No loop.
__global__ __launch_bounds__(kThreads) void cohort_calls_kernel(const uint64_t *__restrict__ sample, uint32_t B, uint32_t W,
                                                                uint32_t start, uint32_t count, uint8_t *__restrict__ out) {
    const uint64_t gid = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (gid >= count || start + gid >= B) return;
    out[gid] = letter_of(sample, W, (uint32_t)(start + gid));
}

unsigned grid_for(size_t n) { return (unsigned)div_up(n, (size_t)kThreads); }
unsigned stride_grid(size_t W) {
    const size_t blocks = div_up(W, (size_t)kWaves);
    return (unsigned)(blocks < kStrideBlocks ? blocks : kStrideBlocks);
}

}  // namespace

void rlz_cohort_pack_counts(Context &ctx, const PileupView &v, const PackedText &block, const ConsensusRule &rule,
                            uint64_t *d_sample, unsigned long long *d_stats) {
    HIP_CHECK(hipMemsetAsync(d_stats, 0, kCohortStats * sizeof(unsigned long long), ctx.stream));
    const size_t W = cohort_words(v.B);
    if (W == 0) return;
    ProfScope ps(ctx.profiler(), "rlz_cohort_pack_counts", ctx.stream, 44.0 * (double)v.B);
    cohort_pack_counts_kernel<<<stride_grid(W), kThreads, 0, ctx.stream>>>(v, block.words, block.terms, rule, (uint32_t)W, d_sample,
                                                                          d_stats);
    KERNEL_CHECK();
}

void rlz_cohort_pack_bytes(Context &ctx, const uint8_t *d_bytes, uint32_t B, const PackedText &block, uint64_t *d_sample,
                           unsigned long long *d_stats) {
    HIP_CHECK(hipMemsetAsync(d_stats, 0, kCohortStats * sizeof(unsigned long long), ctx.stream));
    const size_t W = cohort_words(B);
    if (W == 0) return;
    ProfScope ps(ctx.profiler(), "rlz_cohort_pack_bytes", ctx.stream, 1.625 * (double)B);
    cohort_pack_bytes_kernel<<<stride_grid(W), kThreads, 0, ctx.stream>>>(d_bytes, B, block.words, block.terms, (uint32_t)W, d_sample,
                                                                         d_stats);
    KERNEL_CHECK();
}

// Enough slices that one launch -- the `row_tiles` tiles of a row -- still fills the device (kLaunchBlocks workgroups),
// each a multiple of kChunk words and at least kMinSlice of them, so that the atomics of a workgroup stay few beside its
// counting.  (Sized per launch, not per call: the launches of a call run one behind the other, and the last rows of a
// large cohort hold one or two tiles -- profiles/r18_rlz_index_cohort.txt.)
uint32_t rlz_cohort_default_slice(uint32_t row_tiles, size_t W) {
    const size_t want = div_up((size_t)kLaunchBlocks, (size_t)(row_tiles ? row_tiles : 1));
    size_t slice = div_up(div_up(W, want), (size_t)kChunk) * kChunk;
    slice = slice < kMinSlice ? kMinSlice : slice;
    return (uint32_t)(slice < kCohortMaxSlice ? slice : kCohortMaxSlice);
}

void rlz_cohort_pairs(Context &ctx, const uint64_t *d_planes, uint32_t N, uint32_t B, uint32_t slice_knob, uint32_t *d_diff,
                      uint32_t *d_cmp) {
    if (N == 0) return;
    const size_t W = cohort_words(B), cells = (size_t)N * N;
    HIP_CHECK(hipMemsetAsync(d_diff, 0, sizeof(uint32_t) * cells, ctx.stream));
    HIP_CHECK(hipMemsetAsync(d_cmp, 0, sizeof(uint32_t) * cells, ctx.stream));
    if (W == 0) return;
    const uint32_t nt = (uint32_t)div_up((size_t)N, (size_t)kCohortTile);
    ProfScope ps(ctx.profiler(), "rlz_cohort_pairs", ctx.stream, 24.0 * (double)W * (double)N * (double)nt);
    for (uint32_t ti = 0; ti < nt; ++ti) {
        uint32_t slice = slice_knob ? slice_knob : rlz_cohort_default_slice(nt - ti, W);
        slice = slice < kCohortMaxSlice ? slice : kCohortMaxSlice;
        const uint32_t slices = (uint32_t)div_up(W, (size_t)slice);
        const int atomic = slices > 1 ? 1 : 0;
        // a launch: the tiles of one row and as many slices as keep it below kCohortLaunchWordPairs (one at least)
        const uint64_t per_slice = (uint64_t)(nt - ti) * kCohortTile * kCohortTile * (slice < W ? slice : W);
        uint64_t most = kCohortLaunchWordPairs / per_slice;
        most = most < 1 ? 1 : (most < 65535 ? most : 65535);
        for (uint32_t s0 = 0; s0 < slices; s0 += (uint32_t)most) {
            const uint32_t ns = slices - s0 < most ? slices - s0 : (uint32_t)most;
            cohort_pairs_kernel<<<dim3(nt - ti, ns), kThreads, 0, ctx.stream>>>(d_planes, N, (uint32_t)W, ti, slice, s0, atomic, d_diff,
                                                                               d_cmp);
            KERNEL_CHECK();
        }
    }
    cohort_mirror_kernel<<<grid_for(cells), kThreads, 0, ctx.stream>>>(N, d_diff, d_cmp);
    KERNEL_CHECK();
}

void rlz_cohort_site_flags(Context &ctx, const uint64_t *d_planes, uint32_t N, uint32_t B, const PackedText &block,
                           uint32_t min_present, bool with_reference, uint32_t *d_n) {
    const size_t W = cohort_words(B);
    if (W == 0) return;
    ProfScope ps(ctx.profiler(), "rlz_cohort_site_flags", ctx.stream, 0.375 * (double)B * (double)N + 4.0 * (double)B);
    cohort_site_flags_kernel<<<stride_grid(W), kThreads, 0, ctx.stream>>>(d_planes, N, B, (uint32_t)W, block.words, block.terms,
                                                                         min_present, with_reference ? 1 : 0, d_n);
    KERNEL_CHECK();
}

void rlz_cohort_site_records(Context &ctx, const uint64_t *d_planes, uint32_t N, uint32_t B, const PackedText &block,
                             const uint32_t *d_n, const uint32_t *d_off, uint64_t first, uint32_t count, CohortSiteRec *d_out) {
    const size_t W = cohort_words(B);
    if (W == 0 || count == 0) return;
    ProfScope ps(ctx.profiler(), "rlz_cohort_site_records", ctx.stream, 8.0 * (double)B + 48.0 * (double)count);
    cohort_site_records_kernel<<<stride_grid(W), kThreads, 0, ctx.stream>>>(d_planes, N, B, (uint32_t)W, block.words, block.terms, d_n,
                                                                           d_off, first, count, d_out);
    KERNEL_CHECK();
}

void rlz_cohort_columns(Context &ctx, const uint64_t *d_planes, uint32_t N, uint32_t B, const uint32_t *d_pos, uint64_t S,
                        uint64_t first, uint32_t count, uint8_t *d_out) {
    if (N == 0 || B == 0 || S == 0 || count == 0) return;
    ProfScope ps(ctx.profiler(), "rlz_cohort_columns", ctx.stream, 29.0 * (double)count);
    cohort_columns_kernel<<<grid_for(count), kThreads, 0, ctx.stream>>>(d_planes, N, B, (uint32_t)cohort_words(B), d_pos, S, first,
                                                                       count, d_out);
    KERNEL_CHECK();
}

void rlz_cohort_calls(Context &ctx, const uint64_t *d_sample, uint32_t B, uint32_t start, uint32_t count, uint8_t *d_out) {
    if (B == 0 || count == 0) return;
    ProfScope ps(ctx.profiler(), "rlz_cohort_calls", ctx.stream, 1.375 * (double)count);
    cohort_calls_kernel<<<grid_for(count), kThreads, 0, ctx.stream>>>(d_sample, B, (uint32_t)cohort_words(B), start, count, d_out);
    KERNEL_CHECK();
}

}  // namespace nolzss
