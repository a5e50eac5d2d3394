// suffix_array.hip -- suffix-array construction on gfx950: the driver and the prefix-doubling rounds.
//
// Replaces the SA/CSA part of sdsl::construct_im(cst, text, 1) that the reference calls at
// /root/reference/src/cpp/factorizer.cpp:340,381 and factorizer_core.hpp:208.
//
// Method: a key sort, ONE direct-comparison round, then prefix doubling for what is left.
//   round 0   key(i) = first K symbols of suffix i (bit-packed, K = 17 for 2-bit DNA) plus a
//             length tag; the keys are computed inside the first radix pass (radix_sort.hip: one
//             most-significant-digit pass + four bucket-segmented passes on 8-byte records for
//             plain DNA, 5-8 passes on 12-byte records otherwise); the last pass lands in SA.
//   regroup   one single-pass kernel per round (decoupled look-back): group heads, ranks, LCP
//             of every boundary that appeared, compacted list of the suffixes still tied (sa_regroup.hip).
//   direct    every group of <= 64 suffixes is finished by comparing the packed suffixes
//             themselves, 512 bits per step, pair by pair through LDS (group_refine_kernel, sa_direct.hip;
//             the group-sort passes over what it leaves are there too).
//   repeats   long exact repeats and runs of a short period are ordered arithmetically (sa_repeats.hip).
//   round h   only suffixes whose group is not yet a singleton stay active; key = (group head
//             rank, rank[i + h]); small groups sorted by counting, large ones by radix sort.
// All arrays are 32-bit; rank[i] holds (index of the first slot of i's group) + 1, and 0 means
// "past the end of the text", which sorts before every real suffix exactly as the reference's
// appended terminator does.
// The state of one construction (SaBuild) and the functions of the other files: sa_internal.hpp.
#include "sa_internal.hpp"

#include "pyramid.hpp"
#include "scan.hpp"

#include <algorithm>
#include <cstdlib>

namespace nolzss {

namespace {

// secondary key of a doubling round: rank of the suffix h symbols further on (0 past the end)
__global__ __launch_bounds__(kThreads) void round_keys_kernel(const uint32_t *__restrict__ act_slot,
                                                              uint32_t m, const uint32_t *__restrict__ sa,
                                                              const uint32_t *__restrict__ rank, uint32_t n,
                                                              uint32_t h, uint32_t *__restrict__ lo,
                                                              uint32_t *__restrict__ vals) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t a = (size_t)blockIdx.x * blockDim.x + threadIdx.x; a < m; a += stride) {
        const uint32_t i = sa[act_slot[a]];
        lo[a] = (n - i > h) ? rank[i + h] : 0u;  // i + h < n without overflow
        vals[a] = i;
    }
}

// Segmented sort of the active list by lo inside each group.  Groups are contiguous in the
// list and (for real sequence data) almost all tiny, so each element finds its place by
// counting the smaller members of its own group -- one pass, no radix passes.  Members of
// groups larger than kSmallGroup are flagged for the radix fallback instead.

__global__ __launch_bounds__(kThreads) void small_sort_kernel(const uint32_t *__restrict__ act_slot,
                                                              const uint32_t *__restrict__ act_grp,
                                                              const uint32_t *__restrict__ lo,
                                                              const uint32_t *__restrict__ vals, uint32_t m,
                                                              uint32_t *__restrict__ out_lo,
                                                              uint32_t *__restrict__ out_vals,
                                                              uint32_t *__restrict__ large_flag) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t a = (size_t)blockIdx.x * blockDim.x + threadIdx.x; a < m; a += stride) {
        const uint32_t g = act_grp[a];
        const size_t g0 = a - (act_slot[a] - g);  // list index of the group's first member
        const uint32_t mine = lo[a];
        uint32_t below = 0, cnt = 0;
        // a member of a large group sees that in one look (the group's members are contiguous in the list):
        // on periodic texts every suffix sits in one of a few huge groups for twenty rounds, and counting
        // to kSmallGroup + 1 from the group's head in every round cost as much as the radix sort beside it
        bool large = g0 + kSmallGroup < m && act_grp[g0 + kSmallGroup] == g;
        for (size_t b = g0; !large && b < m; ++b) {
            if (act_grp[b] != g) break;
            if (++cnt > kSmallGroup) {
                large = true;
                break;
            }
            const uint32_t l = lo[b];
            below += (l < mine || (l == mine && b < a)) ? 1u : 0u;
        }
        large_flag[a] = large ? 1u : 0u;
        if (!large) {
            out_lo[g0 + below] = mine;
            out_vals[g0 + below] = vals[a];
        }
    }
}

// The same for groups of kSmallGroup + 1 .. kMidGroup members (collections of many similar genomes tie in groups
// as large as the collection): one workgroup per tile of kMidGroup list positions takes the groups that START in
// its tile; the keys of the tile and of the kMidGroup positions behind it sit in LDS, and every member counts the
// smaller members of its group there (the members of a group read the same entries: broadcasts).  Those groups went
// through the global radix sort beside the truly large ones: 30 ms per doubling round on 96 genomes of 2^28 bases
// in all, six times what the small groups of 24 genomes cost.  handled += members taken (one atomic per workgroup).
constexpr uint32_t kMidGroup = 1024;
constexpr int kMidThreads = 256;
__global__ __launch_bounds__(kMidThreads) void mid_sort_kernel(const uint32_t *__restrict__ act_slot,
                                                               const uint32_t *__restrict__ act_grp,
                                                               const uint32_t *__restrict__ lo,
                                                               const uint32_t *__restrict__ vals, uint32_t m,
                                                               uint32_t *__restrict__ out_lo,
                                                               uint32_t *__restrict__ out_vals,
                                                               uint32_t *__restrict__ large_flag,
                                                               uint32_t *__restrict__ handled) {
    __shared__ uint32_t s_lo[2 * kMidGroup];
    __shared__ uint32_t s_size[kMidGroup];  // members of the group that starts at this tile position (0: none)
    __shared__ uint32_t s_taken;
    const uint32_t base = blockIdx.x * kMidGroup;
    const uint32_t span = m - base < 2 * kMidGroup ? m - base : 2 * kMidGroup;
    for (uint32_t e = threadIdx.x; e < kMidGroup; e += kMidThreads) s_size[e] = 0;
    if (threadIdx.x == 0) s_taken = 0;
    __syncthreads();
    // group sizes first: a tile in which no group of the kernel's size class starts has nothing to do and leaves before it
    // reads a key (a text whose suffixes all sit in a few huge groups -- a Fibonacci word -- ran this kernel for twenty
    // rounds at 4.8 ms each)
    bool any = false;
    for (uint32_t e = threadIdx.x; e < span; e += kMidThreads) {
        const uint32_t a = base + e, g = act_grp[a], j = act_slot[a] - g;
        if ((a + 1 == m || act_grp[a + 1] != g) && j <= e && e - j < kMidGroup) {  // the last member
            s_size[e - j] = j + 1;
            any |= j + 1 > kSmallGroup && j + 1 <= kMidGroup;
        }
    }
    if (__syncthreads_or(any) == 0) return;
    for (uint32_t e = threadIdx.x; e < span; e += kMidThreads) s_lo[e] = lo[base + e];
    __syncthreads();
    uint32_t taken = 0;
    for (uint32_t e = threadIdx.x; e < span; e += kMidThreads) {
        const uint32_t a = base + e, j = act_slot[a] - act_grp[a];
        if (j > e || e - j >= kMidGroup) continue;  // my group starts in a tile in front of this one
        const uint32_t g0 = e - j, gs = s_size[g0];
        if (gs <= kSmallGroup || gs > kMidGroup) continue;  // (0: the group ends beyond the span, i.e. is larger)
        const uint32_t mine = s_lo[e];
        uint32_t below = 0;
        for (uint32_t b = g0; b < g0 + gs; ++b) {
            const uint32_t l = s_lo[b];
            below += (l < mine || (l == mine && b < e)) ? 1u : 0u;
        }
        out_lo[base + g0 + below] = mine;
        out_vals[base + g0 + below] = vals[a];
        large_flag[a] = 0;
        ++taken;
    }
    taken = wave_reduce(taken, OpAdd<uint32_t>());
    if (lane_id() == 0 && taken) atomicAdd(&s_taken, taken);
    __syncthreads();
    if (threadIdx.x == 0 && s_taken) atomicAdd(handled, s_taken);
}

__global__ __launch_bounds__(kThreads) void gather_large_kernel(const uint32_t *__restrict__ large_flag,
                                                                const uint32_t *__restrict__ idx,
                                                                const uint32_t *__restrict__ act_grp,
                                                                const uint32_t *__restrict__ lo,
                                                                const uint32_t *__restrict__ vals, uint32_t m,
                                                                uint64_t *__restrict__ lkeys,
                                                                uint32_t *__restrict__ lvals,
                                                                uint32_t *__restrict__ lidx) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t a = (size_t)blockIdx.x * blockDim.x + threadIdx.x; a < m; a += stride)
        if (large_flag[a]) {
            const uint32_t k = idx[a];
            lkeys[k] = ((uint64_t)act_grp[a] << 32) | lo[a];
            lvals[k] = vals[a];
            lidx[k] = (uint32_t)a;
        }
}

// The same for the segmented sort of the large groups (radix_sort_segments_u32): 32-bit keys, the group of every
// gathered element beside them; then the first gathered element of every group (heads -> scan -> starts).
__global__ __launch_bounds__(kThreads) void gather_large32_kernel(const uint32_t *__restrict__ large_flag,
                                                                  const uint32_t *__restrict__ idx,
                                                                  const uint32_t *__restrict__ act_grp,
                                                                  const uint32_t *__restrict__ lo,
                                                                  const uint32_t *__restrict__ vals, uint32_t m,
                                                                  uint32_t *__restrict__ lkeys, uint32_t *__restrict__ lvals,
                                                                  uint32_t *__restrict__ lidx, uint32_t *__restrict__ lgrp) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t a = (size_t)blockIdx.x * blockDim.x + threadIdx.x; a < m; a += stride)
        if (large_flag[a]) {
            const uint32_t k = idx[a];
            lkeys[k] = lo[a];
            lvals[k] = vals[a];
            lidx[k] = (uint32_t)a;
            lgrp[k] = act_grp[a];
        }
}
__global__ __launch_bounds__(kThreads) void large_heads_kernel(const uint32_t *__restrict__ lgrp, uint32_t count,
                                                               uint32_t *__restrict__ head) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x; k < count; k += stride)
        head[k] = (k == 0 || lgrp[k] != lgrp[k - 1]) ? 1u : 0u;
}
__global__ __launch_bounds__(kThreads) void large_starts_kernel(const uint32_t *__restrict__ head,
                                                                const uint32_t *__restrict__ pos, uint32_t count,
                                                                uint32_t *__restrict__ starts) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x; k < count; k += stride)
        if (head[k]) starts[pos[k]] = (uint32_t)k;
}
__global__ __launch_bounds__(kThreads) void scatter_large32_kernel(const uint32_t *__restrict__ lkeys,
                                                                   const uint32_t *__restrict__ lvals,
                                                                   const uint32_t *__restrict__ lidx, uint32_t count,
                                                                   uint32_t *__restrict__ out_lo,
                                                                   uint32_t *__restrict__ out_vals) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x; k < count; k += stride) {
        const uint32_t a = lidx[k];
        out_lo[a] = lkeys[k];
        out_vals[a] = lvals[k];
    }
}

// the k-th smallest large element goes to the k-th list position owned by a large group
__global__ __launch_bounds__(kThreads) void scatter_large_kernel(const uint64_t *__restrict__ lkeys,
                                                                 const uint32_t *__restrict__ lvals,
                                                                 const uint32_t *__restrict__ lidx, uint32_t count,
                                                                 uint32_t *__restrict__ out_lo,
                                                                 uint32_t *__restrict__ out_vals,
                                                                 uint32_t *__restrict__ lcp_list, uint32_t lcp_code) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x; k < count; k += stride) {
        const uint32_t a = lidx[k];
        out_lo[a] = (uint32_t)lkeys[k];
        out_vals[a] = lvals[k];
        if (lcp_list) lcp_list[a] = lcp_code;
    }
}

}  // namespace

SaKnobs::SaKnobs() {
    auto set = [](const char *name) { return getenv(name) != nullptr; };
    auto u32 = [](const char *name, uint32_t dflt) { return getenv(name) ? (uint32_t)atoi(getenv(name)) : dflt; };
    auto i64 = [](const char *name, long long dflt) { return getenv(name) ? atoll(getenv(name)) : dflt; };
    trace = set("NOLZSS_TRACE");
    dna_fast_min = (uint32_t)i64("NOLZSS_DNA_FAST_MIN", 1ll << 20);
    no_key16 = set("NOLZSS_NO_KEY16");
    no_defer = set("NOLZSS_NO_DEFER_ISA");
    fused_sort = u32("NOLZSS_FUSED_SORT", 0u) != 0;
    regroup_phases = set("NOLZSS_REGROUP_PHASES");
    refine_words = u32("NOLZSS_REFINE_WORDS", 32u);
    refine_phases = set("NOLZSS_REFINE_PHASES");
    group_sort_phases = set("NOLZSS_GROUP_SORT_PHASES");
    no_stragglers = set("NOLZSS_NO_STRAGGLERS");
    no_direct2 = set("NOLZSS_NO_DIRECT2");
    direct2_div = u32("NOLZSS_DIRECT2_MAX", 64u);
    no_equalise = set("NOLZSS_NO_EQUALISE");
    pivot_min = i64("NOLZSS_PIVOT_MIN", -1);
    no_pivot = set("NOLZSS_NO_PIVOT");
    pivot_depth = u32("NOLZSS_PIVOT_DEPTH", 2048u);
    pivot_passes = (int)u32("NOLZSS_PIVOT_PASSES", 3u);
    pair_runs_min = i64("NOLZSS_PAIR_RUNS_MIN", -1);
    no_periodic = set("NOLZSS_NO_PERIODIC");
    runs_avg4 = u32("NOLZSS_PAIR_RUNS_AVG4", 10u);
    no_mid_sort = set("NOLZSS_NO_MID_SORT");
    no_seg_large = set("NOLZSS_NO_SEG_LARGE");
    inject_pending = set("NOLZSS_TEST_INJECT_PENDING");
}

const SaKnobs &sa_knobs() {
    static const SaKnobs knobs;
    return knobs;
}

namespace {

// Which key sort a text takes, and everything that follows from the choice.
// 2-bit texts, segmented or not, sort on the plain 40-bit key [17 bases][6-bit tag]: suffixes that
// meet a terminator inside the key window and tie on the key are already in their final order
// after the (stable) sort -- ascending start = ascending terminator -- and the regroup kernel
// makes each of them a group of its own.
KeyPlan plan_keys(const PackedText &text) {
    const SaKnobs &knobs = sa_knobs();
    const uint32_t n = text.n;
    KeyPlan p;
    // independent sequences (merged batch): the number of the sequence sits above the plain 40-bit key
    const bool independent = text.terms.seq_shift != 0;
    if (independent) {
        if (text.bits != 2 || text.terms.seq_shift != (uint32_t)kIndKeyBits) throw HipError("suffix array: independent sequences need the 2-bit key layout");
        while (p.seq_bits < 24 && (1u << p.seq_bits) < text.terms.count) ++p.seq_bits;
        if ((1u << p.seq_bits) < text.terms.count) throw HipError("suffix array: too many independent sequences");
    }
    const bool dna_fast = text.bits == 2 && n >= knobs.dna_fast_min && !independent;
    // plain one-segment DNA: the 16-base key whose tag is not sorted (text.hpp, kP16Syms) -- one radix pass less
    // (segmented texts with a short terminator table take it too: the reverse-complement string of one sequence)
    const bool key16 = dna_fast && !knobs.no_key16 && key16_applicable(text);
    // independent LONG records (text.hpp, kRecSyms): the records are the buckets of the segmented sort
    const bool rec_fast = independent && !text.terms.mirror && n >= knobs.dna_fast_min && sort_knobs().rec_bucket_min > 0 &&
                          (uint64_t)text.terms.count * sort_knobs().rec_bucket_min <= (uint64_t)n;
    const bool fused = key16 && knobs.fused_sort && !text.segmented;
    // ... and the 35-bit key where that sort ranks its low digits in LDS (radix_sort.hpp: key35_applicable)
    const bool key35 = key16 && !fused && key35_applicable(text);
    p.choice = fused ? KeyPlan::kFused : key35 ? KeyPlan::kKey35 : key16 ? KeyPlan::kKey16 : dna_fast ? KeyPlan::kDnaFast : rec_fast ? KeyPlan::kRecFast
               : independent ? KeyPlan::kIndependent : text.segmented ? KeyPlan::kSegmented : KeyPlan::kGeneral;
    switch (p.choice) {
    case KeyPlan::kFused:
    case KeyPlan::kKey16:  // bucket = first four bases, stored word [24 key bits][8-bit tag]
        p.k_syms = kP16Syms, p.tag_bits = kP16TagBits, p.key_bits = kP16Syms * 2;
        break;
    case KeyPlan::kKey35:  // bucket = first four bases, stored word [27 key bits][5-bit tag]: 17 1/2 bases
        p.k_syms = kP35Syms, p.tag_bits = kP35TagBits, p.key_bits = kP35KeyBits;
        break;
    case KeyPlan::kRecFast:  // bucket = record, [kRecSyms bases][4-bit tag]
        p.k_syms = kRecSyms, p.tag_bits = kRecTagBits, p.key_bits = kRecSyms * 2 + kRecTagBits;
        break;
    case KeyPlan::kIndependent:  // [record][kIndSyms bases][4-bit tag]
        p.k_syms = kIndSyms, p.tag_bits = kIndTagBits, p.key_bits = kIndKeyBits + p.seq_bits;
        break;
    case KeyPlan::kSegmented:  // [kSegSyms symbols][5-bit tag][8-bit terminator index]
        p.k_syms = kSegSyms, p.tag_bits = kSegTagBits, p.low_bits = kSegTermBits, p.key_bits = kSegSyms * 2 + kSegTagBits + kSegTermBits;
        break;
    case KeyPlan::kDnaFast:
    case KeyPlan::kGeneral:  // [kSyms symbols][tag]
        dispatch_bits(text.bits, [&](auto B) {
            using L = KeyLayout<decltype(B)::value>;
            p.k_syms = L::kSyms, p.tag_bits = L::kTagBits, p.key_bits = L::kSyms * decltype(B)::value + L::kTagBits;
        });
        break;
    }
    p.key_passes = std::min(8, (p.key_bits + kRadixBits - 1) / kRadixBits);
    if (p.choice == KeyPlan::kKey35) p.key_passes = 4;  // (as kKey16: the two digits ranked in LDS are wider, not more)
    // (the bucketed sorts name the buffer their keys end in, radix_sort.hpp; the general sort alternates)
    p.cur = p.choice == KeyPlan::kDnaFast ? 1 : p.choice <= KeyPlan::kRecFast ? 0 : (p.key_passes & 1);
    p.bucketed = dna_fast || rec_fast;
    // (mirrored independent sequences have two terminators each: a short suffix can tie with its copy at the other one)
    p.short_tag = (dna_fast || (independent && text.terms.mirror)) ? (uint32_t)p.k_syms : 0u;
    p.seq_shift = rec_fast ? 32u : text.terms.seq_shift;
    return p;
}

// ---- round 0: order by the first K symbols, then the first regroup ----------------------------------------------
// (the keys are never materialised in text order: the first radix pass computes them from the
// packed text, radix_sort_initial_keys)
void key_sort_round0(SaBuild &b, const KeyPlan &plan) {
    Context &ctx = b.ctx;
    const PackedText &text = b.text;
    hipStream_t s = ctx.stream;
    Arena &arena = ctx.arena;
    const uint32_t n = b.n;
    uint32_t *seg_mem = arena.alloc<uint32_t>((size_t)kSegDescWords *
                                              (div_up(n, kSortTile) + (plan.rec_fast() ? (size_t)text.terms.count + 1 : (size_t)257)));  // 16-byte aligned
    const size_t sort_mark = arena.mark();
    // the bucketed sort of plain DNA works on 8-byte (u32 key, u32 suffix) records: two 4n-byte key buffers;
    // the general sort on 12-byte records: two 8n-byte key buffers
    const bool fused = plan.choice == KeyPlan::kFused;
    uint64_t *keys[2];
    if (plan.bucketed && !fused) {
        uint32_t *k32 = arena.alloc<uint32_t>(2 * (size_t)n + 4);
        keys[0] = reinterpret_cast<uint64_t *>(k32);
        keys[1] = reinterpret_cast<uint64_t *>(k32 + (((size_t)n + 1) & ~size_t(1)));
    } else {
        keys[0] = arena.alloc<uint64_t>(n);
        keys[1] = arena.alloc<uint64_t>(n);
    }
    uint32_t *keys32[2] = {reinterpret_cast<uint32_t *>(keys[0]), reinterpret_cast<uint32_t *>(keys[1])};
    // The value buffers of the key sort: the one the last pass lands in IS sa (no copy afterwards).
    uint32_t *vals_other = fused ? nullptr : arena.alloc<uint32_t>(n);
    uint32_t *vals[2] = {vals_other, vals_other};
    vals[plan.key_passes & 1] = b.sa;
    SegView seg;
    Round0Regroup round0;
    int cur = plan.cur;
    {
        ProfScope ps(ctx.profiler(), "sa_sort_initial", s);
        switch (plan.choice) {
        case KeyPlan::kFused:
            radix_sort_dna_keys16_fused(text, keys, b.sa, seg_mem, seg, arena, s, ctx.profiler());
            break;
        case KeyPlan::kKey16:
        case KeyPlan::kKey35:
            // (where the sort finishes its sub-buckets in LDS it does the regroup of round 0 on the way, if nobody needs
            // the ranks it would store: the sorted keys are then never written)
            round0.lcp = b.lcp;
            round0.new_slot = b.next_slot();
            round0.new_grp = b.next_grp();
            round0.d_total = b.d_total;
            radix_sort_dna_keys16(text, keys32, vals, seg_mem, seg, arena, s, ctx.profiler(), b.store_ranks ? nullptr : &round0,
                                  plan.choice == KeyPlan::kKey35);
            break;
        case KeyPlan::kDnaFast:
            // plain DNA: partition by the first four bases, then sort the buckets on 8-byte records
            radix_sort_dna_keys(text, keys32, vals, seg_mem, seg, arena, s, ctx.profiler());
            break;
        case KeyPlan::kRecFast: {
            std::vector<uint32_t> h_terms(text.terms.count);
            HIP_CHECK(hipMemcpyAsync(h_terms.data(), text.terms.pos, sizeof(uint32_t) * h_terms.size(), hipMemcpyDeviceToHost, s));
            HIP_CHECK(hipStreamSynchronize(s));
            radix_sort_record_keys(text, h_terms, keys32, vals, seg_mem, seg, arena, s, ctx.profiler());
            break;
        }
        default: {
            int shifts0[8];  // only the low key_bits of the key are populated
            for (int p = 0; p < plan.key_passes; ++p) shifts0[p] = p * kRadixBits;
            cur = radix_sort_initial_keys(text, keys, vals, shifts0, plan.key_passes, arena, s, ctx.profiler());
        }
        }
        if (cur != plan.cur || (!fused && vals[cur] != b.sa)) throw HipError("suffix array: key sort did not end in sa");
    }
    if (round0.done) {
        uint32_t total2[2] = {0, 0};
        ctx.read_back(b.d_total, total2, 2);
        b.m = total2[0];
        b.a_cur ^= 1;
    } else {
        RegroupIn in;
        in.keys = keys[plan.cur];
        in.vals = b.sa;
        if (plan.bucketed) {
            in.keys32 = keys32[plan.cur];
            in.seg = &seg;
        }
        in.sym_bits = plan.choice == KeyPlan::kKey35 ? plan.key_bits : plan.k_syms * text.bits;
        in.tag_bits = plan.tag_bits;
        in.bits = text.bits;
        in.low_bits = plan.low_bits;
        in.short_tag = plan.short_tag;
        in.seq_shift = plan.seq_shift;
        in.by_slot = true;
        regroup<true>(b, in);
    }
    arena.rewind(sort_mark);  // keys and the second value buffer are done
}

}  // namespace

// Work arrays of the rounds behind write_all_ranks, one entry per tied suffix -- or per text position when the
// pair-run pass will run (it works in text order; the rounds behind it then use the same arrays) --, the counts
// that tell which of the passes of sa_repeats.hip can do anything, and the pyramid over the LCP values known so far.
// (force_pair_runs: the test hook nolzss_debug_repeat_pass, whatever NOLZSS_PAIR_RUNS_MIN says)
void set_up_late_rounds(SaBuild &b, bool force_pair_runs) {
    const SaKnobs &knobs = sa_knobs();
    hipStream_t s = b.stream();
    Arena &arena = b.arena();
    const uint32_t n = b.n, m = b.m;
    b.pair_runs = m > 0 && (force_pair_runs || (knobs.pair_runs_min >= 0 ? (long long)m >= knobs.pair_runs_min : m >= n / 16));
    b.wlen = m == 0 ? 0 : (b.pair_runs ? (size_t)n : (size_t)m);
    if (m > 0) {
        try {
            for (uint32_t **a : {&b.tmp_a, &b.tmp_b, &b.tmp_c, &b.rank_val, &b.scratch_idx, &b.scratch_val, &b.lo, &b.out_lo, &b.out_vals})
                *a = arena.alloc<uint32_t>(b.wlen);
        } catch (const HipError &) {
            char buf[256];
            snprintf(buf, sizeof buf,
                     "suffix array: %u of %u suffixes are still tied after the direct round (a highly repetitive text); "
                     "the rounds that resolve them need about %.1f GiB more device memory than this device has left",
                     m, n, 60.0 * (double)b.wlen / 1073741824.0);
            throw HipError(buf);
        }
    }
    b.d_large = arena.alloc<uint32_t>(4);
    if (b.pair_runs) {
        uint32_t h4[4] = {0, 0, 0, 0};
        count_large_groups(b, kRunGroupMax, b.d_large, h4);
        b.in_large = h4[0];
        b.large_members = h4[0] + kRunGroupMax * h4[1];
        b.tied_groups = h4[2];
        b.near_members = h4[3];
        if (knobs.trace) fprintf(stderr, "[nolzss]   %u tied suffixes in %u groups, %u of them in groups of more than %u, %u next to a member at most %u symbols away\n",
                                 m, b.tied_groups, b.large_members, kRunGroupMax, b.near_members, kPerVerifyMax);
    }
    b.pyr_mark = arena.mark();
    if (m > 0) {
        ProfScope ps(b.ctx.profiler(), "sa_lcp_pyramid", s);
        b.Plcp = build_pyramid(b.lcp, n + 1, false, arena, s);
    }
    int nbits = 1;
    while (nbits < 32 && (1ull << nbits) <= (uint64_t)n) ++nbits;  // ranks and slots are <= n
    b.half_passes = (nbits + kRadixBits - 1) / kRadixBits;
    for (int p = 0; p < b.half_passes; ++p) b.shifts[b.npasses++] = p * kRadixBits;
    for (int p = 0; p < b.half_passes; ++p) b.shifts[b.npasses++] = 32 + p * kRadixBits;
}

namespace {

// Members of the large groups: the group of an element is known from where it lies (a group's members are
// consecutive in the list, so also in the gathered array), so the groups are the BUCKETS of a segmented
// sort by the key alone -- four passes on 8-byte records instead of eight on 12-byte ones.
// false: the groups are too small for it (nothing has been sorted).
bool sort_large_groups_segmented(SaBuild &b, uint32_t n_large, const uint32_t *rvals) {
    hipStream_t s = b.stream();
    Arena &arena = b.arena();
    const uint32_t m = b.m;
    ProfScope ps(b.ctx.profiler(), "sa_sort_large", s);
    const size_t lmark = arena.mark();
    uint32_t *lk[2] = {arena.alloc<uint32_t>(n_large), arena.alloc<uint32_t>(n_large)};
    uint32_t *lv[2] = {arena.alloc<uint32_t>(n_large), arena.alloc<uint32_t>(n_large)};
    uint32_t *lgrp = arena.alloc<uint32_t>(n_large);
    uint32_t *lidx = b.tmp_c;
    gather_large32_kernel<<<grid_for(m, kThreads), kThreads, 0, s>>>(b.tmp_a, b.tmp_b, b.grp(), b.lo, rvals, m, lk[0], lv[0], lidx, lgrp);
    KERNEL_CHECK();
    // first element of every group -> segment table on the host
    uint32_t *head = lk[1], *pos = lv[1];  // (free until the first pass)
    large_heads_kernel<<<grid_for(n_large, kThreads), kThreads, 0, s>>>(lgrp, n_large, head);
    KERNEL_CHECK();
    scan_exclusive_add_u32(head, pos, n_large, b.d_total + 3, arena, s);
    uint32_t nb = 0;
    b.ctx.read_back(b.d_total + 3, &nb, 1);
    // (a tile of the segmented passes never straddles a group: groups of a few hundred members would leave the
    // 4096-pair tiles mostly empty -- those keep the global sort)
    const bool take = (uint64_t)nb * 2048u <= (uint64_t)n_large;
    if (take) {
        uint32_t *d_starts = arena.alloc<uint32_t>((size_t)nb + 1);
        large_starts_kernel<<<grid_for(n_large, kThreads), kThreads, 0, s>>>(head, pos, n_large, d_starts);
        KERNEL_CHECK();
        std::vector<uint32_t> h_start((size_t)nb + 1);
        HIP_CHECK(hipMemcpyAsync(h_start.data(), d_starts, (size_t)nb * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipStreamSynchronize(s));
        h_start[nb] = n_large;
        const int c = radix_sort_segments_u32(lk, lv, n_large, h_start, b.half_passes, arena, s, b.ctx.profiler());
        scatter_large32_kernel<<<grid_for(n_large, kThreads), kThreads, 0, s>>>(lk[c], lv[c], lidx, n_large, b.out_lo, b.out_vals);
        KERNEL_CHECK();
    }
    arena.rewind(lmark);
    return take;
}

// members of groups larger than kSmallGroup: global radix sort of 12-byte (group, key) records
void sort_large_groups_global(SaBuild &b, uint32_t n_large, const uint32_t *rvals) {
    hipStream_t s = b.stream();
    Arena &arena = b.arena();
    const uint32_t m = b.m;
    ProfScope ps(b.ctx.profiler(), "sa_sort_large", s);
    const size_t lmark = arena.mark();
    uint64_t *lk[2] = {arena.alloc<uint64_t>(n_large), arena.alloc<uint64_t>(n_large)};
    uint32_t *lv[2] = {arena.alloc<uint32_t>(n_large), arena.alloc<uint32_t>(n_large)};
    uint32_t *lidx = b.tmp_c;
    gather_large_kernel<<<grid_for(m, kThreads), kThreads, 0, s>>>(b.tmp_a, b.tmp_b, b.grp(), b.lo, rvals, m, lk[0], lv[0], lidx);
    KERNEL_CHECK();
    const int c = radix_sort_pairs(lk, lv, n_large, b.shifts, b.npasses, arena, s, b.ctx.profiler());
    scatter_large_kernel<<<grid_for(n_large, kThreads), kThreads, 0, s>>>(lk[c], lv[c], lidx, n_large, b.out_lo, b.out_vals, nullptr, 0u);
    KERNEL_CHECK();
    arena.rewind(lmark);
}

// One doubling round: the tied suffixes are sorted inside their groups by rank[i + h].  mid_groups: groups of
// 65 .. 1024 members are sorted in LDS (until a round finds none: groups only shrink).
void doubling_round(SaBuild &b, bool &mid_groups) {
    hipStream_t s = b.stream();
    const uint32_t m = b.m;
    const uint32_t *slot = b.slot(), *grp = b.grp();
    uint32_t *rvals = b.rank_by_slot;  // free since rank[] has been written
    {
        ProfScope ps(b.ctx.profiler(), "sa_round_keys", s);
        round_keys_kernel<<<grid_for(m, kThreads), kThreads, 0, s>>>(slot, m, b.sa, b.rank, b.n, (uint32_t)b.h, b.lo, rvals);
        KERNEL_CHECK();
    }
    {
        ProfScope ps(b.ctx.profiler(), "sa_small_sort", s);
        small_sort_kernel<<<grid_for(m, kThreads), kThreads, 0, s>>>(slot, grp, b.lo, rvals, m, b.out_lo, b.out_vals, b.tmp_a);
        KERNEL_CHECK();
        if (mid_groups) {
            HIP_CHECK(hipMemsetAsync(b.d_total + 1, 0, sizeof(uint32_t), s));
            mid_sort_kernel<<<(unsigned)div_up(m, kMidGroup), kMidThreads, 0, s>>>(slot, grp, b.lo, rvals, m, b.out_lo, b.out_vals,
                                                                                  b.tmp_a, b.d_total + 1);
            KERNEL_CHECK();
        }
        scan_exclusive_add_u32(b.tmp_a, b.tmp_b, m, b.d_total, b.arena(), s);
    }
    uint32_t h2[2] = {0, 0};
    b.ctx.read_back(b.d_total, h2, 2);
    const uint32_t n_large = h2[0];
    if (mid_groups && h2[1] == 0 && n_large == 0) mid_groups = false;
    if (n_large > 0 && (sa_knobs().no_seg_large || !sort_large_groups_segmented(b, n_large, rvals)))
        sort_large_groups_global(b, n_large, rvals);
    RegroupIn in;
    in.lo = b.out_lo;
    in.vals = b.out_vals;
    in.dbl_h = (uint32_t)b.h;
    regroup<false>(b, in);
    if (sa_knobs().trace)
        fprintf(stderr, "[nolzss]   doubling round h=%llu: %u in large groups, %u still tied\n", (unsigned long long)b.h, n_large, b.m);
    b.h *= 2;
}

}  // namespace

int build_suffix_array(Context &ctx, const PackedText &text, uint32_t *sa, uint32_t *isa, uint32_t *lcp,
                       bool *isa_deferred) {
    if (isa_deferred) *isa_deferred = false;
    const SaKnobs &knobs = sa_knobs();
    const uint32_t n = text.n;
    hipStream_t s = ctx.stream;
    Arena &arena = ctx.arena;
    const size_t mark = arena.mark();
    const KeyPlan plan = plan_keys(text);
    SaBuild b{ctx, text, n, sa, /*rank=*/isa, lcp};
    b.independent = plan.independent();

    // Buffers live in scopes (the arena is a stack): what the whole construction needs first -- the two
    // active lists and the rank of every slot -- then the buffers of one phase at a time, released when the
    // phase ends.  Everything behind the direct round is sized by the number of suffixes that are still
    // tied, not by n: 32 n bytes stay for the whole construction (sa, rank, lcp from the caller, the
    // lists, rank_by_slot), the key sort adds 12.5 n (2-bit texts) and the rank scatter 12 n on top of
    // them, the doubling rounds 60 bytes per TIED suffix (96 n only when every suffix is tied, as on a
    // periodic text; a text with 5 % of its suffixes tied after the direct round peaks at 45 n).
    // Can the caller be left without rank[] if the direct rounds finish the suffix array (see below)?  The regroup
    // kernels then do not store the rank of every slot either (nobody would read it; if doubling rounds turn out
    // to be needed, write_all_ranks recovers it from the LCP array).
    // (the two-value permutation takes 8 n bytes more than the one it replaces: 57 n at the peak of the candidate
    // stage; an arena that settled for less keeps the rank scatter.  Texts of more than 2^30 symbols keep it too:
    // the two-value form has two partition passes.)
    // (a merged batch of long records: its block-diagonal permutation has the two-value form too, RecordScatterPlan)
    const bool plan_two = ctx.rec_plan && ctx.rec_plan->seg.desc && ctx.rec_plan->n == n && !text.terms.mirror;
    b.can_defer = isa_deferred && !knobs.no_defer && (plan_two || (text.terms.seq_shift == 0 && n <= (1u << 30))) &&
                  arena.capacity() >= 60 * (size_t)n + (size_t(64) << 20);
    if (knobs.trace && isa_deferred && !b.can_defer)
        fprintf(stderr, "[nolzss]   rank[] is scattered after the direct rounds (arena %.1f of %.1f GiB, %s)\n",
                (double)arena.capacity() / 1073741824.0, (60.0 * (double)n + 67108864.0) / 1073741824.0,
                text.terms.seq_shift ? (plan_two ? "records with a plan" : "independent records without a plan") : "one text");
    b.store_ranks = !b.can_defer;
    for (uint32_t **a : {&b.act_slot[0], &b.act_slot[1], &b.act_grp[0], &b.act_grp[1], &b.rank_by_slot}) *a = arena.alloc<uint32_t>(n);
    b.d_total = arena.alloc<uint32_t>(4);

    b.m = n;
    b.a_cur = 1;  // (round 0 fills list 0)
    key_sort_round0(b, plan);
    b.h = (uint64_t)plan.k_syms;
    if (knobs.trace) {
        // (the name tells rows of the plan with the same width apart: dna_fast, segmented and general all sort 17 bases)
        static const char *const kPlanNames[] = {"fused", "key16", "key35", "dna_fast", "rec_fast", "independent", "segmented", "general"};
        const char *name = plan.choice == KeyPlan::kIndependent && text.terms.mirror ? "independent_mirrored" : kPlanNames[plan.choice];
        if (plan.choice == KeyPlan::kKey35)
            fprintf(stderr, "[nolzss] n=%u: %u suffixes tied after the %d-bit key sort (plan: %s)\n", n, b.m, plan.key_bits, name);
        else
            fprintf(stderr, "[nolzss] n=%u: %u suffixes tied after the %d-symbol key sort (plan: %s)\n", n, b.m, plan.k_syms, name);
    }
    if (b.m > 0 && b.h < n) direct_round(b, plan.k_syms);
    group_sort_passes(b);

    // Nothing is tied any more: no round below needs rank[].  A caller that can wait gets it from the permutation
    // that brings the factor-length codes into text order (pipeline.hpp) -- one full random permutation per
    // factorization instead of two.
    if (b.m == 0 && b.can_defer) {
        *isa_deferred = true;
        if (knobs.trace) fprintf(stderr, "[nolzss]   suffix array finished by the direct rounds: rank[] is left to the permutation of the codes\n");
        HIP_CHECK(hipMemsetAsync(lcp + n, 0, sizeof(uint32_t), s));
        arena.rewind(mark);
        return 0;
    }
    write_all_ranks(b);
    set_up_late_rounds(b);
    if (b.pair_runs) periodic_pass(b);
    pair_run_passes(b);

    int rounds = 0;
    bool mid_groups = !knobs.no_mid_sort;
    while (b.m > 0) {
        if (b.h >= n || rounds > 40) throw HipError("suffix array: prefix doubling failed to converge");
        if (b.pair_runs && b.per_hint != 0 && b.h >= b.per_hint && b.m >= n / 16) {
            periodic_pass(b);
            if (b.m == 0) break;
        }
        doubling_round(b, mid_groups);
        ++rounds;
    }
    // (rank[] stays 1-based: every group is a singleton now, so rank[i] = ISA[i] + 1; the consumers
    // subtract the one instead of a pass over the array doing it)
    // every boundary received its LCP when it appeared; the caller checks that no pending code is left
    // while it builds the LCP pyramid (build_lcp_pyramid) instead of a pass of its own
    HIP_CHECK(hipMemsetAsync(lcp + n, 0, sizeof(uint32_t), s));
    arena.rewind(mark);
    return rounds;
}

}  // namespace nolzss
