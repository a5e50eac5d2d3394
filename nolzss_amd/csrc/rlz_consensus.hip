// rlz_consensus.hip -- the insertion alleles of a pileup's log and the consensus of its counters (DESIGN.md 5,
// "Relative-LZ index: consensus"; the entry points: rlz_pileup_api.hip, nolzss_rlz_pileup_insertions / _consensus; the
// rules: include/nolzss_hip.h).
//
// The log holds one 24-byte event per I op (rlz_pileup.hip).  The allele table is its distinct events with their
// multiplicities: a permutation sorted by three chained stable radix sorts -- bases[1], then bases[0], then (position,
// length) --, a flag at the first event of every run of equal events, one scan, and a scatter of the run heads; a run's
// length is the distance to the next head.  The consensus is the shape a variants query has: a byte count per position,
// one exclusive scan, and a scatter of the bytes -- the call of the position, then the modal insertion allele behind it.
//
// No kernel here spins or communicates between workgroups; every loop bound is a count clamped on load, and no store
// leaves the [first, first + count) window of the stage it writes.
#include "rlz_pileup_device.hpp"

#include "radix_sort.hpp"
#include "scan.hpp"

namespace nolzss {
namespace {

constexpr int kThreads = 256;
constexpr uint32_t kNoAllele = 0xffffffffu;
constexpr unsigned kLengthBlocks = 2048;  // workgroups of the consensus length kernel: eight per CU of an MI355X

__device__ __forceinline__ bool same_event(const PileupEvent &a, const PileupEvent &b) {
    return a.position == b.position && a.length == b.length && a.bases[0] == b.bases[0] && a.bases[1] == b.bases[1];
}

// One lane per event: the identity permutation and the first sort key.  No loop.
__global__ __launch_bounds__(kThreads) void allele_first_keys_kernel(const PileupEvent *__restrict__ ev, uint32_t E,
                                                                     uint64_t *__restrict__ keys, uint32_t *__restrict__ perm) {
    const uint64_t gid = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (gid >= E) return;
    keys[gid] = ev[gid].bases[1];
    perm[gid] = (uint32_t)gid;
}

// One lane per place of the permutation: the next sort key of the event there.  which 0: bases[0]; 1: (position,
// length).  No loop.
__global__ __launch_bounds__(kThreads) void allele_next_keys_kernel(const PileupEvent *__restrict__ ev, uint32_t E,
                                                                    const uint32_t *__restrict__ perm, int which,
                                                                    uint64_t *__restrict__ keys) {
    const uint64_t gid = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (gid >= E) return;
    uint32_t e = perm[gid];
    e = e < E ? e : E - 1u;
    keys[gid] = which == 0 ? ev[e].bases[0] : ((uint64_t)ev[e].position << 32) | ev[e].length;
}

// One lane per place: 1 where the event differs from the one in front of it.  No loop.
__global__ __launch_bounds__(kThreads) void allele_heads_kernel(const PileupEvent *__restrict__ ev, uint32_t E,
                                                                const uint32_t *__restrict__ perm, uint32_t *__restrict__ head) {
    const uint64_t gid = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (gid >= E) return;
    uint32_t e = perm[gid], f = gid ? perm[gid - 1] : 0u;
    e = e < E ? e : E - 1u;
    f = f < E ? f : E - 1u;
    head[gid] = (gid == 0 || !same_event(ev[e], ev[f])) ? 1u : 0u;
}

// One lane per place: a head writes its event and its place to the slot its rank names.  No loop.
__global__ __launch_bounds__(kThreads) void allele_scatter_kernel(const PileupEvent *__restrict__ ev, uint32_t E,
                                                                  const uint32_t *__restrict__ perm,
                                                                  const uint32_t *__restrict__ head,
                                                                  const uint32_t *__restrict__ rank,
                                                                  PileupAllele *__restrict__ out, uint32_t *__restrict__ first) {
    const uint64_t gid = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (gid >= E || !head[gid]) return;
    const uint32_t g = rank[gid];
    if (g >= E) return;  // (the ranks of E places stay below E)
    uint32_t e = perm[gid];
    e = e < E ? e : E - 1u;
    PileupAllele a;
    a.position = ev[e].position;
    a.length = ev[e].length;
    a.count = 0;
    a.pad = 0;
    a.bases[0] = ev[e].bases[0];
    a.bases[1] = ev[e].bases[1];
    out[g] = a;
    first[g] = (uint32_t)gid;
}

// One lane per allele: its events are the places from its head to the next one.  No loop.
__global__ __launch_bounds__(kThreads) void allele_counts_kernel(PileupAllele *__restrict__ out, const uint32_t *__restrict__ first,
                                                                 uint32_t G, uint32_t E) {
    const uint64_t gid = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (gid >= G) return;
    out[gid].count = (gid + 1 < G ? first[gid + 1] : E) - first[gid];
}

// The first allele at a position >= p.  Loop: at most 32 halvings.
__device__ __forceinline__ uint32_t allele_lower_bound(const PileupAllele *__restrict__ al, uint32_t G, uint32_t p) {
    uint32_t lo = 0, hi = G;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (al[mid].position >= p)
            hi = mid;
        else
            lo = mid + 1;
    }
    return lo;
}

// One lane per allele: whether it passes the rule against its position's depth.  Loop: the separator search.
__global__ __launch_bounds__(kThreads) void insertion_flags_kernel(PileupView v, const uint64_t *__restrict__ xwords, TermTable xt,
                                                                   const PileupAllele *__restrict__ al, uint32_t G,
                                                                   PileupRule rule, uint32_t *__restrict__ nrec) {
    const uint64_t gid = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (gid >= G) return;
    const PileupAllele a = al[gid];
    uint32_t pass = 0;
    if (a.position < v.B) {
        uint32_t first, ch[kPileupChannels];
        bool separator;
        block_record_of(xt, a.position, first, separator);
        channels_of(v, xwords, separator, a.position, ch);
        const uint64_t d = depth_of(ch), n = a.count;
        pass = (!separator && n >= rule.min_count && n * rule.den >= rule.num * d) ? 1u : 0u;
    }
    nrec[gid] = pass;
}

// One lane per allele: a passing one inside the window writes its record.  Loop: the separator search.
__global__ __launch_bounds__(kThreads) void insertion_records_kernel(PileupView v, const uint64_t *__restrict__ xwords,
                                                                     TermTable xt, const PileupAllele *__restrict__ al, uint32_t G,
                                                                     const uint32_t *__restrict__ nrec,
                                                                     const uint32_t *__restrict__ off, uint64_t first,
                                                                     uint32_t count, PileupInsertionRec *__restrict__ out) {
    const uint64_t gid = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (gid >= G || !nrec[gid]) return;
    const uint64_t at = off[gid];
    if (at < first || at >= first + count) return;
    const PileupAllele a = al[gid];
    if (a.position >= v.B) return;
    uint32_t rec_first, ch[kPileupChannels];
    bool separator;
    const uint32_t record = block_record_of(xt, a.position, rec_first, separator);
    channels_of(v, xwords, separator, a.position, ch);
    PileupInsertionRec r;
    r.position = a.position;
    r.record_offset = a.position - rec_first;
    r.record = record;
    r.length = a.length;
    r.count = a.count;
    r.depth = depth_of(ch);
    r.ins_total = ch[5];
    r.truncated = a.length > kPileupInsBases ? 1u : 0u;
    r.bases[0] = a.bases[0];
    r.bases[1] = a.bases[1];
    out[at - first] = r;
}

// What position p < B of the block emits: `letter` (0: nothing) and behind it the bases of allele `allele` (kNoAllele:
// none).  The flags feed the statistics.
struct Call {
    uint32_t letter, allele, length;  // length: of the allele emitted, 1 .. kPileupInsBases
    bool separator, low, substitution, deleted, truncated;
};
// Loops: the separator search; the bisection of the allele table; the alleles of p (at most G).
__device__ __forceinline__ Call call_of(const PileupView &v, const uint64_t *__restrict__ xwords, const TermTable &xt,
                                        const PileupAllele *__restrict__ al, uint32_t G, const ConsensusRule &rule, uint32_t p) {
    Call c;
    c.letter = 0;
    c.allele = kNoAllele;
    c.length = 0;
    c.separator = c.low = c.substitution = c.deleted = c.truncated = false;
    uint32_t first, ch[kPileupChannels];
    block_record_of(xt, p, first, c.separator);
    if (c.separator) {
        c.letter = 1u;
        return c;
    }
    const uint32_t b = channels_of(v, xwords, false, p, ch);
    uint32_t call;
    uint64_t d;
    if (base_call_of(ch, b, rule, call, d)) {  // (the rule shared with a cohort's pack: rlz_pileup_device.hpp)
        c.low = true;
        c.letter = rule.low ? 'N' : "ACGT"[b];
        return c;
    }
    c.substitution = call < 4u && call != b;
    c.deleted = call == 4u;
    c.letter = call < 4u ? "ACGT"[call] : 0u;
    uint32_t best = kNoAllele, best_count = 0;
    for (uint32_t g = allele_lower_bound(al, G, p); g < G && al[g].position == p; ++g) {
        const uint32_t n = al[g].count;
        if (n > best_count) {  // (strictly: ties go to the first in table order)
            best_count = n;
            best = g;
        }
    }
    if (best != kNoAllele && (uint64_t)best_count * rule.den >= rule.num * d) {
        const uint32_t len = al[best].length;
        if (len > kPileupInsBases || len == 0) {
            c.truncated = true;
        } else {
            c.allele = best;
            c.length = len;
        }
    }
    return c;
}

// The entries of d_len (B + 1): the bytes of position p, 0 for entry B; the statistics summed per lane, then per
// wavefront.  Loops: those of call_of; the stride over the entries (at most ceil((B + 1) / the grid's lanes) turns).
__global__ __launch_bounds__(kThreads) void consensus_lengths_kernel(PileupView v, const uint64_t *__restrict__ xwords,
                                                                     TermTable xt, const PileupAllele *__restrict__ al, uint32_t G,
                                                                     ConsensusRule rule, uint32_t *__restrict__ len,
                                                                     unsigned long long *__restrict__ stats) {
    unsigned long long st[kConsensusStats] = {0, 0, 0, 0, 0, 0, 0};
    // a grid of at most kLengthBlocks workgroups strides over the entries, so the seven words take at most
    // 4 * kLengthBlocks atomics each, not one per 64 positions (profiles/r17_rlz_index_consensus.txt)
    const uint64_t stride = (uint64_t)gridDim.x * kThreads;
    for (uint64_t gid = (uint64_t)blockIdx.x * kThreads + threadIdx.x; gid <= v.B; gid += stride) {
        if (gid == v.B) {
            len[gid] = 0;
            break;
        }
        const Call c = call_of(v, xwords, xt, al, G, rule, (uint32_t)gid);
        len[gid] = (c.letter ? 1u : 0u) + c.length;
        if (!c.separator) {
            st[0] += c.low ? 0 : 1;
            st[1] += c.low ? 1 : 0;
            st[2] += c.substitution ? 1 : 0;
            st[3] += c.deleted ? 1 : 0;
            st[4] += c.allele != kNoAllele ? 1 : 0;
            st[5] += c.length;
            st[6] += c.truncated ? 1 : 0;
        }
    }
#pragma unroll
    for (uint32_t k = 0; k < kConsensusStats; ++k) {
#pragma unroll
        for (int o = 32; o; o >>= 1) st[k] += __shfl_xor(st[k], o, 64);
        if ((threadIdx.x & 63u) == 0 && st[k]) atomicAdd(stats + k, st[k]);
    }
}

// One lane per position: those of its bytes that fall into [first, first + count).  Loops: those of call_of; the
// allele's bases (at most kPileupInsBases).
__global__ __launch_bounds__(kThreads) void consensus_text_kernel(PileupView v, const uint64_t *__restrict__ xwords, TermTable xt,
                                                                  const PileupAllele *__restrict__ al, uint32_t G,
                                                                  ConsensusRule rule, const uint32_t *__restrict__ off,
                                                                  uint64_t first, uint32_t count, uint8_t *__restrict__ out) {
    const uint64_t gid = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (gid >= v.B) return;
    uint64_t at = off[gid];
    const uint64_t end = off[gid + 1];  // (the scan holds B + 1 entries)
    if (at >= first + count || end <= first) return;
    const Call c = call_of(v, xwords, xt, al, G, rule, (uint32_t)gid);
    if (c.letter) {
        if (at >= first && at < first + count) out[at - first] = (uint8_t)c.letter;
        ++at;
    }
    if (c.allele == kNoAllele) return;
    const uint64_t w0 = al[c.allele].bases[0], w1 = al[c.allele].bases[1];
    for (uint32_t j = 0; j < c.length; ++j, ++at)
        if (at >= first && at < first + count) out[at - first] = (uint8_t)"ACGT"[base_of(j < 32u ? w0 : w1, j)];
}

__global__ __launch_bounds__(kThreads) void consensus_starts_kernel(const uint32_t *__restrict__ off, uint64_t first,
                                                                    uint32_t count, uint64_t *__restrict__ out) {
    const uint64_t gid = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (gid >= count) return;
    out[gid] = off[first + gid];
}

// One lane per entry: record r begins behind terminator r - 1 of the block's table.  No loop.
__global__ __launch_bounds__(kThreads) void consensus_record_offsets_kernel(TermTable xt, const uint32_t *__restrict__ off,
                                                                            uint32_t B, uint32_t records, uint64_t total,
                                                                            uint64_t *__restrict__ out) {
    const uint64_t gid = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (gid > records) return;
    if (gid == records) {
        out[gid] = total + 1;
        return;
    }
    uint32_t p = gid ? (gid - 1 < xt.count ? xt.pos[gid - 1] : B) + 1u : 0u;
    p = p < B ? p : B;
    out[gid] = p < B ? (uint64_t)off[p] : total + 1;  // (a record behind the block's end: an empty one, none by construction)
}

unsigned grid_for(size_t n) { return (unsigned)div_up(n, (size_t)kThreads); }

}  // namespace

const PileupAllele *rlz_pileup_alleles(Context &ctx, const PileupEvent *d_events, uint32_t E, uint32_t *count) {
    hipStream_t s = ctx.stream;
    *count = 0;
    if (E == 0) return nullptr;
    PileupAllele *out = ctx.arena.alloc<PileupAllele>(E);
    uint32_t *first = ctx.arena.alloc<uint32_t>(E);
    const size_t mark = ctx.arena.mark();
    uint64_t *keys[2] = {ctx.arena.alloc<uint64_t>(E), ctx.arena.alloc<uint64_t>(E)};
    uint32_t *vals[2] = {ctx.arena.alloc<uint32_t>(E), ctx.arena.alloc<uint32_t>(E)};
    uint32_t *head = ctx.arena.alloc<uint32_t>(E), *rank = ctx.arena.alloc<uint32_t>(E);
    uint32_t *d_total = ctx.arena.alloc<uint32_t>(1);
    const int shifts[8] = {0, 8, 16, 24, 32, 40, 48, 56};
    uint32_t G = 0;
    {
        ProfScope ps(ctx.profiler(), "rlz_pileup_alleles", s, 3.0 * 8.0 * 24.0 * (double)E);
        allele_first_keys_kernel<<<grid_for(E), kThreads, 0, s>>>(d_events, E, keys[0], vals[0]);
        KERNEL_CHECK();
        int at = radix_sort_pairs(keys, vals, E, shifts, 8, ctx.arena, s, ctx.profiler());
        for (int which = 0; which < 2; ++which) {  // stable: the later key dominates
            uint64_t *k2[2] = {keys[at], keys[at ^ 1]};
            uint32_t *v2[2] = {vals[at], vals[at ^ 1]};
            allele_next_keys_kernel<<<grid_for(E), kThreads, 0, s>>>(d_events, E, v2[0], which, k2[0]);
            KERNEL_CHECK();
            at ^= radix_sort_pairs(k2, v2, E, shifts, 8, ctx.arena, s, ctx.profiler());
        }
        const uint32_t *perm = vals[at];
        allele_heads_kernel<<<grid_for(E), kThreads, 0, s>>>(d_events, E, perm, head);
        KERNEL_CHECK();
        scan_exclusive_add_u32(head, rank, E, d_total, ctx.arena, s);
        allele_scatter_kernel<<<grid_for(E), kThreads, 0, s>>>(d_events, E, perm, head, rank, out, first);
        KERNEL_CHECK();
        HIP_CHECK(hipMemcpyAsync(&G, d_total, sizeof G, hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipStreamSynchronize(s));  // (G is a local)
        G = G < E ? G : E;
        allele_counts_kernel<<<grid_for(G), kThreads, 0, s>>>(out, first, G, E);
        KERNEL_CHECK();
    }
    ctx.arena.rewind(mark);  // (the kernels queued read it in stream order, in front of whatever takes it next)
    *count = G;
    return out;
}

void rlz_pileup_insertion_flags(Context &ctx, const PileupView &v, const PackedText &block, const PileupAllele *d_alleles,
                                uint32_t G, const PileupRule &rule, uint32_t *d_n) {
    if (G == 0) return;
    ProfScope ps(ctx.profiler(), "rlz_pileup_insertion_flags", ctx.stream, 80.0 * (double)G);
    insertion_flags_kernel<<<grid_for(G), kThreads, 0, ctx.stream>>>(v, block.words, block.terms, d_alleles, G, rule, d_n);
    KERNEL_CHECK();
}

void rlz_pileup_insertion_records(Context &ctx, const PileupView &v, const PackedText &block, const PileupAllele *d_alleles,
                                  uint32_t G, const uint32_t *d_n, const uint32_t *d_off, uint64_t first, uint32_t count,
                                  PileupInsertionRec *d_out) {
    if (G == 0 || count == 0) return;
    ProfScope ps(ctx.profiler(), "rlz_pileup_insertion_records", ctx.stream, 40.0 * (double)G + 56.0 * (double)count);
    insertion_records_kernel<<<grid_for(G), kThreads, 0, ctx.stream>>>(v, block.words, block.terms, d_alleles, G, d_n, d_off, first,
                                                                      count, d_out);
    KERNEL_CHECK();
}

void rlz_consensus_lengths(Context &ctx, const PileupView &v, const PackedText &block, const PileupAllele *d_alleles, uint32_t G,
                           const ConsensusRule &rule, uint32_t *d_len, unsigned long long *d_stats) {
    HIP_CHECK(hipMemsetAsync(d_stats, 0, kConsensusStats * sizeof(unsigned long long), ctx.stream));
    ProfScope ps(ctx.profiler(), "rlz_consensus_lengths", ctx.stream, 48.0 * (double)v.B);
    const unsigned blocks = grid_for((size_t)v.B + 1);
    consensus_lengths_kernel<<<blocks < kLengthBlocks ? blocks : kLengthBlocks, kThreads, 0, ctx.stream>>>(v, block.words, block.terms, d_alleles, G, rule,
                                                                                    d_len, d_stats);
    KERNEL_CHECK();
}

void rlz_consensus_text(Context &ctx, const PileupView &v, const PackedText &block, const PileupAllele *d_alleles, uint32_t G,
                        const ConsensusRule &rule, const uint32_t *d_off, uint64_t first, uint32_t count, uint8_t *d_out) {
    if (v.B == 0 || count == 0) return;
    ProfScope ps(ctx.profiler(), "rlz_consensus_text", ctx.stream, 48.0 * (double)v.B + (double)count);
    consensus_text_kernel<<<grid_for(v.B), kThreads, 0, ctx.stream>>>(v, block.words, block.terms, d_alleles, G, rule, d_off, first,
                                                                     count, d_out);
    KERNEL_CHECK();
}

void rlz_consensus_starts(Context &ctx, const uint32_t *d_off, uint64_t first, uint32_t count, uint64_t *d_out) {
    if (count == 0) return;
    consensus_starts_kernel<<<grid_for(count), kThreads, 0, ctx.stream>>>(d_off, first, count, d_out);
    KERNEL_CHECK();
}

void rlz_consensus_record_offsets(Context &ctx, const PackedText &block, const uint32_t *d_off, uint32_t B, uint32_t records,
                                  uint64_t total, uint64_t *d_out) {
    consensus_record_offsets_kernel<<<grid_for((size_t)records + 1), kThreads, 0, ctx.stream>>>(block.terms, d_off, B, records, total,
                                                                                               d_out);
    KERNEL_CHECK();
}

}  // namespace nolzss
