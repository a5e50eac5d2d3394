// rlz_find.hip -- locate through the parse of a relative-LZ archive ("Relative-LZ archive: locate through
// the parse"; the entry points: rlz_find_api.hip, nolzss_rlz_finder_*).
//
// The records tile the decoded space.  An occurrence of a pattern in a target either lies inside ONE copy record -- then
// the record's source interval [lo, hi) of the block holds the same bytes (or their reverse complement), the pattern
// occurs in the block, and the occurrence is found from that block occurrence by asking which records' sources cover it
// (secondary) --, or it crosses a record start or is a literal (primary) -- then it lies inside the window of M - 1 bases
// to either side of that record start, and the windows of all record starts, extracted once into the kernel text K
// and indexed like a reference, hold every such occurrence.
//
// Covering sources: the source table orders the records by lo.  The records with lo <= x are a prefix [0, r] of it, and
// among them those with hi >= x + m are listed right to left by repeated nearest-left queries on the max pyramid over
// hi[].  Every query returns one covering record or ends the walk, so a walk takes (covering records + 1) queries.
//
// No kernel here spins, communicates between workgroups or uses an atomic.  Every loop is bounded by a data size: the
// binary searches by 32 steps, the record search by 9 (rlz_archive.hpp), the walk by z + 1 queries, the scan of the tile
// sums by their number.  Every index that leads a load or a store is checked against the size the host passes.
#include "rlz_find.hpp"

#include "radix_sort.hpp"
#include "scan.hpp"

namespace nolzss {
namespace {

constexpr int kThreads = 256;

__device__ __forceinline__ uint32_t complement(uint32_t c) {  // 0: not a nucleotide
    return c == 'A' ? 'T' : c == 'T' ? 'A' : c == 'C' ? 'G' : c == 'G' ? 'C' : 0u;
}

// the number of entries of a[0 .. n) that are <= x (a ascending): at most 32 steps
__device__ __forceinline__ uint32_t upper_bound_u32(const uint32_t *__restrict__ a, uint32_t n, uint32_t x) {
    uint32_t lo = 0, hi = n;
    for (int step = 0; step < 32 && lo < hi; ++step) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (a[mid] <= x) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// ---- intervals ---------------------------------------------------------------------------------------------------------
// The target [tb, te) that holds the record start b (empty targets repeat a base: the last one at or below b is the one
// with a byte), and the window of b clipped to it.
__device__ __forceinline__ void window_of(const uint32_t *__restrict__ bases, uint32_t k, uint32_t b, uint32_t W,
                                          uint32_t &tb, uint32_t &ws, uint32_t &we) {
    uint32_t j = upper_bound_u32(bases, k + 1, b);  // bases[0] = 0 <= b: j >= 1; b < bases[k]: j <= k
    j = j ? j - 1 : 0;
    j = j < k ? j : k - 1;
    tb = bases[j];
    const uint32_t te = bases[j + 1];
    ws = b - tb > W ? b - W : tb;
    we = te - b > W ? b + W : te;
}

// flag[i] = 1 where record i opens an interval: the first record of all, the first of a target, or a window that starts
// behind the end of the previous record's
__global__ __launch_bounds__(kThreads) void find_flags_kernel(const ArchiveRec *__restrict__ recs, uint32_t z,
                                                              const uint32_t *__restrict__ bases, uint32_t k, uint32_t W,
                                                              uint32_t *__restrict__ flag) {
    const uint64_t gid = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (gid >= z) return;
    const uint32_t i = (uint32_t)gid;
    const uint32_t b = recs[i].start;
    uint32_t tb, ws, we;
    window_of(bases, k, b, W, tb, ws, we);
    uint32_t opens = 1;
    if (i && b != tb) {  // the previous record lies in the same target
        uint32_t ptb, pws, pwe;
        window_of(bases, k, recs[i - 1].start, W, ptb, pws, pwe);
        opens = ws > pwe ? 1u : 0u;
    }
    flag[i] = opens;
}

// slot = the exclusive scan of flag.  The record that opens interval s writes dstart[s], the last record of interval s
// writes dend[s]: windows ascend with the records, so the last window ends the interval.
__global__ __launch_bounds__(kThreads) void find_bounds_kernel(const ArchiveRec *__restrict__ recs, uint32_t z,
                                                               const uint32_t *__restrict__ bases, uint32_t k, uint32_t W,
                                                               const uint32_t *__restrict__ flag,
                                                               const uint32_t *__restrict__ slot, uint32_t nI,
                                                               uint32_t *__restrict__ dstart, uint32_t *__restrict__ dend) {
    const uint64_t gid = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (gid >= z) return;
    const uint32_t i = (uint32_t)gid;
    const bool opens = flag[i] != 0, closes = i + 1 == z || flag[i + 1] != 0;
    if (!opens && !closes) return;
    uint32_t tb, ws, we;
    window_of(bases, k, recs[i].start, W, tb, ws, we);
    const uint32_t s = opens ? slot[i] : slot[i] - 1u;  // (a record that does not open one lies behind an opener)
    if (s >= nI) return;
    if (opens) dstart[s] = ws;
    if (closes) dend[s] = we;
}

// len[s] = the bytes of interval s, len[nI] = 0 (the scan over nI + 1 entries then ends in |K|); dstart[nI] = decoded
__global__ __launch_bounds__(kThreads) void find_lengths_kernel(uint32_t *__restrict__ dstart,
                                                                const uint32_t *__restrict__ dend, uint32_t nI,
                                                                uint32_t decoded, uint32_t *__restrict__ len) {
    const uint64_t gid = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (gid > nI) return;
    const uint32_t s = (uint32_t)gid;
    if (s == nI) {
        len[s] = 0;
        dstart[s] = decoded;
    } else {
        len[s] = dend[s] - dstart[s];
    }
}

// X[K_len] = s0; with the mirror: X[K_len + 1 + i] = comp(X[K_len - 1 - i]), X[2 K_len + 1] = s1.  bad: set to 1 by a
// byte of K that is not a nucleotide (plain stores of one value).
__global__ __launch_bounds__(kThreads) void find_mirror_kernel(uint8_t *__restrict__ X, uint32_t K_len, uint32_t with_rc,
                                                               uint8_t s0, uint8_t s1, uint32_t *__restrict__ bad) {
    const uint64_t gid = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (gid > K_len) return;
    const uint32_t i = (uint32_t)gid;
    if (i == K_len) {
        X[K_len] = s0;
        if (with_rc) X[2ull * K_len + 1] = s1;
        return;
    }
    const uint32_t c = complement(X[K_len - 1 - i]);
    if (c == 0) *bad = 1u;
    if (with_rc) X[(uint64_t)K_len + 1 + i] = (uint8_t)c;
}

// ---- source table ------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void source_of(const ArchiveRec &f, uint32_t &lo, uint32_t &hi) {
    const uint32_t kind = f.meta & 3u;
    if (kind == kArchiveLiteral) {
        lo = hi = 0;
    } else if (kind == kArchiveRc) {  // src is the source of byte 0, the last byte of the interval
        lo = f.src + 1u - f.length;
        hi = f.src + 1u;
    } else {
        lo = f.src;
        hi = f.src + f.length;
    }
}

__global__ __launch_bounds__(kThreads) void find_source_keys_kernel(const ArchiveRec *__restrict__ recs, uint32_t z,
                                                                    uint64_t *__restrict__ keys, uint32_t *__restrict__ vals) {
    const uint64_t gid = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (gid >= z) return;
    uint32_t lo, hi;
    source_of(recs[gid], lo, hi);
    keys[gid] = lo;
    vals[gid] = (uint32_t)gid;
}

__global__ __launch_bounds__(kThreads) void find_source_table_kernel(const ArchiveRec *__restrict__ recs, uint32_t z,
                                                                     const uint32_t *__restrict__ order,
                                                                     uint32_t *__restrict__ lo, uint32_t *__restrict__ hi,
                                                                     uint32_t *__restrict__ rec) {
    const uint64_t gid = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (gid >= z) return;
    uint32_t r = order[gid];
    r = r < z ? r : z - 1;  // (a record index by construction)
    uint32_t l, h;
    source_of(recs[r], l, h);
    lo[gid] = l;
    hi[gid] = h;
    rec[gid] = r;
}

// ---- query -------------------------------------------------------------------------------------------------------------
// pattern j of the batch P1 s P2 s .. Pq s (rlz_locate.hip): its length from the terminator table
__device__ __forceinline__ uint32_t pattern_length(const uint32_t *__restrict__ tpos, uint32_t j) {
    const uint32_t p = j ? tpos[j - 1] + 1u : 0u;
    return tpos[j] - p;
}

struct HitKey {
    uint32_t j, x, strand;
};
__device__ __forceinline__ HitKey unpack_hit(uint64_t key) {
    return HitKey{(uint32_t)(key >> 33), (uint32_t)((key >> 1) & 0xffffffffull), (uint32_t)(key & 1ull)};
}

// where pattern j's occurrences go, and whether it is reported at all
__device__ __forceinline__ bool reported(const FindEmit &e, uint32_t j) { return e.out_off[j + 1] > e.out_off[j]; }

// One lane per block hit (x, strand) of pattern j.  The walk: r = the last table entry with lo <= x; the nearest entry
// at or left of r with hi > x + m - 1 covers the hit; go on left of it.  At most z + 1 queries.
template <bool kEmit>
__global__ __launch_bounds__(kThreads) void find_secondary_kernel(FinderView f, ArchiveView v,
                                                                  const uint64_t *__restrict__ hits, uint32_t T,
                                                                  const uint32_t *__restrict__ tpos,
                                                                  uint32_t *__restrict__ cnt, FindEmit e) {
    const uint64_t gid = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (gid >= T) return;
    const uint32_t t = (uint32_t)gid;
    const HitKey h = unpack_hit(hits[t]);
    const uint32_t m = pattern_length(tpos, h.j);
    uint32_t at = 0, end = 0;
    if (kEmit) {
        if (!reported(e, h.j)) return;
        at = e.out_off[h.j] + (uint32_t)(e.scanS[t] - e.scanS[e.offS[h.j]]);
        end = e.out_off[h.j + 1] < e.total ? e.out_off[h.j + 1] : e.total;
    }
    uint32_t count = 0;
    int64_t r = (int64_t)upper_bound_u32(f.lo, f.z, h.x) - 1;
    for (uint32_t step = 0; step <= f.z && r >= 0 && m; ++step) {
        const int64_t c = pyr_nearest_left<true>(f.Phi, (uint32_t)r, h.x + m - 1u);
        if (c < 0) break;
        if (kEmit) {
            const uint32_t ci = (uint32_t)c;
            uint32_t ri = f.rec[ci];
            ri = ri < v.z ? ri : v.z - 1;  // (a record index by construction)
            const ArchiveRec R = archive_load_record(v, ri);
            const bool rc = (R.meta & 3u) == kArchiveRc;
            const uint32_t pos = rc ? R.start + (f.hi[ci] - h.x - m) : R.start + (h.x - f.lo[ci]);
            const uint32_t strand = rc ? h.strand ^ 1u : h.strand;
            if (at + count < end) {
                e.keys[at + count] = ((uint64_t)h.j << 33) | ((uint64_t)pos << 1) | strand;
                e.vals[at + count] = 0u;
            }
        }
        ++count;
        r = c - 1;
    }
    if (!kEmit) cnt[t] = count;
}

// One lane per kernel hit (kp, strand) of pattern j: inside one interval, back to decoded coordinates, and primary iff
// the record that covers its first byte is a literal or ends before the hit does.
template <bool kEmit>
__global__ __launch_bounds__(kThreads) void find_primary_kernel(FinderView f, ArchiveView v,
                                                                const uint64_t *__restrict__ hits, uint32_t T,
                                                                const uint32_t *__restrict__ tpos,
                                                                uint32_t *__restrict__ cnt, FindEmit e) {
    const uint64_t gid = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (gid >= T) return;
    const uint32_t t = (uint32_t)gid;
    const HitKey h = unpack_hit(hits[t]);
    const uint32_t m = pattern_length(tpos, h.j);
    if (kEmit && !reported(e, h.j)) return;
    bool keep = false;
    uint32_t p = 0;
    const uint32_t i1 = upper_bound_u32(f.kstart, f.nI, h.x);  // kstart[0] = 0 <= x: i1 >= 1
    if (i1 && m) {
        const uint32_t i = i1 - 1u;
        const uint32_t k0 = f.kstart[i], k1 = f.kstart[i + 1];
        if (h.x >= k0 && (uint64_t)h.x + m <= k1) {  // (an occurrence that runs over the interval's end is none)
            p = f.dstart[i] + (h.x - k0);
            if (p < f.dstart[f.nI]) {
                const ArchiveRec R = archive_load_record(v, archive_find_record(v, p));
                keep = (R.meta & 3u) == kArchiveLiteral || (uint64_t)p + m > (uint64_t)R.start + R.length;
            }
        }
    }
    if (!kEmit) {
        cnt[t] = keep ? 1u : 0u;
        return;
    }
    if (!keep) return;
    const uint32_t secondary = (uint32_t)(e.scanS[e.offS[h.j + 1]] - e.scanS[e.offS[h.j]]);
    const uint32_t at = e.out_off[h.j] + secondary + (uint32_t)(e.scanP[t] - e.scanP[e.offP[h.j]]);
    const uint32_t end = e.out_off[h.j + 1] < e.total ? e.out_off[h.j + 1] : e.total;
    if (at < end) {
        e.keys[at] = ((uint64_t)h.j << 33) | ((uint64_t)p << 1) | h.strand;
        e.vals[at] = 1u;
    }
}

// ---- the 64-bit scan: reduce, scan the tile sums, scan the tiles -------------------------------------------------------
constexpr uint32_t kScanItems = 8;
constexpr uint32_t kScanTile = kThreads * kScanItems;

// exclusive scan of one value per thread over the workgroup; *total = their sum
__device__ __forceinline__ uint64_t block_exclusive_u64(uint64_t v, uint64_t *lds, uint64_t *total) {
    const uint32_t tid = threadIdx.x;
    lds[tid] = v;
    __syncthreads();
    for (uint32_t d = 1; d < (uint32_t)kThreads; d <<= 1) {  // 8 steps
        const uint64_t add = tid >= d ? lds[tid - d] : 0ull;
        __syncthreads();
        lds[tid] += add;
        __syncthreads();
    }
    const uint64_t incl = lds[tid];
    *total = lds[kThreads - 1];
    __syncthreads();
    return incl - v;
}

__global__ __launch_bounds__(kThreads) void find_scan_reduce_kernel(const uint32_t *__restrict__ in, uint32_t n,
                                                                    uint64_t *__restrict__ sums) {
    __shared__ uint64_t lds[kThreads];
    const uint64_t base = (uint64_t)blockIdx.x * kScanTile + (uint64_t)threadIdx.x * kScanItems;
    uint64_t v = 0;
    for (uint32_t i = 0; i < kScanItems; ++i)
        if (base + i < n) v += in[base + i];
    uint64_t total;
    block_exclusive_u64(v, lds, &total);
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

// one workgroup: sums[0 .. nb) -> their exclusive scan in place, kThreads entries per step
__global__ __launch_bounds__(kThreads) void find_scan_sums_kernel(uint64_t *__restrict__ sums, uint32_t nb) {
    __shared__ uint64_t lds[kThreads];
    uint64_t carry = 0;
    for (uint32_t base = 0; base < nb; base += kThreads) {
        const uint32_t i = base + threadIdx.x;
        const uint64_t v = i < nb ? sums[i] : 0ull;
        uint64_t total;
        const uint64_t ex = block_exclusive_u64(v, lds, &total);
        if (i < nb) sums[i] = carry + ex;
        carry += total;
    }
}

// out[i] for i < n, and out[n] = the grand total (written by the lane that owns item n - 1, or by lane 0 when n = 0)
__global__ __launch_bounds__(kThreads) void find_scan_tiles_kernel(const uint32_t *__restrict__ in, uint32_t n,
                                                                   const uint64_t *__restrict__ sums,
                                                                   uint64_t *__restrict__ out) {
    __shared__ uint64_t lds[kThreads];
    const uint64_t base = (uint64_t)blockIdx.x * kScanTile + (uint64_t)threadIdx.x * kScanItems;
    uint32_t x[kScanItems];
    uint64_t v = 0;
    for (uint32_t i = 0; i < kScanItems; ++i) {
        x[i] = base + i < n ? in[base + i] : 0u;
        v += x[i];
    }
    uint64_t total;
    uint64_t run = sums[blockIdx.x] + block_exclusive_u64(v, lds, &total);
    for (uint32_t i = 0; i < kScanItems; ++i) {
        if (base + i < n) out[base + i] = run;
        run += x[i];
        if (base + i + 1 == n) out[n] = run;
    }
}

__global__ __launch_bounds__(kThreads) void find_pattern_counts_kernel(const uint64_t *__restrict__ scanS,
                                                                       const uint32_t *__restrict__ offS,
                                                                       const uint64_t *__restrict__ scanP,
                                                                       const uint32_t *__restrict__ offP, uint32_t q,
                                                                       uint64_t *__restrict__ counts) {
    const uint64_t j = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (j >= q) return;
    counts[j] = (scanS[offS[j + 1]] - scanS[offS[j]]) + (scanP[offP[j + 1]] - scanP[offP[j]]);
}

__global__ __launch_bounds__(kThreads) void find_hit_records_kernel(FinderView f, const uint64_t *__restrict__ keys,
                                                                    const uint32_t *__restrict__ vals, uint32_t count,
                                                                    TargetHit *__restrict__ out) {
    const uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= count) return;
    const uint64_t key = keys[i];
    const uint32_t p = (uint32_t)((key >> 1) & 0xffffffffull);
    uint32_t j = upper_bound_u32(f.bases, f.k + 1, p);  // the last target that starts at or below p: it is not empty
    j = j ? j - 1 : 0;
    j = j < f.k ? j : f.k - 1;
    TargetHit h;
    h.target = j;
    h.position = p - f.bases[j];
    h.is_rc = (uint32_t)(key & 1ull);
    h.primary = vals[i];
    out[i] = h;
}

unsigned blocks_for(size_t items) { return (unsigned)div_up(items, (size_t)kThreads); }

int bits_of(uint64_t v) {
    int b = 0;
    while (v >> b) ++b;
    return b;
}

}  // namespace

uint32_t find_intervals(Context &ctx, const ArchiveView &v, const uint32_t *d_bases, uint32_t k, uint32_t W,
                        uint32_t *d_kstart, uint32_t *d_dstart, uint32_t *K_len) {
    const uint32_t z = v.z;
    hipStream_t s = ctx.stream;
    ArenaRewind rewind(ctx.arena);
    ProfScope ps(ctx.profiler(), "rlz_find_intervals", s, 40.0 * (double)z);
    uint32_t *flag = ctx.arena.alloc<uint32_t>(z), *slot = ctx.arena.alloc<uint32_t>(z);
    uint32_t *dend = ctx.arena.alloc<uint32_t>(z), *len = ctx.arena.alloc<uint32_t>((size_t)z + 1);
    uint32_t *d_total = ctx.arena.alloc<uint32_t>(1);
    find_flags_kernel<<<blocks_for(z), kThreads, 0, s>>>(v.recs, z, d_bases, k, W, flag);
    KERNEL_CHECK();
    scan_exclusive_add_u32(flag, slot, z, d_total, ctx.arena, s);
    uint32_t nI = 0;
    ctx.read_back(d_total, &nI, 1);
    if (nI == 0 || nI > z) throw HipError("rlz finder: the intervals of the record starts are laid out wrongly");
    find_bounds_kernel<<<blocks_for(z), kThreads, 0, s>>>(v.recs, z, d_bases, k, W, flag, slot, nI, d_dstart, dend);
    KERNEL_CHECK();
    uint32_t decoded = 0;
    HIP_CHECK(hipMemcpyAsync(&decoded, d_bases + k, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    find_lengths_kernel<<<blocks_for((size_t)nI + 1), kThreads, 0, s>>>(d_dstart, dend, nI, decoded, len);
    KERNEL_CHECK();
    scan_exclusive_add_u32(len, d_kstart, (size_t)nI + 1, nullptr, ctx.arena, s);
    ctx.read_back(d_kstart + nI, K_len, 1);
    return nI;
}

void find_kernel_text(Context &ctx, const ArchiveView &v, const uint32_t *d_kstart, const uint32_t *d_dstart, uint32_t nI,
                      uint32_t K_len, bool with_rc, uint8_t s0, uint8_t s1, uint8_t *d_X) {
    hipStream_t s = ctx.stream;
    ArenaRewind rewind(ctx.arena);
    ProfScope ps(ctx.profiler(), "rlz_find_kernel_text", s, (with_rc ? 3.0 : 1.0) * (double)K_len);
    unsigned long long *d_err = ctx.arena.alloc<unsigned long long>(1);
    uint32_t *d_bad = ctx.arena.alloc<uint32_t>(1);
    HIP_CHECK(hipMemsetAsync(d_err, 0xff, sizeof(unsigned long long), s));
    HIP_CHECK(hipMemsetAsync(d_bad, 0, sizeof(uint32_t), s));
    archive_extract(ctx, v, d_kstart, d_dstart, nI, K_len, d_X, d_err);
    find_mirror_kernel<<<blocks_for((size_t)K_len + 1), kThreads, 0, s>>>(d_X, K_len, with_rc ? 1u : 0u, s0, s1, d_bad);
    KERNEL_CHECK();
    uint32_t e[2], bad = 0;
    ctx.read_back(reinterpret_cast<const uint32_t *>(d_err), e, 2);
    ctx.read_back(d_bad, &bad, 1);
    if ((e[0] & e[1]) != 0xffffffffu || bad)
        throw HipError("rlz finder: the targets of the archive hold a byte that is not a nucleotide");
}

SourceTable find_source_table(Context &ctx, const ArchiveView &v, uint32_t block_len) {
    const uint32_t z = v.z;
    hipStream_t s = ctx.stream;
    SourceTable t;
    t.lo = ctx.arena.alloc<uint32_t>(z);
    t.hi = ctx.arena.alloc<uint32_t>(z);
    t.rec = ctx.arena.alloc<uint32_t>(z);
    {
        ArenaRewind rewind(ctx.arena);
        ProfScope ps(ctx.profiler(), "rlz_find_source_table", s, 64.0 * (double)z);
        uint64_t *keys[2] = {ctx.arena.alloc<uint64_t>(z), ctx.arena.alloc<uint64_t>(z)};
        uint32_t *vals[2] = {ctx.arena.alloc<uint32_t>(z), ctx.arena.alloc<uint32_t>(z)};
        find_source_keys_kernel<<<blocks_for(z), kThreads, 0, s>>>(v.recs, z, keys[0], vals[0]);
        KERNEL_CHECK();
        int shifts[4], npasses = 0;  // lo < block_len < 2^32: the digits that can differ
        for (int b = 0; b < bits_of(block_len) && npasses < 4; b += kRadixBits) shifts[npasses++] = b;
        if (npasses == 0) shifts[npasses++] = 0;
        // the sort is stable and the pairs go in by record index: equal lo stay in that order
        const int at = radix_sort_pairs(keys, vals, z, shifts, npasses, ctx.arena, s, ctx.profiler());
        find_source_table_kernel<<<blocks_for(z), kThreads, 0, s>>>(v.recs, z, vals[at], t.lo, t.hi, t.rec);
        KERNEL_CHECK();
    }
    t.Phi = build_pyramid(t.hi, z, true, ctx.arena, s);
    return t;
}

void find_secondary_count(Context &ctx, const FinderView &f, const uint64_t *d_hits, uint32_t T, const uint32_t *d_tpos,
                          uint32_t *d_cnt) {
    if (T == 0) return;
    ProfScope ps(ctx.profiler(), "rlz_find_walk_count", ctx.stream);
    find_secondary_kernel<false><<<blocks_for(T), kThreads, 0, ctx.stream>>>(f, ArchiveView{}, d_hits, T, d_tpos, d_cnt, FindEmit{});
    KERNEL_CHECK();
}

void find_secondary_emit(Context &ctx, const FinderView &f, const ArchiveView &v, const uint64_t *d_hits, uint32_t T,
                         const uint32_t *d_tpos, const FindEmit &e) {
    if (T == 0) return;
    ProfScope ps(ctx.profiler(), "rlz_find_walk_emit", ctx.stream);
    find_secondary_kernel<true><<<blocks_for(T), kThreads, 0, ctx.stream>>>(f, v, d_hits, T, d_tpos, nullptr, e);
    KERNEL_CHECK();
}

void find_primary_count(Context &ctx, const FinderView &f, const ArchiveView &v, const uint64_t *d_hits, uint32_t T,
                        const uint32_t *d_tpos, uint32_t *d_cnt) {
    if (T == 0) return;
    ProfScope ps(ctx.profiler(), "rlz_find_primary_count", ctx.stream, 28.0 * (double)T);
    find_primary_kernel<false><<<blocks_for(T), kThreads, 0, ctx.stream>>>(f, v, d_hits, T, d_tpos, d_cnt, FindEmit{});
    KERNEL_CHECK();
}

void find_primary_emit(Context &ctx, const FinderView &f, const ArchiveView &v, const uint64_t *d_hits, uint32_t T,
                       const uint32_t *d_tpos, const FindEmit &e) {
    if (T == 0) return;
    ProfScope ps(ctx.profiler(), "rlz_find_primary_emit", ctx.stream, 40.0 * (double)T);
    find_primary_kernel<true><<<blocks_for(T), kThreads, 0, ctx.stream>>>(f, v, d_hits, T, d_tpos, nullptr, e);
    KERNEL_CHECK();
}

void find_scan_u64(Context &ctx, const uint32_t *d_in, uint32_t n, uint64_t *d_out) {
    hipStream_t s = ctx.stream;
    if (n == 0) {
        HIP_CHECK(hipMemsetAsync(d_out, 0, sizeof(uint64_t), s));
        return;
    }
    ArenaRewind rewind(ctx.arena);
    ProfScope ps(ctx.profiler(), "rlz_find_scan", s, 16.0 * (double)n);
    const uint32_t nb = (uint32_t)div_up((size_t)n, (size_t)kScanTile);
    uint64_t *sums = ctx.arena.alloc<uint64_t>(nb);
    find_scan_reduce_kernel<<<nb, kThreads, 0, s>>>(d_in, n, sums);
    KERNEL_CHECK();
    find_scan_sums_kernel<<<1, kThreads, 0, s>>>(sums, nb);
    KERNEL_CHECK();
    find_scan_tiles_kernel<<<nb, kThreads, 0, s>>>(d_in, n, sums, d_out);
    KERNEL_CHECK();
}

void find_pattern_counts(Context &ctx, const uint64_t *d_scanS, const uint32_t *d_offS, const uint64_t *d_scanP,
                         const uint32_t *d_offP, uint32_t q, uint64_t *d_counts) {
    if (q == 0) return;
    ProfScope ps(ctx.profiler(), "rlz_find_counts", ctx.stream, 56.0 * (double)q);
    find_pattern_counts_kernel<<<blocks_for(q), kThreads, 0, ctx.stream>>>(d_scanS, d_offS, d_scanP, d_offP, q, d_counts);
    KERNEL_CHECK();
}

void find_hit_records(Context &ctx, const FinderView &f, const uint64_t *d_keys, const uint32_t *d_vals, uint32_t count,
                      TargetHit *d_out) {
    if (count == 0) return;
    ProfScope ps(ctx.profiler(), "rlz_find_hit_records", ctx.stream, 36.0 * (double)count);
    find_hit_records_kernel<<<blocks_for(count), kThreads, 0, ctx.stream>>>(f, d_keys, d_vals, count, d_out);
    KERNEL_CHECK();
}

}  // namespace nolzss
