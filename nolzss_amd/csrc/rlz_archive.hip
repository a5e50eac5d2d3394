// rlz_archive.hip -- the relative-LZ archive: the record check, the resident form, the position sample and the range
// extraction ("Relative-LZ archive: ranges from resident records"; semantics: include/nolzss_hip.h,
// nolzss_rlz_archive_*).
//
// Every copy points into the reference block, so output byte x of range i is one search and one gathered byte:
//     range    i = the last range with offsets[i] <= x                    (upper-bound search: empty ranges are skipped)
//     position p = first[i] + (x - offsets[i])                            (decoded coordinates: behind the block)
//     record   k = the last record with start <= p                        (search between two entries of the sample)
//     byte       = block[src + t] | comp(block[src - t]) | the folded symbol,  t = p - start[k]
// Every loop is bounded by the call's shape and not by its data: log2(q + 1) steps per range search, at most 9 steps per
// record search (two neighbouring sample entries are at most 256 records apart: every record has a base), 16 bytes
// per lane.  No spinning, no communication between lanes; the only atomic is the error atomicMin.
#include "rlz_archive.hpp"

namespace nolzss {
namespace {

constexpr int kThreads = 256;
constexpr uint32_t kChunk = 16;  // output bytes of one lane

__device__ __forceinline__ uint32_t complement(uint32_t c) {  // 0: not a nucleotide
    return c == 'A' ? 'T' : c == 'T' ? 'A' : c == 'C' ? 'G' : c == 'G' ? 'C' : 0u;
}

__device__ __forceinline__ bool is_literal(const Rec &f) { return f.ref == f.start; }

// ctl[0]: (record index << 3 | rule) of the first offending record, atomicMin; ctl[1]: literal records
__global__ __launch_bounds__(kThreads) void archive_check_kernel(const Rec *__restrict__ recs, uint64_t z,
                                                                 uint64_t block_len, uint64_t n,
                                                                 const uint64_t *__restrict__ bounds, uint32_t k,
                                                                 uint32_t *__restrict__ flags,
                                                                 unsigned long long *__restrict__ ctl) {
    unsigned long long bad = ~0ull, literals = 0;
    const uint64_t stride = (uint64_t)gridDim.x * kThreads;
    for (uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x; i < z; i += stride) {
        const Rec f = recs[i];
        uint64_t expect = block_len;
        if (i) {
            const Rec p = recs[i - 1];
            expect = p.start + p.length;
        }
        uint32_t rule = kDecodeOk;
        const bool lit = is_literal(f);
        const uint64_t r = f.ref & ~kRcMask;
        if (f.start != expect || f.length == 0 || f.start > n || f.length > n - f.start ||
            (i == z - 1 && f.length != n - f.start))
            rule = kDecodeTiling;
        else if (lit && f.length != 1) rule = kDecodeLiteralLength;
        else if (!lit && (r > block_len || f.length > block_len - r)) rule = kDecodeSourceInBlock;
        else {
            // the first boundary behind start ends the target the record lies in (empty targets repeat a boundary)
            uint32_t lo = 0, hi = k + 1;  // bounds[0 .. lo) <= start
            while (lo < hi) {
                const uint32_t mid = lo + ((hi - lo) >> 1);
                if (bounds[mid] <= f.start) lo = mid + 1;
                else hi = mid;
            }
            if (lo > k || f.length > bounds[lo] - f.start) rule = kDecodeTargetBoundary;
        }
        if (rule != kDecodeOk) {
            const unsigned long long key = (i << 3) | rule;
            bad = key < bad ? key : bad;
        }
        flags[i] = lit ? 1u : 0u;
        literals += lit ? 1u : 0u;
    }
    if (bad != ~0ull) atomicMin(&ctl[0], bad);
    if (literals) atomicAdd(&ctl[1], literals);
}

// lit_index: the exclusive add-scan of the literal flags
__global__ __launch_bounds__(kThreads) void archive_pack_kernel(const Rec *__restrict__ recs, uint64_t z,
                                                                uint64_t block_len,
                                                                const uint32_t *__restrict__ lit_index,
                                                                const uint8_t *__restrict__ literals,
                                                                ArchiveRec *__restrict__ out) {
    const uint64_t stride = (uint64_t)gridDim.x * kThreads;
    for (uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x; i < z; i += stride) {
        const Rec f = recs[i];
        ArchiveRec a;
        a.start = (uint32_t)(f.start - block_len);
        a.length = (uint32_t)f.length;
        if (is_literal(f)) {
            a.src = 0;
            a.meta = kArchiveLiteral | ((uint32_t)literals[lit_index[i]] << 8);
        } else if (f.ref & kRcMask) {
            a.src = (uint32_t)((f.ref & ~kRcMask) + f.length - 1);
            a.meta = kArchiveRc;
        } else {
            a.src = (uint32_t)f.ref;
            a.meta = kArchiveForward;
        }
        out[i] = a;
    }
}

// sample[s] = the last record with start <= 256 * s
__global__ __launch_bounds__(kThreads) void archive_sample_kernel(const ArchiveRec *__restrict__ recs, uint32_t z,
                                                                  uint32_t samples, uint32_t *__restrict__ sample) {
    const uint32_t s = blockIdx.x * kThreads + threadIdx.x;
    if (s >= samples) return;
    const uint32_t p = s << kSampleShift;
    uint32_t lo = 0, hi = z;  // recs[lo].start <= p (record 0 starts at 0), recs[hi].start > p or hi == z
    while (hi - lo > 1) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (recs[mid].start <= p) lo = mid;
        else hi = mid;
    }
    sample[s] = lo;
}

// the last range i in [lo, q) with offsets[i] <= x; offsets[lo] <= x < offsets[q].  offsets[i + 1] > x: range i is not empty
__device__ __forceinline__ uint32_t find_range(const uint32_t *__restrict__ offsets, uint32_t q, uint32_t x, uint32_t lo) {
    uint32_t hi = q;
    while (hi - lo > 1) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (offsets[mid] <= x) lo = mid;
        else hi = mid;
    }
    return lo;
}

// One lane owns output bytes [16 g, 16 g + 16) of the call; wide: d_out is 16-byte aligned, a whole chunk goes out as
// one 16-byte store.
__global__ __launch_bounds__(kThreads) void rlz_extract_kernel(ArchiveView v, const uint32_t *__restrict__ offsets,
                                                               const uint32_t *__restrict__ first, uint32_t q,
                                                               uint32_t total, uint8_t *__restrict__ out, uint32_t wide,
                                                               unsigned long long *__restrict__ err) {
    const uint64_t at = ((uint64_t)blockIdx.x * kThreads + threadIdx.x) * kChunk;
    if (at >= total) return;
    const uint32_t o = (uint32_t)at;
    const uint32_t count = total - o < kChunk ? total - o : kChunk;

    uint32_t i = find_range(offsets, q, o, 0);
    uint32_t range_begin = offsets[i], range_end = offsets[i + 1];
    uint32_t k = archive_find_record(v, first[i] + (o - range_begin));
    ArchiveRec f = archive_load_record(v, k);
    uint32_t t = first[i] + (o - range_begin) - f.start;
    unsigned long long w0 = 0, w1 = 0;
    // A whole chunk inside one range and one copy record: its 16 source bytes are contiguous in the block, one
    // (unaligned) 16-byte load.  A reverse-complement chunk with a non-nucleotide goes through the bytewise walk,
    // which reports the first one.
    bool done = false;
    if (count == kChunk && range_end - o >= kChunk && (f.meta & 3u) != kArchiveLiteral && f.length - t >= kChunk) {
        const bool rc = (f.meta & 3u) == kArchiveRc;
        ulonglong2 s;
        __builtin_memcpy(&s, v.block + (rc ? f.src - t - (kChunk - 1) : f.src + t), sizeof s);
        if (!rc) {
            w0 = s.x;
            w1 = s.y;
            done = true;
        } else {
            uint32_t valid = 1;
#pragma unroll
            for (uint32_t b = 0; b < kChunk; ++b) {  // output byte b = comp(source byte 15 - b)
                const uint32_t j = kChunk - 1 - b;
                const uint32_t c = complement((uint32_t)((j < 8 ? s.x >> (8 * j) : s.y >> (8 * (j - 8))) & 0xffu));
                valid &= c != 0 ? 1u : 0u;
                if (b < 8) w0 |= (unsigned long long)c << (8 * b);
                else w1 |= (unsigned long long)c << (8 * (b - 8));
            }
            done = valid != 0;
            if (!done) w0 = w1 = 0;
        }
    }
    for (uint32_t b = 0; !done && b < count; ++b) {
        const uint32_t x = o + b;
        if (x >= range_end) {
            // x < total = offsets[q] and x >= offsets[i + 1]: i + 2 <= q.  The next range unless it is empty.
            i = offsets[i + 2] > x ? i + 1 : find_range(offsets, q, x, i + 1);
            range_begin = offsets[i];
            range_end = offsets[i + 1];
            const uint32_t p = first[i] + (x - range_begin);
            k = archive_find_record(v, p);
            f = archive_load_record(v, k);
            t = p - f.start;
        } else if (t >= f.length) {  // inside a range the next position is the next record's first (tiling)
            f = archive_load_record(v, ++k);
            t = 0;
        }
        const uint32_t kind = f.meta & 3u;
        uint32_t c;
        if (kind == kArchiveLiteral) {
            c = (f.meta >> 8) & 0xffu;
        } else if (kind == kArchiveForward) {
            c = v.block[f.src + t];
        } else {
            c = complement(v.block[f.src - t]);
            if (c == 0) atomicMin(err, ((unsigned long long)i << 32) | (x - range_begin));
        }
        ++t;
        if (b < 8) w0 |= (unsigned long long)c << (8 * b);
        else w1 |= (unsigned long long)c << (8 * (b - 8));
    }
    if (wide && count == kChunk) {
        *reinterpret_cast<ulonglong2 *>(out + o) = make_ulonglong2(w0, w1);
    } else {
        for (uint32_t b = 0; b < count; ++b) out[o + b] = (uint8_t)((b < 8 ? w0 >> (8 * b) : w1 >> (8 * (b - 8))) & 0xffu);
    }
}

// ---- batches appended from the index, export ("Relative-LZ archive: batches appended from the index") ----
// Every kernel below is bounded by the call's shape: the separator search takes ceil(log2(k + 1)) steps, the sample
// search ceil(log2(new records)) steps, the terminator walk of the unpack at most 32.  No spinning, no communication
// between workgroups, no atomics (the literal count of an append is one ballot and one store per wavefront); every load stays inside the handle's arrays and the batch's (the indices are checked
// against the sizes the host passes, not trusted from the data).

// One lane per packed word of the index text: 32 bases -> 32 bytes of Rblk, the terminators below B as 0x01.
__global__ __launch_bounds__(kThreads) void archive_unpack_kernel(PackedText x, uint32_t B, uint8_t *__restrict__ block) {
    const uint64_t g = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    const uint64_t at = g * 32u;
    if (at >= B) return;
    const uint32_t p0 = (uint32_t)at;
    const uint32_t count = B - p0 < 32u ? B - p0 : 32u;
    const uint64_t w = x.words[g];
    // the terminators in [p0, p0 + count) as a bit mask: the table is ascending and its last entry is the end of the
    // text, >= B
    uint32_t seps = 0;
    uint32_t t = term_lower_bound(x.terms, p0);
    for (int step = 0; step < 32 && t < x.terms.count; ++step, ++t) {
        const uint32_t q = x.terms.pos[t];
        if (q >= p0 + count) break;
        seps |= 1u << (q - p0);
    }
    uint32_t out[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        uint32_t v = 0;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const uint32_t code = (uint32_t)(w >> (62 - 2 * (4 * q + e))) & 3u;
            uint32_t c = code == 0 ? 'A' : code == 1 ? 'C' : code == 2 ? 'G' : 'T';
            c = (seps >> (4 * q + e)) & 1u ? 1u : c;
            v |= c << (8 * e);
        }
        out[q] = v;
    }
    if (count == 32u) {  // (block is a device allocation: 32 g is 16-byte aligned)
        uint4 *dst = reinterpret_cast<uint4 *>(block + p0);
        dst[0] = make_uint4(out[0], out[1], out[2], out[3]);
        dst[1] = make_uint4(out[4], out[5], out[6], out[7]);
    } else {
#pragma unroll
        for (uint32_t b = 0; b < 32u; ++b)
            if (b < count) block[p0 + b] = (uint8_t)(out[b >> 2] >> (8 * (b & 3)));
    }
}

// One lane per look-up of the chunk.  lit_counts[blockIdx.x * 4 + wavefront]: the literal records this wavefront wrote
// (one store per wavefront, every wavefront of the grid writes its own word: the host adds them up).
__global__ __launch_bounds__(kThreads) void archive_append_kernel(const IndexRec *__restrict__ chunk,
                                                                  const uint32_t *__restrict__ fpos, uint32_t first,
                                                                  uint32_t cnt, uint64_t base, AppendBatch b,
                                                                  ArchiveRec *__restrict__ out,
                                                                  uint32_t *__restrict__ lit_counts) {
    const uint64_t t = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    bool literal = false;
    const uint32_t p = t < cnt ? fpos[t] : b.n;
    if (p < b.n) {  // (a factor start is a batch position)
        // j = the separators below p: at most ceil(log2(k + 1)) steps.  Adjacent separators are empty targets.
        uint32_t lo = 0, hi = b.k;  // seps[0 .. lo) < p <= seps[hi ..)
        while (lo < hi) {
            const uint32_t mid = lo + ((hi - lo) >> 1);
            if (b.seps[mid] < p) lo = mid + 1;
            else hi = mid;
        }
        const uint32_t j = lo;
        // every separator below p is a factor start below p: j <= first + t
        const uint64_t o = (uint64_t)b.z_old + first + t - j;
        if (!(j < b.k && b.seps[j] == p) && o < b.z_new) {  // (not the separator's own literal)
            const IndexRec f = chunk[t];
            ArchiveRec a;
            a.start = b.decoded_old + p - j;
            a.length = (uint32_t)f.length;
            if (f.ref == base + p) {
                a.src = 0;
                a.meta = kArchiveLiteral | ((uint32_t)b.text[p] << 8);
                literal = true;
            } else if (f.ref & kRcMask) {
                a.src = (uint32_t)((f.ref & ~kRcMask) + f.length - 1);
                a.meta = kArchiveRc;
            } else {
                a.src = (uint32_t)f.ref;
                a.meta = kArchiveForward;
            }
            reinterpret_cast<uint4 *>(out)[o] = make_uint4(a.start, a.length, a.src, a.meta);
        }
    }
    const unsigned long long lits = __ballot(literal);  // (all lanes are back together here)
    if ((threadIdx.x & (kWave - 1)) == 0) lit_counts[blockIdx.x * (kThreads / kWave) + threadIdx.x / kWave] = (uint32_t)__popcll(lits);
}

// sample[s] = the last record of [z_old, z_new) with start <= 256 s; recs[z_old].start <= 256 s for every s here
__global__ __launch_bounds__(kThreads) void archive_extend_sample_kernel(const ArchiveRec *__restrict__ recs, uint32_t z_old,
                                                                         uint32_t z_new, uint32_t s_lo, uint32_t s_hi,
                                                                         uint32_t *__restrict__ sample) {
    const uint64_t g = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (g >= s_hi - s_lo) return;
    const uint32_t s = s_lo + (uint32_t)g;
    const uint32_t p = s << kSampleShift;
    uint32_t lo = z_old, hi = z_new;
    while (hi - lo > 1) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (recs[mid].start <= p) lo = mid;
        else hi = mid;
    }
    sample[s] = lo;
}

__global__ __launch_bounds__(kThreads) void archive_literal_flags_kernel(const ArchiveRec *__restrict__ recs, uint64_t cnt,
                                                                         uint32_t *__restrict__ flags) {
    const uint64_t stride = (uint64_t)gridDim.x * kThreads;
    for (uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x; i < cnt; i += stride)
        flags[i] = (recs[i].meta & 3u) == kArchiveLiteral ? 1u : 0u;
}

// lit_index: the exclusive add-scan of the literal flags of ALL records; archive_pack_kernel the other way round
__global__ __launch_bounds__(kThreads) void archive_export_kernel(const ArchiveRec *__restrict__ recs, uint64_t first,
                                                                  uint64_t cnt, uint64_t block_len,
                                                                  const uint32_t *__restrict__ lit_index,
                                                                  Rec *__restrict__ out, uint8_t *__restrict__ literals) {
    const uint64_t stride = (uint64_t)gridDim.x * kThreads;
    for (uint64_t t = (uint64_t)blockIdx.x * kThreads + threadIdx.x; t < cnt; t += stride) {
        const uint4 w = reinterpret_cast<const uint4 *>(recs)[first + t];
        const ArchiveRec a{w.x, w.y, w.z, w.w};
        Rec f;
        f.start = block_len + a.start;
        f.length = a.length;
        const uint32_t kind = a.meta & 3u;
        if (kind == kArchiveLiteral) {
            f.ref = f.start;
            literals[lit_index[first + t]] = (uint8_t)((a.meta >> 8) & 0xffu);
        } else if (kind == kArchiveRc) {
            f.ref = ((uint64_t)a.src - (a.length - 1u)) | kRcMask;
        } else {
            f.ref = a.src;
        }
        out[t] = f;
    }
}

}  // namespace

void archive_unpack_block(Context &ctx, const PackedText &x, uint32_t B, uint8_t *d_block) {
    if (B == 0) return;
    ProfScope ps(ctx.profiler(), "rlz_archive_unpack", ctx.stream, 1.25 * (double)B);
    const uint64_t lanes = div_up((uint64_t)B, (uint64_t)32);
    archive_unpack_kernel<<<(unsigned)div_up(lanes, (uint64_t)kThreads), kThreads, 0, ctx.stream>>>(x, B, d_block);
    KERNEL_CHECK();
}

size_t archive_append_counts(size_t cnt) { return div_up(cnt, (size_t)kThreads) * (kThreads / kWave); }

void archive_append_records(Context &ctx, const IndexRec *d_chunk, const uint32_t *d_fpos, uint32_t first, uint32_t cnt,
                            uint64_t base, const AppendBatch &b, ArchiveRec *d_recs, uint32_t *d_lit_counts) {
    if (cnt == 0) return;
    ProfScope ps(ctx.profiler(), "rlz_append_records", ctx.stream, 45.0 * (double)cnt);
    archive_append_kernel<<<(unsigned)div_up((size_t)cnt, (size_t)kThreads), kThreads, 0, ctx.stream>>>(
        d_chunk, d_fpos, first, cnt, base, b, d_recs, d_lit_counts);
    KERNEL_CHECK();
}

void archive_extend_sample(Context &ctx, const ArchiveRec *d_recs, uint32_t z_old, uint32_t z_new, uint32_t s_lo,
                           uint32_t s_hi, uint32_t *d_sample) {
    if (s_hi <= s_lo || z_new <= z_old) return;
    ProfScope ps(ctx.profiler(), "rlz_append_sample", ctx.stream, 4.0 * (double)(s_hi - s_lo));
    archive_extend_sample_kernel<<<(unsigned)div_up((size_t)(s_hi - s_lo), (size_t)kThreads), kThreads, 0, ctx.stream>>>(
        d_recs, z_old, z_new, s_lo, s_hi, d_sample);
    KERNEL_CHECK();
}

uint64_t archive_literal_index(Context &ctx, const ArchiveRec *d_recs, size_t cnt, uint32_t *d_index) {
    if (cnt == 0) return 0;
    hipStream_t s = ctx.stream;
    const size_t mark = ctx.arena.mark();
    uint32_t *d_total = ctx.arena.alloc<uint32_t>(1);
    {
        ProfScope ps(ctx.profiler(), "rlz_archive_literal_index", s, 24.0 * (double)cnt);
        archive_literal_flags_kernel<<<record_grid(cnt), kThreads, 0, s>>>(d_recs, cnt, d_index);
        KERNEL_CHECK();
        scan_exclusive_add_u32(d_index, d_index, cnt, d_total, ctx.arena, s);
    }
    uint32_t total = 0;
    ctx.read_back(d_total, &total, 1);
    ctx.arena.rewind(mark);
    return total;
}

void archive_export_records(Context &ctx, const ArchiveRec *d_recs, size_t first, size_t cnt, uint64_t block_len,
                            const uint32_t *d_index, Rec *d_out, uint8_t *d_literals) {
    if (cnt == 0) return;
    ProfScope ps(ctx.profiler(), "rlz_archive_export", ctx.stream, 45.0 * (double)cnt);
    archive_export_kernel<<<record_grid(cnt), kThreads, 0, ctx.stream>>>(d_recs, first, cnt, block_len, d_index, d_out,
                                                                        d_literals);
    KERNEL_CHECK();
}

const char *archive_rule_text(uint32_t rule) {
    switch (rule) {
    case kDecodeTiling: return "tiling (start[0] = block_len, start[k + 1] = start[k] + length[k], length >= 1)";
    case kDecodeLiteralLength: return "literal length (a literal, ref == start, has length 1)";
    case kDecodeSourceInBlock:
        return "source inside the block (ref + length must not exceed block_len: every copy comes from the reference "
               "block; a self-referential factorisation has no one-hop random access, decode it with nolzss_decode)";
    case kDecodeTargetBoundary:
        return "target boundary (a record lies inside one target: it must not straddle the end of a target or lie behind "
               "the last one)";
    default: return "unknown rule";
    }
}

ArchiveCheck archive_check(Context &ctx, const Rec *d_recs, size_t z, uint64_t block_len, uint64_t n,
                           const uint64_t *d_bounds, size_t k, uint32_t *lit_flags) {
    Arena &arena = ctx.arena;
    hipStream_t s = ctx.stream;
    const size_t mark = arena.mark();
    unsigned long long *ctl = arena.alloc<unsigned long long>(2);
    HIP_CHECK(hipMemsetAsync(ctl, 0xff, sizeof(unsigned long long), s));
    HIP_CHECK(hipMemsetAsync(ctl + 1, 0, sizeof(unsigned long long), s));
    {
        ProfScope ps(ctx.profiler(), "rlz_archive_check", s, 28.0 * (double)z);
        archive_check_kernel<<<record_grid(z), kThreads, 0, s>>>(d_recs, z, block_len, n, d_bounds, (uint32_t)k, lit_flags,
                                                                  ctl);
        KERNEL_CHECK();
    }
    uint32_t h[4];
    ctx.read_back(reinterpret_cast<const uint32_t *>(ctl), h, 4);
    arena.rewind(mark);
    ArchiveCheck res;
    res.bad = (uint64_t)h[0] | ((uint64_t)h[1] << 32);
    res.literals = (uint64_t)h[2] | ((uint64_t)h[3] << 32);
    return res;
}

void archive_pack(Context &ctx, const Rec *d_recs, size_t z, uint64_t block_len, uint64_t n, uint32_t *lit_flags,
                  const uint8_t *d_literals, ArchiveRec *d_packed, uint32_t *d_sample) {
    hipStream_t s = ctx.stream;
    const size_t samples = archive_samples((size_t)(n - block_len));
    ProfScope ps(ctx.profiler(), "rlz_archive_pack", s, 44.0 * (double)z + 4.0 * (double)samples);
    scan_exclusive_add_u32(lit_flags, lit_flags, z, nullptr, ctx.arena, s);
    archive_pack_kernel<<<record_grid(z), kThreads, 0, s>>>(d_recs, z, block_len, lit_flags, d_literals, d_packed);
    KERNEL_CHECK();
    archive_sample_kernel<<<(unsigned)div_up(samples, (size_t)kThreads), kThreads, 0, s>>>(d_packed, (uint32_t)z,
                                                                                           (uint32_t)samples, d_sample);
    KERNEL_CHECK();
}

void archive_extract(Context &ctx, const ArchiveView &v, const uint32_t *d_offsets, const uint32_t *d_first, uint32_t q,
                     uint32_t total, uint8_t *d_out, unsigned long long *d_err) {
    hipStream_t s = ctx.stream;
    ProfScope ps(ctx.profiler(), "rlz_extract", s, 2.0 * (double)total + 8.0 * (double)q);
    const uint64_t lanes = div_up((uint64_t)total, (uint64_t)kChunk);
    const uint32_t wide = (reinterpret_cast<uintptr_t>(d_out) & 15) == 0 ? 1u : 0u;
    rlz_extract_kernel<<<(unsigned)div_up(lanes, (uint64_t)kThreads), kThreads, 0, s>>>(v, d_offsets, d_first, q, total, d_out,
                                                                                        wide, d_err);
    KERNEL_CHECK();
}

}  // namespace nolzss
