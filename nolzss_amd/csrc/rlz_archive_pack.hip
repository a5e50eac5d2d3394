// rlz_archive_pack.hip -- the compact container of a relative-LZ archive: the resident records packed into control
// nibbles, data bytes and 2-bit symbols, and expanded again with every rule of the format checked (DESIGN.md 5,
// "Relative-LZ archive: the compact container"; the format: include/nolzss_hip.h, nolzss_rlz_archive_pack).
//
// A copy is coded by its length and by the step of its diagonal g = y - p from the copy before it, y the mirrored
// source coordinate in which a reverse-complement match reads forward.  Which copy comes before it is a rank (an
// exclusive scan of the copy flags), where a record's bytes go is an offset (an exclusive scan of the byte counts), and
// the way back turns the steps into diagonals with one more scan: everything is scan_exclusive_add_u32 and kernels of
// one lane per record, per pair of records or per output byte.
// Every loop is bounded by the format and not by the data: at most 4 length bytes and 5 code bytes per record, 4 symbols
// per packed byte, ceil(log2(k + 1)) steps of the target search, 8 steps of a workgroup's sum.  No spinning, no
// communication between workgroups; the only atomic is the atomicMin on the error word of an unpack.  Every read of an
// uploaded section is bounded by the section's size, which the host has checked, and never by what the section says.
#include "rlz_archive_pack.hpp"

namespace nolzss {
namespace {

constexpr int kThreads = 256;

__device__ __forceinline__ uint32_t base_code(uint32_t c) {  // 4: not a nucleotide
    return c == 'A' ? 0u : c == 'C' ? 1u : c == 'G' ? 2u : c == 'T' ? 3u : 4u;
}
__device__ __forceinline__ uint32_t code_base(uint32_t code) {
    return code == 0 ? 'A' : code == 1 ? 'C' : code == 2 ? 'G' : 'T';
}
__device__ __forceinline__ uint32_t length_bytes(uint32_t a) { return a == 3 ? 4u : a; }       // 0, 1, 2, 4
__device__ __forceinline__ uint32_t code_bytes(uint32_t b) { return b == 0 ? 0u : 2u * b - 1u; }  // 0, 1, 3, 5

// partial[blockIdx.x] = the sum of this workgroup's share of in[0 .. n), exact in 64 bits
__global__ __launch_bounds__(kThreads) void sum_u32_kernel(const uint32_t *__restrict__ in, uint64_t n,
                                                          unsigned long long *__restrict__ partial) {
    __shared__ unsigned long long s[kThreads];
    unsigned long long acc = 0;
    const uint64_t stride = (uint64_t)gridDim.x * kThreads;
    for (uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += stride) acc += in[i];
    s[threadIdx.x] = acc;
    __syncthreads();
    for (int half = kThreads / 2; half > 0; half >>= 1) {
        if ((int)threadIdx.x < half) s[threadIdx.x] += s[threadIdx.x + half];
        __syncthreads();
    }
    if (threadIdx.x == 0) partial[blockIdx.x] = s[0];
}

// one workgroup: *out = the sum of partial[0 .. count)
__global__ __launch_bounds__(kThreads) void sum_u64_kernel(const unsigned long long *__restrict__ partial, uint32_t count,
                                                          unsigned long long *__restrict__ out) {
    __shared__ unsigned long long s[kThreads];
    unsigned long long acc = 0;
    for (uint32_t i = threadIdx.x; i < count; i += kThreads) acc += partial[i];
    s[threadIdx.x] = acc;
    __syncthreads();
    for (int half = kThreads / 2; half > 0; half >>= 1) {
        if ((int)threadIdx.x < half) s[threadIdx.x] += s[threadIdx.x + half];
        __syncthreads();
    }
    if (threadIdx.x == 0) *out = s[0];
}

// *d_out (one 64-bit word of the arena) = sum of d_in[0 .. n), on the stream
void sum_u32(Context &ctx, const uint32_t *d_in, size_t n, unsigned long long *d_out) {
    const size_t mark = ctx.arena.mark();
    const unsigned grid = record_grid(n);
    unsigned long long *partial = ctx.arena.alloc<unsigned long long>(grid);
    sum_u32_kernel<<<grid, kThreads, 0, ctx.stream>>>(d_in, n, partial);
    KERNEL_CHECK();
    sum_u64_kernel<<<1, kThreads, 0, ctx.stream>>>(partial, grid, d_out);
    KERNEL_CHECK();
    ctx.arena.rewind(mark);  // (the stream orders whatever takes the words next behind the two launches)
}

// ---- pack ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void pack_copy_flags_kernel(const ArchiveRec *__restrict__ recs, uint64_t z,
                                                                  uint32_t *__restrict__ flags) {
    const uint64_t stride = (uint64_t)gridDim.x * kThreads;
    for (uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x; i < z; i += stride)
        flags[i] = (recs[i].meta & 3u) == kArchiveLiteral ? 0u : 1u;
}

// diag[rank[i]] = (g, r) of copy i: r the strand, g = y - p with y = x (forward) or 2 B + 1 - x - L (reverse complement)
__global__ __launch_bounds__(kThreads) void pack_diagonals_kernel(const ArchiveRec *__restrict__ recs, uint64_t z, uint32_t B,
                                                                 const uint32_t *__restrict__ rank, uint64_t copies,
                                                                 uint2 *__restrict__ diag) {
    const uint64_t stride = (uint64_t)gridDim.x * kThreads;
    for (uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x; i < z; i += stride) {
        const uint4 w = reinterpret_cast<const uint4 *>(recs)[i];
        const uint32_t kind = w.w & 3u;
        if (kind == kArchiveLiteral) continue;
        const uint32_t r = kind == kArchiveRc ? 1u : 0u;
        const uint32_t x = r ? w.z - (w.y - 1u) : w.z;  // (the resident src of an RC record is ref + length - 1)
        const uint32_t y = r ? 2u * B + 1u - x - w.y : x;
        if (rank[i] < copies) diag[rank[i]] = make_uint2(y - w.x, r);  // (packed_plan has checked the count)
    }
}

struct RecordCode {
    uint32_t nibble, length, length_count, code_count;
    unsigned long long v;
};
__device__ __forceinline__ RecordCode record_code(const ArchiveRec *__restrict__ recs, const uint32_t *__restrict__ rank,
                                                  const uint2 *__restrict__ diag, uint64_t i) {
    const uint4 w = reinterpret_cast<const uint4 *>(recs)[i];
    RecordCode c{0u, w.y, 0u, 0u, 0ull};
    if ((w.w & 3u) == kArchiveLiteral) return c;
    const uint32_t j = rank[i];
    const uint2 cur = diag[j];
    const uint2 prev = j ? diag[j - 1] : make_uint2(0u, 0u);
    const uint32_t d = cur.x - prev.x;
    const uint32_t zz = (d << 1) ^ (uint32_t)((int32_t)d >> 31);
    c.v = ((unsigned long long)zz << 1) | (cur.y ^ prev.y);
    const uint32_t a = w.y <= 0xffu ? 1u : w.y <= 0xffffu ? 2u : 3u;
    const uint32_t b = c.v == 0 ? 0u : c.v < (1ull << 8) ? 1u : c.v < (1ull << 24) ? 2u : 3u;
    c.nibble = a | (b << 2);
    c.length_count = length_bytes(a);
    c.code_count = code_bytes(b);
    return c;
}

__global__ __launch_bounds__(kThreads) void pack_counts_kernel(const ArchiveRec *__restrict__ recs, uint64_t z,
                                                              const uint32_t *__restrict__ rank, const uint2 *__restrict__ diag,
                                                              uint32_t *__restrict__ counts) {
    const uint64_t stride = (uint64_t)gridDim.x * kThreads;
    for (uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x; i < z; i += stride) {
        const RecordCode c = record_code(recs, rank, diag, i);
        counts[i] = c.length_count + c.code_count;
    }
}

// the bytes of one record at data[at ..): its length, then its code (the counts are at most 4 and 5)
__device__ __forceinline__ void put_record(uint8_t *__restrict__ data, uint32_t at, const RecordCode &c) {
    for (uint32_t t = 0; t < c.length_count; ++t) data[at + t] = (uint8_t)(c.length >> (8 * t));
    at += c.length_count;
    for (uint32_t t = 0; t < c.code_count; ++t) data[at + t] = (uint8_t)(c.v >> (8 * t));
}

// One lane per pair of records: its control byte and the data bytes of both.
__global__ __launch_bounds__(kThreads) void pack_write_kernel(const ArchiveRec *__restrict__ recs, uint64_t z,
                                                             const uint32_t *__restrict__ rank, const uint2 *__restrict__ diag,
                                                             const uint32_t *__restrict__ offset, uint8_t *__restrict__ control,
                                                             uint8_t *__restrict__ data) {
    const uint64_t pairs = (z + 1) / 2, stride = (uint64_t)gridDim.x * kThreads;
    for (uint64_t j = (uint64_t)blockIdx.x * kThreads + threadIdx.x; j < pairs; j += stride) {
        const uint64_t i = 2 * j;
        const RecordCode lo = record_code(recs, rank, diag, i);
        uint32_t nibbles = lo.nibble;
        put_record(data, offset[i], lo);
        if (i + 1 < z) {
            const RecordCode hi = record_code(recs, rank, diag, i + 1);
            nibbles |= hi.nibble << 4;
            put_record(data, offset[i + 1], hi);
        }
        control[j] = (uint8_t)nibbles;
    }
}

// raw[index[i]] = the symbol of literal record i; *wide = 1 when one of them is not A, C, G or T (every writer stores
// the same value: no atomic)
__global__ __launch_bounds__(kThreads) void pack_literal_symbols_kernel(const ArchiveRec *__restrict__ recs, uint64_t z,
                                                                       const uint32_t *__restrict__ index, uint64_t n_literals,
                                                                       uint8_t *__restrict__ raw, uint32_t *__restrict__ wide) {
    const uint64_t stride = (uint64_t)gridDim.x * kThreads;
    for (uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x; i < z; i += stride) {
        const uint32_t meta = recs[i].meta;
        if ((meta & 3u) != kArchiveLiteral) continue;
        const uint32_t c = (meta >> 8) & 0xffu, at = index[i];
        if (at < n_literals) raw[at] = (uint8_t)c;
        if (base_code(c) > 3u) *wide = 1u;
    }
}

// One lane per output byte: four symbols of in[0 .. n) at 2 bits, the first in the low bits; anything but C, G, T is 0
__global__ __launch_bounds__(kThreads) void pack_quarter_kernel(const uint8_t *__restrict__ in, uint64_t n,
                                                               uint8_t *__restrict__ out) {
    const uint64_t bytes = (n + 3) / 4, stride = (uint64_t)gridDim.x * kThreads;
    for (uint64_t q = (uint64_t)blockIdx.x * kThreads + threadIdx.x; q < bytes; q += stride) {
        uint32_t v = 0;
#pragma unroll
        for (uint32_t t = 0; t < 4; ++t) {
            const uint64_t at = 4 * q + t;
            const uint32_t code = at < n ? base_code(in[at]) : 0u;
            v |= (code & 3u) << (2 * t);
        }
        out[q] = (uint8_t)v;
    }
}

// flags[p] = 1 for a 0x01 byte; *raw = 1 when a byte is none of A, C, G, T, 0x01
__global__ __launch_bounds__(kThreads) void pack_block_flags_kernel(const uint8_t *__restrict__ block, uint64_t B,
                                                                   uint32_t *__restrict__ flags, uint32_t *__restrict__ raw) {
    const uint64_t stride = (uint64_t)gridDim.x * kThreads;
    for (uint64_t p = (uint64_t)blockIdx.x * kThreads + threadIdx.x; p < B; p += stride) {
        const uint32_t c = block[p];
        flags[p] = c == 1u ? 1u : 0u;
        if (c != 1u && base_code(c) > 3u) *raw = 1u;
    }
}

// seps[index[p]] = p for every 0x01 byte (index: the exclusive scan of the flags)
__global__ __launch_bounds__(kThreads) void pack_separators_kernel(const uint8_t *__restrict__ block, uint64_t B,
                                                                  const uint32_t *__restrict__ index, uint32_t count,
                                                                  uint32_t *__restrict__ seps) {
    const uint64_t stride = (uint64_t)gridDim.x * kThreads;
    for (uint64_t p = (uint64_t)blockIdx.x * kThreads + threadIdx.x; p < B; p += stride)
        if (block[p] == 1u && index[p] < count) seps[index[p]] = (uint32_t)p;
}

// ---- unpack -------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t nibble_at(const uint8_t *__restrict__ control, uint64_t i) {
    return (control[i >> 1] >> (4 * (i & 1))) & 15u;
}
__device__ __forceinline__ void report(unsigned long long *err, unsigned long long index, uint32_t rule) {
    atomicMin(err, (index << 4) | rule);
}

// From the nibbles alone: counts[i] = the data bytes of record i, flags[i] = 1 for a copy.
__global__ __launch_bounds__(kThreads) void unpack_sizes_kernel(const uint8_t *__restrict__ control, uint64_t z,
                                                               uint32_t *__restrict__ counts, uint32_t *__restrict__ flags,
                                                               unsigned long long *__restrict__ err) {
    const uint64_t stride = (uint64_t)gridDim.x * kThreads;
    for (uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x; i < z; i += stride) {
        const uint32_t nib = nibble_at(control, i), a = nib & 3u, b = nib >> 2;
        if (a == 0 && b != 0) report(err, i, kPackLiteralNibble);
        if (i == z - 1 && (z & 1) && (control[i >> 1] >> 4) != 0) report(err, z, kPackSpareNibble);
        counts[i] = length_bytes(a) + code_bytes(b);
        flags[i] = a != 0 ? 1u : 0u;
    }
}

__device__ __forceinline__ unsigned long long bytes_at(const uint8_t *__restrict__ data, uint64_t size, uint64_t at,
                                                       uint32_t count) {  // count <= 5; a byte behind the section reads 0
    unsigned long long v = 0;
    for (uint32_t t = 0; t < count; ++t) {
        const uint64_t p = at + t;
        v |= (unsigned long long)(p < size ? data[p] : 0u) << (8 * t);
    }
    return v;
}

// lengths[i] = L; steps[rank[i]] = (e, s) of a copy
__global__ __launch_bounds__(kThreads) void unpack_read_kernel(const uint8_t *__restrict__ control, const uint8_t *__restrict__ data,
                                                              uint64_t data_bytes, const uint32_t *__restrict__ offset,
                                                              const uint32_t *__restrict__ rank, uint64_t z, uint64_t copies,
                                                              uint32_t *__restrict__ lengths, uint32_t *__restrict__ step_e,
                                                              uint32_t *__restrict__ step_s, unsigned long long *__restrict__ err) {
    const uint64_t stride = (uint64_t)gridDim.x * kThreads;
    for (uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x; i < z; i += stride) {
        const uint32_t nib = nibble_at(control, i), a = nib & 3u, b = nib >> 2;
        if (a == 0) {
            lengths[i] = 1u;
            continue;
        }
        const uint64_t at = offset[i];
        const uint32_t L = (uint32_t)bytes_at(data, data_bytes, at, length_bytes(a));
        const unsigned long long v = bytes_at(data, data_bytes, at + length_bytes(a), code_bytes(b));
        if (L == 0) report(err, i, kPackLength);
        if (v >> 33) report(err, i, kPackDiagonalCode);
        lengths[i] = L;
        const uint32_t zz = (uint32_t)(v >> 1), j = rank[i];
        if (j < copies) {
            step_e[j] = (zz >> 1) ^ (0u - (zz & 1u));
            step_s[j] = (uint32_t)(v & 1u);
        }
    }
}

struct UnpackArrays {
    const uint32_t *pos, *lengths, *rank;           // z each; pos: the exclusive sum of the lengths
    const uint32_t *step_e, *step_s, *sum_e, *sum_s;  // copies each; sum_*: the exclusive sums of step_*
};

__global__ __launch_bounds__(kThreads) void unpack_records_kernel(UnpackIn in, UnpackArrays u, uint64_t z, uint64_t copies,
                                                                 ArchiveRec *__restrict__ out, unsigned long long *__restrict__ err) {
    const uint64_t stride = (uint64_t)gridDim.x * kThreads;
    for (uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x; i < z; i += stride) {
        const uint32_t a = nibble_at(in.control, i) & 3u;
        const uint32_t p = u.pos[i], L = u.lengths[i], j = u.rank[i];
        uint32_t src = 0, meta = kArchiveLiteral;
        if (a == 0) {
            const uint64_t t = i - j;  // the literals among records [0, i)
            uint32_t c = 0;
            if (t >= in.n_literals) report(err, i, kPackLiteralCount);
            else if (in.literal_mode) c = code_base((in.literals[t >> 2] >> (2 * (t & 3))) & 3u);
            else c = in.literals[t];
            meta |= c << 8;
        } else if (j < copies) {
            const uint32_t g = u.sum_e[j] + u.step_e[j], r = (u.sum_s[j] + u.step_s[j]) & 1u;
            const uint32_t y = g + p;
            const uint32_t x = r ? 2u * in.B + 1u - y - L : y;
            if ((uint64_t)x + L > in.B) report(err, i, kPackSourceInBlock);
            src = r ? x + (L - 1u) : x;
            meta = r ? kArchiveRc : kArchiveForward;
        }
        // the first boundary behind p ends the target the record lies in (empty targets repeat a boundary)
        uint32_t lo = 0, hi = in.k + 1;  // bounds[0 .. lo) <= p
        while (lo < hi) {
            const uint32_t mid = lo + ((hi - lo) >> 1);
            if (in.bounds[mid] <= p) lo = mid + 1;
            else hi = mid;
        }
        if (lo > in.k || (uint64_t)p + L > in.bounds[lo]) report(err, i, kPackTargetBoundary);
        reinterpret_cast<uint4 *>(out)[i] = make_uint4(p, L, src, meta);
    }
}

// One lane per packed byte: four bases of the block
__global__ __launch_bounds__(kThreads) void unpack_quarter_kernel(const uint8_t *__restrict__ in, uint64_t n,
                                                                 uint8_t *__restrict__ out) {
    const uint64_t bytes = (n + 3) / 4, stride = (uint64_t)gridDim.x * kThreads;
    for (uint64_t q = (uint64_t)blockIdx.x * kThreads + threadIdx.x; q < bytes; q += stride) {
        const uint32_t v = in[q];
#pragma unroll
        for (uint32_t t = 0; t < 4; ++t)
            if (4 * q + t < n) out[4 * q + t] = (uint8_t)code_base((v >> (2 * t)) & 3u);
    }
}

__device__ __forceinline__ uint32_t word_at(const uint8_t *__restrict__ list, uint64_t t) {  // (any alignment)
    return (uint32_t)list[4 * t] | ((uint32_t)list[4 * t + 1] << 8) | ((uint32_t)list[4 * t + 2] << 16) |
           ((uint32_t)list[4 * t + 3] << 24);
}

// One lane per entry of the separator list: ascending, below B, then the 0x01 goes in (behind the bases: one stream)
__global__ __launch_bounds__(kThreads) void unpack_separators_kernel(const uint8_t *__restrict__ list, uint32_t count, uint64_t B,
                                                                    uint8_t *__restrict__ block, unsigned long long *__restrict__ err) {
    const uint64_t stride = (uint64_t)gridDim.x * kThreads;
    for (uint64_t t = (uint64_t)blockIdx.x * kThreads + threadIdx.x; t < count; t += stride) {
        const uint32_t p = word_at(list, t);
        if (p >= B || (t && word_at(list, t - 1) >= p)) report(err, t, kPackSeparatorList);
        else block[p] = 1u;
    }
}

unsigned long long read_word(Context &ctx, const unsigned long long *d_word) {
    uint32_t h[2];
    ctx.read_back(reinterpret_cast<const uint32_t *>(d_word), h, 2);
    return (unsigned long long)h[0] | ((unsigned long long)h[1] << 32);
}

}  // namespace

const char *packed_rule_text(uint32_t rule) {
    switch (rule) {
    case kPackSpareNibble: return "spare nibble (the unused high nibble of the last control byte of an odd z is 0)";
    case kPackLiteralNibble: return "literal nibble (a literal, a == 0, has b == 0)";
    case kPackLength: return "length (L >= 1)";
    case kPackDiagonalCode: return "diagonal code (v has 33 bits)";
    case kPackSourceInBlock:
        return "source inside the block (x + L must not exceed block_length, on either strand and after wrap-around)";
    case kPackTargetBoundary:
        return "target boundary (a record lies inside one target: it must not straddle the end of a target or lie behind "
               "the last one)";
    case kPackLiteralCount: return "literal count";
    case kPackDataSize: return "data size";
    case kPackSeparatorList: return "separator list (ascending positions below block_length)";
    default: return "unknown rule";
    }
}

PackPlan packed_plan(Context &ctx, const ArchiveRec *d_recs, size_t z, uint32_t B, size_t copies) {
    hipStream_t s = ctx.stream;
    PackPlan plan{};
    plan.rank = ctx.arena.alloc<uint32_t>(z);
    plan.diag = ctx.arena.alloc<uint2>(z);  // (a rank is below z whatever the handle counts: no read leaves the array)
    plan.offset = ctx.arena.alloc<uint32_t>(z);
    unsigned long long *d_sum = ctx.arena.alloc<unsigned long long>(1);
    uint32_t *d_copies = ctx.arena.alloc<uint32_t>(1);
    {
        ProfScope ps(ctx.profiler(), "rlz_packed_plan", s, 60.0 * (double)z);
        pack_copy_flags_kernel<<<record_grid(z), kThreads, 0, s>>>(d_recs, z, plan.rank);
        KERNEL_CHECK();
        scan_exclusive_add_u32(plan.rank, plan.rank, z, d_copies, ctx.arena, s);
        pack_diagonals_kernel<<<record_grid(z), kThreads, 0, s>>>(d_recs, z, B, plan.rank, copies, plan.diag);
        KERNEL_CHECK();
        pack_counts_kernel<<<record_grid(z), kThreads, 0, s>>>(d_recs, z, plan.rank, plan.diag, plan.offset);
        KERNEL_CHECK();
        sum_u32(ctx, plan.offset, z, d_sum);
        scan_exclusive_add_u32(plan.offset, plan.offset, z, nullptr, ctx.arena, s);
    }
    plan.data_bytes = read_word(ctx, d_sum);
    uint32_t found = 0;
    ctx.read_back(d_copies, &found, 1);
    if (found != copies) throw HipError("rlz archive: the resident records do not hold the literals the handle counts");
    return plan;
}

void packed_write(Context &ctx, const ArchiveRec *d_recs, size_t z, const PackPlan &plan, uint8_t *d_control, uint8_t *d_data) {
    ProfScope ps(ctx.profiler(), "rlz_packed_write", ctx.stream, 24.0 * (double)z + (double)plan.data_bytes);
    pack_write_kernel<<<record_grid((z + 1) / 2), kThreads, 0, ctx.stream>>>(d_recs, z, plan.rank, plan.diag, plan.offset,
                                                                             d_control, d_data);
    KERNEL_CHECK();
}

uint32_t packed_literals(Context &ctx, const ArchiveRec *d_recs, size_t z, size_t n_literals, uint8_t *d_raw, uint8_t *d_two) {
    if (n_literals == 0) return 1;
    hipStream_t s = ctx.stream;
    uint32_t *d_index = ctx.arena.alloc<uint32_t>(z);
    uint32_t *d_wide = ctx.arena.alloc<uint32_t>(1);
    const uint64_t found = archive_literal_index(ctx, d_recs, z, d_index);
    if (found != n_literals) throw HipError("rlz archive: the resident records do not hold the literals the handle counts");
    HIP_CHECK(hipMemsetAsync(d_wide, 0, sizeof(uint32_t), s));
    {
        ProfScope ps(ctx.profiler(), "rlz_packed_literals", s, 20.0 * (double)z + 1.25 * (double)n_literals);
        pack_literal_symbols_kernel<<<record_grid(z), kThreads, 0, s>>>(d_recs, z, d_index, n_literals, d_raw, d_wide);
        KERNEL_CHECK();
        pack_quarter_kernel<<<record_grid(packed_quarter(n_literals)), kThreads, 0, s>>>(d_raw, n_literals, d_two);
        KERNEL_CHECK();
    }
    uint32_t wide = 0;
    ctx.read_back(d_wide, &wide, 1);
    return wide ? 0u : 1u;
}

uint32_t packed_block(Context &ctx, const uint8_t *d_block, size_t B, uint8_t *d_two, uint32_t **d_seps, uint32_t *num_seps) {
    *d_seps = nullptr;
    *num_seps = 0;
    if (B == 0) return 1;
    hipStream_t s = ctx.stream;
    uint32_t *d_index = ctx.arena.alloc<uint32_t>(B);
    uint32_t *d_ctl = ctx.arena.alloc<uint32_t>(2);  // raw flag, separators
    HIP_CHECK(hipMemsetAsync(d_ctl, 0, 2 * sizeof(uint32_t), s));
    {
        ProfScope ps(ctx.profiler(), "rlz_packed_block", s, 10.25 * (double)B);
        pack_block_flags_kernel<<<record_grid(B), kThreads, 0, s>>>(d_block, B, d_index, d_ctl);
        KERNEL_CHECK();
        scan_exclusive_add_u32(d_index, d_index, B, d_ctl + 1, ctx.arena, s);
        pack_quarter_kernel<<<record_grid(packed_quarter(B)), kThreads, 0, s>>>(d_block, B, d_two);
        KERNEL_CHECK();
    }
    uint32_t h[2];
    ctx.read_back(d_ctl, h, 2);
    if (h[0]) return 0;
    if (h[1]) {
        *d_seps = ctx.arena.alloc<uint32_t>(h[1]);
        *num_seps = h[1];
        ProfScope ps(ctx.profiler(), "rlz_packed_block", s, 5.0 * (double)B);
        pack_separators_kernel<<<record_grid(B), kThreads, 0, s>>>(d_block, B, d_index, h[1], *d_seps);
        KERNEL_CHECK();
    }
    return 1;
}

uint64_t unpack_block(Context &ctx, const uint8_t *d_section, size_t B, uint32_t num_seps, uint8_t *d_block) {
    if (B == 0) return ~0ull;
    hipStream_t s = ctx.stream;
    unsigned long long *d_err = ctx.arena.alloc<unsigned long long>(1);
    HIP_CHECK(hipMemsetAsync(d_err, 0xff, sizeof(unsigned long long), s));
    {
        ProfScope ps(ctx.profiler(), "rlz_unpack_block", s, 1.25 * (double)B + 5.0 * (double)num_seps);
        unpack_quarter_kernel<<<record_grid(packed_quarter(B)), kThreads, 0, s>>>(d_section, B, d_block);
        KERNEL_CHECK();
        if (num_seps) {
            unpack_separators_kernel<<<record_grid(num_seps), kThreads, 0, s>>>(d_section + packed_quarter(B), num_seps, B, d_block,
                                                                                 d_err);
            KERNEL_CHECK();
        }
    }
    return read_word(ctx, d_err);
}

UnpackOut unpack_records(Context &ctx, const UnpackIn &in, size_t z, ArchiveRec *d_recs) {
    hipStream_t s = ctx.stream;
    Arena &arena = ctx.arena;
    UnpackOut res;
    uint32_t *offset = arena.alloc<uint32_t>(z);
    uint32_t *rank = arena.alloc<uint32_t>(z);
    unsigned long long *ctl = arena.alloc<unsigned long long>(2);  // the error word, the byte total
    uint32_t *d_copies = arena.alloc<uint32_t>(1);
    HIP_CHECK(hipMemsetAsync(ctl, 0xff, sizeof(unsigned long long), s));
    {
        ProfScope ps(ctx.profiler(), "rlz_unpack_sizes", s, 32.5 * (double)z);
        unpack_sizes_kernel<<<record_grid(z), kThreads, 0, s>>>(in.control, z, offset, rank, ctl);
        KERNEL_CHECK();
        sum_u32(ctx, offset, z, ctl + 1);
        scan_exclusive_add_u32(offset, offset, z, nullptr, arena, s);
        scan_exclusive_add_u32(rank, rank, z, d_copies, arena, s);
    }
    // the sizes are settled before a data byte is read
    uint32_t h[5];
    ctx.read_back(reinterpret_cast<const uint32_t *>(ctl), h, 4);
    ctx.read_back(d_copies, h + 4, 1);
    res.bad = (uint64_t)h[0] | ((uint64_t)h[1] << 32);
    res.copies = h[4];
    if (res.bad != ~0ull) return res;
    const uint64_t need = (uint64_t)h[2] | ((uint64_t)h[3] << 32);
    if (need != in.data_bytes) {
        res.bad = ((uint64_t)z << 4) | kPackDataSize;
        return res;
    }
    const size_t copies = (size_t)res.copies;
    uint32_t *lengths = arena.alloc<uint32_t>(z);
    uint32_t *pos = arena.alloc<uint32_t>(z);
    uint32_t *step_e = arena.alloc<uint32_t>(copies ? copies : 1);
    uint32_t *step_s = arena.alloc<uint32_t>(copies ? copies : 1);
    uint32_t *sum_e = arena.alloc<uint32_t>(copies ? copies : 1);
    uint32_t *sum_s = arena.alloc<uint32_t>(copies ? copies : 1);
    uint32_t *d_last = arena.alloc<uint32_t>(1);
    {
        ProfScope ps(ctx.profiler(), "rlz_unpack_records", s, 60.0 * (double)z + (double)in.data_bytes);
        unpack_read_kernel<<<record_grid(z), kThreads, 0, s>>>(in.control, in.data, in.data_bytes, offset, rank, z, copies, lengths,
                                                               step_e, step_s, ctl);
        KERNEL_CHECK();
        scan_exclusive_add_u32(lengths, pos, z, d_last, arena, s);
        scan_exclusive_add_u32(step_e, sum_e, copies, nullptr, arena, s);
        scan_exclusive_add_u32(step_s, sum_s, copies, nullptr, arena, s);
        const UnpackArrays u{pos, lengths, rank, step_e, step_s, sum_e, sum_s};
        unpack_records_kernel<<<record_grid(z), kThreads, 0, s>>>(in, u, z, copies, d_recs, ctl);
        KERNEL_CHECK();
    }
    ctx.read_back(reinterpret_cast<const uint32_t *>(ctl), h, 2);
    ctx.read_back(d_last, h + 2, 1);
    res.bad = (uint64_t)h[0] | ((uint64_t)h[1] << 32);
    res.covered = h[2];
    return res;
}

// What the container of the factor records of the other modes shares with this one (factor_pack.hip)
void packed_sum_u32(Context &ctx, const uint32_t *d_in, size_t n, unsigned long long *d_out) { sum_u32(ctx, d_in, n, d_out); }

void packed_quarter_pack(Context &ctx, const uint8_t *d_in, size_t n, uint8_t *d_out) {
    if (n == 0) return;
    pack_quarter_kernel<<<record_grid(packed_quarter(n)), kThreads, 0, ctx.stream>>>(d_in, n, d_out);
    KERNEL_CHECK();
}

void packed_quarter_unpack(Context &ctx, const uint8_t *d_in, size_t n, uint8_t *d_out) {
    if (n == 0) return;
    unpack_quarter_kernel<<<record_grid(packed_quarter(n)), kThreads, 0, ctx.stream>>>(d_in, n, d_out);
    KERNEL_CHECK();
}

}  // namespace nolzss
