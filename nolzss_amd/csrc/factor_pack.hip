// factor_pack.hip -- the compact container of the factor records of every mode but relative LZ: the 24-byte (start,
// length, ref) records packed into control nibbles and data bytes, and expanded again with every rule of the format
// checked ("Factor records: the compact container"; the format: include/nolzss_hip.h, nolzss_factors_pack).
//
// The shape is that of rlz_archive_pack.hip over another record and another mirror.  A copy is coded by its length and
// by the step of its diagonal g = y - p from the copy before it, y = x on the forward strand and -(x + L) mod 2^32 on
// the reverse-complement one: the coordinate in which a reverse-complement match reads forward, so that a copy that
// goes on colinearly on either strand steps by 0.  Which copy comes before it is a rank (an exclusive scan of the copy
// flags), where a record's bytes go is an offset (an exclusive scan of the byte counts), and the way back turns lengths
// into positions, steps into diagonals and strand toggles into strands with three more scans: everything is
// scan_exclusive_add_u32 and kernels of one lane per record or per pair of records.
// Every loop is bounded by the format and not by the data: at most 4 length bytes and 5 code bytes per record.  No
// spinning, no communication between workgroups; the only atomic is the atomicMin on the error word.  Every read of an
// uploaded section is bounded by the section's size, which the host has checked, and never by what the section says.
#include "factor_pack.hpp"
#include "rlz_archive_pack.hpp"

namespace nolzss {
namespace {

constexpr int kThreads = 256;

__device__ __forceinline__ uint32_t length_bytes(uint32_t a) { return a == 3 ? 4u : a; }              // 0, 1, 2, 4
__device__ __forceinline__ uint32_t code_bytes(uint32_t b) { return b == 3 ? 5u : 2u * b; }            // 0, 2, 4, 5
__device__ __forceinline__ bool is_literal(const Rec &f) { return f.ref == f.start; }
__device__ __forceinline__ void report(unsigned long long *err, unsigned long long index, uint32_t rule) {
    atomicMin(err, (index << 4) | rule);
}

// ---- pack ---------------------------------------------------------------------------------------------------------
// The rules over host-made records, each judged against the record before it alone.
__global__ __launch_bounds__(kThreads) void factor_check_kernel(const Rec *__restrict__ recs, uint64_t z, uint64_t limit,
                                                                unsigned long long *__restrict__ err) {
    unsigned long long bad = ~0ull;
    const uint64_t stride = (uint64_t)gridDim.x * kThreads;
    for (uint64_t k = (uint64_t)blockIdx.x * kThreads + threadIdx.x; k < z; k += stride) {
        const Rec f = recs[k];
        uint64_t expect = f.start;  // (the first record sets first_start)
        if (k) {
            const Rec p = recs[k - 1];
            expect = p.start + p.length;
        }
        const bool lit = is_literal(f);
        const uint64_t r = f.ref & ~kRcMask;
        uint32_t rule = kFacOk;
        if (f.start != expect || f.length == 0 || f.start > limit || f.length > limit - f.start) rule = kFacTiling;
        else if (lit && f.length != 1) rule = kFacLiteralLength;
        else if (!lit && (r > f.start || f.length > f.start - r)) rule = kFacSourceRange;
        if (rule != kFacOk) {
            const unsigned long long key = (k << 4) | rule;
            bad = key < bad ? key : bad;
        }
    }
    if (bad != ~0ull) atomicMin(err, bad);
}

__global__ __launch_bounds__(kThreads) void factor_copy_flags_kernel(const Rec *__restrict__ recs, uint64_t z,
                                                                     uint32_t *__restrict__ flags) {
    const uint64_t stride = (uint64_t)gridDim.x * kThreads;
    for (uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x; i < z; i += stride)
        flags[i] = is_literal(recs[i]) ? 0u : 1u;
}

// diag[rank[i]] = (g, r) of copy i: r the strand, g = y - p with y = x (forward) or -(x + L) (reverse complement)
__global__ __launch_bounds__(kThreads) void factor_diagonals_kernel(const Rec *__restrict__ recs, uint64_t z,
                                                                    const uint32_t *__restrict__ rank,
                                                                    uint2 *__restrict__ diag) {
    const uint64_t stride = (uint64_t)gridDim.x * kThreads;
    for (uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x; i < z; i += stride) {
        const Rec f = recs[i];
        if (is_literal(f)) continue;
        const uint32_t r = (uint32_t)(f.ref >> 63), x = (uint32_t)f.ref, L = (uint32_t)f.length, p = (uint32_t)f.start;
        const uint32_t y = r ? 0u - (x + L) : x;
        const uint32_t j = rank[i];
        if (j < z) diag[j] = make_uint2(y - p, r);  // (a rank is below z: diag has room for z)
    }
}

struct RecordCode {
    uint32_t nibble, length, length_count, code_count;
    unsigned long long v;
};
__device__ __forceinline__ RecordCode record_code(const Rec *__restrict__ recs, const uint32_t *__restrict__ rank,
                                                  const uint2 *__restrict__ diag, uint64_t i) {
    const Rec f = recs[i];
    RecordCode c{0u, (uint32_t)f.length, 0u, 0u, 0ull};
    if (is_literal(f)) return c;
    const uint32_t j = rank[i];
    const uint2 cur = diag[j];
    const uint2 prev = j ? diag[j - 1] : make_uint2(0u, 0u);
    const uint32_t e = cur.x - prev.x;
    const uint32_t zz = (e << 1) ^ (uint32_t)((int32_t)e >> 31);
    c.v = ((unsigned long long)zz << 1) | (cur.y ^ prev.y);
    const uint32_t a = c.length <= 0xffu ? 1u : c.length <= 0xffffu ? 2u : 3u;
    const uint32_t b = c.v == 0 ? 0u : c.v < (1ull << 16) ? 1u : c.v < (1ull << 32) ? 2u : 3u;
    c.nibble = a | (b << 2);
    c.length_count = length_bytes(a);
    c.code_count = code_bytes(b);
    return c;
}

__global__ __launch_bounds__(kThreads) void factor_counts_kernel(const Rec *__restrict__ recs, uint64_t z,
                                                                 const uint32_t *__restrict__ rank, const uint2 *__restrict__ diag,
                                                                 uint32_t *__restrict__ counts) {
    const uint64_t stride = (uint64_t)gridDim.x * kThreads;
    for (uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x; i < z; i += stride) {
        const RecordCode c = record_code(recs, rank, diag, i);
        counts[i] = c.length_count + c.code_count;
    }
}

// the bytes of one record at data[at ..): its length, then its code (the counts are at most 4 and 5; the caller has
// refused a section of 2^32 bytes or more, so at + 9 does not wrap)
__device__ __forceinline__ void put_record(uint8_t *__restrict__ data, uint64_t size, uint64_t at, const RecordCode &c) {
    for (uint32_t t = 0; t < c.length_count; ++t)
        if (at + t < size) data[at + t] = (uint8_t)(c.length >> (8 * t));
    at += c.length_count;
    for (uint32_t t = 0; t < c.code_count; ++t)
        if (at + t < size) data[at + t] = (uint8_t)(c.v >> (8 * t));
}

// One lane per pair of records: its control byte and the data bytes of both.
__global__ __launch_bounds__(kThreads) void factor_write_kernel(const Rec *__restrict__ recs, uint64_t z,
                                                                const uint32_t *__restrict__ rank, const uint2 *__restrict__ diag,
                                                                const uint32_t *__restrict__ offset, uint64_t data_bytes,
                                                                uint8_t *__restrict__ control, uint8_t *__restrict__ data) {
    const uint64_t pairs = (z + 1) / 2, stride = (uint64_t)gridDim.x * kThreads;
    for (uint64_t j = (uint64_t)blockIdx.x * kThreads + threadIdx.x; j < pairs; j += stride) {
        const uint64_t i = 2 * j;
        const RecordCode lo = record_code(recs, rank, diag, i);
        uint32_t nibbles = lo.nibble;
        put_record(data, data_bytes, offset[i], lo);
        if (i + 1 < z) {
            const RecordCode hi = record_code(recs, rank, diag, i + 1);
            nibbles |= hi.nibble << 4;
            put_record(data, data_bytes, offset[i + 1], hi);
        }
        control[j] = (uint8_t)nibbles;
    }
}

// *wide = 1 when a symbol is none of A, C, G, T (every writer stores the same value: no atomic)
__global__ __launch_bounds__(kThreads) void factor_literals_wide_kernel(const uint8_t *__restrict__ raw, uint64_t n,
                                                                        uint32_t *__restrict__ wide) {
    const uint64_t stride = (uint64_t)gridDim.x * kThreads;
    for (uint64_t t = (uint64_t)blockIdx.x * kThreads + threadIdx.x; t < n; t += stride) {
        const uint32_t c = raw[t];
        if (c != 'A' && c != 'C' && c != 'G' && c != 'T') *wide = 1u;
    }
}

// ---- unpack -------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t nibble_at(const uint8_t *__restrict__ control, uint64_t i) {
    return (control[i >> 1] >> (4 * (i & 1))) & 15u;
}

// From the nibbles alone: counts[i] = the data bytes of record i, flags[i] = 1 for a copy.
__global__ __launch_bounds__(kThreads) void factor_unpack_sizes_kernel(const uint8_t *__restrict__ control, uint64_t z,
                                                                       uint32_t *__restrict__ counts, uint32_t *__restrict__ flags,
                                                                       unsigned long long *__restrict__ err) {
    const uint64_t stride = (uint64_t)gridDim.x * kThreads;
    for (uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x; i < z; i += stride) {
        const uint32_t nib = nibble_at(control, i), a = nib & 3u, b = nib >> 2;
        if (a == 0 && b != 0) report(err, i, kFacLiteralNibble);
        if (i == z - 1 && (z & 1) && (control[i >> 1] >> 4) != 0) report(err, z, kFacSpareNibble);
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

// lengths[i] = L; (step_e, step_s)[rank[i]] = (e, s) of a copy
__global__ __launch_bounds__(kThreads) void factor_unpack_read_kernel(const uint8_t *__restrict__ control,
                                                                      const uint8_t *__restrict__ data, uint64_t data_bytes,
                                                                      const uint32_t *__restrict__ offset,
                                                                      const uint32_t *__restrict__ rank, uint64_t z, uint64_t copies,
                                                                      uint32_t *__restrict__ lengths, uint32_t *__restrict__ step_e,
                                                                      uint32_t *__restrict__ step_s,
                                                                      unsigned long long *__restrict__ err) {
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
        if (L == 0) report(err, i, kFacLength);
        if (v >> 33) report(err, i, kFacDiagonalCode);
        lengths[i] = L;
        const uint32_t zz = (uint32_t)(v >> 1), j = rank[i];
        if (j < copies) {
            step_e[j] = (zz >> 1) ^ (0u - (zz & 1u));
            step_s[j] = (uint32_t)(v & 1u);
        }
    }
}

struct UnpackArrays {
    const uint32_t *pos, *lengths, *rank;             // z each; pos: the exclusive sum of the lengths
    const uint32_t *step_e, *step_s, *sum_e, *sum_s;  // copies each; sum_*: the exclusive sums of step_*
};

// (the lengths sum to `decoded` and first_start + decoded stays inside the pipeline: no position wraps)
__global__ __launch_bounds__(kThreads) void factor_unpack_records_kernel(const uint8_t *__restrict__ control, UnpackArrays u,
                                                                         uint64_t z, uint64_t copies, uint32_t first_start,
                                                                         uint64_t n_literals, Rec *__restrict__ out,
                                                                         unsigned long long *__restrict__ err) {
    const uint64_t stride = (uint64_t)gridDim.x * kThreads;
    for (uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x; i < z; i += stride) {
        const uint32_t a = nibble_at(control, i) & 3u;
        const uint32_t p = first_start + u.pos[i], L = u.lengths[i], j = u.rank[i];
        uint64_t ref = p;
        if (a == 0) {
            if (i - j >= n_literals) report(err, i, kFacLiteralCount);  // i - j: the literals among records [0, i)
        } else if (j < copies) {
            const uint32_t g = u.sum_e[j] + u.step_e[j], r = (u.sum_s[j] + u.step_s[j]) & 1u;
            const uint32_t y = g + p;
            const uint32_t x = r ? 0u - y - L : y;
            if ((uint64_t)x + L > p) report(err, i, kFacSourceRange);
            ref = (uint64_t)x | (r ? kRcMask : 0ull);
        }
        out[i] = Rec{p, L, ref};
    }
}

unsigned long long read_word(Context &ctx, const unsigned long long *d_word) {
    uint32_t h[2];
    ctx.read_back(reinterpret_cast<const uint32_t *>(d_word), h, 2);
    return (unsigned long long)h[0] | ((unsigned long long)h[1] << 32);
}

}  // namespace

const char *factor_pack_rule_text(uint32_t rule) {
    switch (rule) {
    case kFacTiling: return "tiling (start[k + 1] = start[k] + length[k], length >= 1, the end inside the 32-bit pipeline)";
    case kFacLiteralLength: return "literal length (a literal, ref == start, has length 1)";
    case kFacSourceRange: return "source range (ref + length must not exceed start)";
    case kFacSpareNibble: return "spare nibble (the unused high nibble of the last control byte of an odd z is 0)";
    case kFacLiteralNibble: return "literal nibble (a literal, a == 0, has b == 0)";
    case kFacLength: return "length (L >= 1)";
    case kFacDiagonalCode: return "diagonal code (v has 33 bits)";
    case kFacLiteralCount: return "literal count";
    case kFacDataSize: return "data size";
    case kFacDecoded: return "decoded length (the lengths sum to decoded)";
    default: return "unknown rule";
    }
}

uint64_t factor_check_records(Context &ctx, const Rec *d_recs, size_t z, uint64_t limit) {
    if (z == 0) return ~0ull;
    hipStream_t s = ctx.stream;
    unsigned long long *d_err = ctx.arena.alloc<unsigned long long>(1);
    HIP_CHECK(hipMemsetAsync(d_err, 0xff, sizeof(unsigned long long), s));
    {
        ProfScope ps(ctx.profiler(), "factors_pack_check", s, 24.0 * (double)z);
        factor_check_kernel<<<record_grid(z), kThreads, 0, s>>>(d_recs, z, limit, d_err);
        KERNEL_CHECK();
    }
    return read_word(ctx, d_err);
}

FactorPackPlan factor_pack_plan(Context &ctx, const Rec *d_recs, size_t z) {
    hipStream_t s = ctx.stream;
    FactorPackPlan plan{};
    plan.rank = ctx.arena.alloc<uint32_t>(z);
    plan.diag = ctx.arena.alloc<uint2>(z);
    plan.offset = ctx.arena.alloc<uint32_t>(z);
    unsigned long long *d_sum = ctx.arena.alloc<unsigned long long>(1);
    uint32_t *d_copies = ctx.arena.alloc<uint32_t>(1);
    {
        ProfScope ps(ctx.profiler(), "factors_pack_plan", s, 100.0 * (double)z);
        factor_copy_flags_kernel<<<record_grid(z), kThreads, 0, s>>>(d_recs, z, plan.rank);
        KERNEL_CHECK();
        scan_exclusive_add_u32(plan.rank, plan.rank, z, d_copies, ctx.arena, s);
        factor_diagonals_kernel<<<record_grid(z), kThreads, 0, s>>>(d_recs, z, plan.rank, plan.diag);
        KERNEL_CHECK();
        factor_counts_kernel<<<record_grid(z), kThreads, 0, s>>>(d_recs, z, plan.rank, plan.diag, plan.offset);
        KERNEL_CHECK();
        packed_sum_u32(ctx, plan.offset, z, d_sum);
        scan_exclusive_add_u32(plan.offset, plan.offset, z, nullptr, ctx.arena, s);
    }
    plan.data_bytes = read_word(ctx, d_sum);
    uint32_t found = 0;
    ctx.read_back(d_copies, &found, 1);
    plan.copies = found;
    return plan;
}

void factor_pack_write(Context &ctx, const Rec *d_recs, size_t z, const FactorPackPlan &plan, uint8_t *d_control, uint8_t *d_data) {
    ProfScope ps(ctx.profiler(), "factors_pack_write", ctx.stream, 32.0 * (double)z + (double)plan.data_bytes);
    factor_write_kernel<<<record_grid((z + 1) / 2), kThreads, 0, ctx.stream>>>(d_recs, z, plan.rank, plan.diag, plan.offset,
                                                                               plan.data_bytes, d_control, d_data);
    KERNEL_CHECK();
}

uint32_t factor_pack_literals(Context &ctx, const uint8_t *d_raw, size_t n_literals, uint8_t *d_two) {
    if (n_literals == 0) return 1;
    hipStream_t s = ctx.stream;
    uint32_t *d_wide = ctx.arena.alloc<uint32_t>(1);
    HIP_CHECK(hipMemsetAsync(d_wide, 0, sizeof(uint32_t), s));
    {
        ProfScope ps(ctx.profiler(), "factors_pack_literals", s, 2.25 * (double)n_literals);
        factor_literals_wide_kernel<<<record_grid(n_literals), kThreads, 0, s>>>(d_raw, n_literals, d_wide);
        KERNEL_CHECK();
        packed_quarter_pack(ctx, d_raw, n_literals, d_two);
    }
    uint32_t wide = 0;
    ctx.read_back(d_wide, &wide, 1);
    return wide ? 0u : 1u;
}

FactorUnpackOut factor_unpack_records(Context &ctx, const FactorUnpackIn &in, size_t z, Rec *d_recs) {
    hipStream_t s = ctx.stream;
    Arena &arena = ctx.arena;
    FactorUnpackOut res;
    uint32_t *offset = arena.alloc<uint32_t>(z);
    uint32_t *rank = arena.alloc<uint32_t>(z);
    unsigned long long *ctl = arena.alloc<unsigned long long>(2);  // the error word, a total
    uint32_t *d_copies = arena.alloc<uint32_t>(1);
    HIP_CHECK(hipMemsetAsync(ctl, 0xff, sizeof(unsigned long long), s));
    {
        ProfScope ps(ctx.profiler(), "factors_unpack_sizes", s, 32.5 * (double)z);
        factor_unpack_sizes_kernel<<<record_grid(z), kThreads, 0, s>>>(in.control, z, offset, rank, ctl);
        KERNEL_CHECK();
        packed_sum_u32(ctx, offset, z, ctl + 1);
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
        res.bad = ((uint64_t)z << 4) | kFacDataSize;
        return res;
    }
    const size_t copies = (size_t)res.copies;
    uint32_t *lengths = arena.alloc<uint32_t>(z);
    uint32_t *pos = arena.alloc<uint32_t>(z);
    uint32_t *step_e = arena.alloc<uint32_t>(copies ? copies : 1);
    uint32_t *step_s = arena.alloc<uint32_t>(copies ? copies : 1);
    uint32_t *sum_e = arena.alloc<uint32_t>(copies ? copies : 1);
    uint32_t *sum_s = arena.alloc<uint32_t>(copies ? copies : 1);
    {
        ProfScope ps(ctx.profiler(), "factors_unpack_read", s, 20.0 * (double)z + (double)in.data_bytes);
        factor_unpack_read_kernel<<<record_grid(z), kThreads, 0, s>>>(in.control, in.data, in.data_bytes, offset, rank, z, copies,
                                                                      lengths, step_e, step_s, ctl);
        KERNEL_CHECK();
        packed_sum_u32(ctx, lengths, z, ctl + 1);
    }
    // every length is at least 1 and they sum to `decoded` before a position is formed
    ctx.read_back(reinterpret_cast<const uint32_t *>(ctl), h, 4);
    res.bad = (uint64_t)h[0] | ((uint64_t)h[1] << 32);
    res.covered = (uint64_t)h[2] | ((uint64_t)h[3] << 32);
    if (res.bad != ~0ull) return res;
    if (res.covered != in.decoded) {
        res.bad = ((uint64_t)z << 4) | kFacDecoded;
        return res;
    }
    {
        ProfScope ps(ctx.profiler(), "factors_unpack_records", s, 64.0 * (double)z);
        scan_exclusive_add_u32(lengths, pos, z, nullptr, arena, s);
        if (copies) {
            scan_exclusive_add_u32(step_e, sum_e, copies, nullptr, arena, s);
            scan_exclusive_add_u32(step_s, sum_s, copies, nullptr, arena, s);
        }
        const UnpackArrays u{pos, lengths, rank, step_e, step_s, sum_e, sum_s};
        factor_unpack_records_kernel<<<record_grid(z), kThreads, 0, s>>>(in.control, u, z, copies, in.first_start, in.n_literals,
                                                                         d_recs, ctl);
        KERNEL_CHECK();
    }
    res.bad = read_word(ctx, ctl);
    return res;
}

}  // namespace nolzss
