// decode.hip -- factors and literals back to text: the record check, the per-position state words, the pointer-jumping
// rounds over them and the byte output; the literal gather and the byte comparison of the device-resident round trip
// ("Decoding: factors and literals back to text"; semantics: include/nolzss_hip.h, nolzss_decode).
//
// State word of a decoded position x (one u64, index x - prefix_len):
//     bits 63..32  source: an earlier decoded position y, prefix_len <= y < x   (0 once resolved)
//     bit  9       strand: text[x] = comp(text[y]) if set, text[y] otherwise    (0 once resolved)
//     bit  8       resolved: bits 7..0 hold text[x]
// Every word ever stored for x is a true statement about text[x], and the words of one position only ever move
// towards "resolved" along x's chain.  A round may therefore read the word of y in any state, old or new: each word
// is read and written as ONE 64-bit relaxed agent-scope atomic, so a reader sees a whole older or a whole newer
// statement, never a mixture.  Between two launches everything is visible, so a round makes at least the progress of
// synchronous pointer doubling: a chain of d copy hops is resolved after floor(log2 d) + 1 rounds.
#include "decode.hpp"

namespace nolzss {
namespace {

constexpr int kThreads = 256;
constexpr int kTile = 4096;
constexpr int kPerThread = kTile / kThreads;  // 16
constexpr int kMaxRounds = 34;
constexpr int kJumpBatch = 4;

constexpr uint64_t kResolved = 1ull << 8;
constexpr uint64_t kStrand = 1ull << 9;
constexpr uint32_t kNoPosition = 0xffffffffu;

// control words of one decode (u32 indices into one block that is zeroed / preset per call)
enum : int {
    kCtlBadLo = 0,     // u64 at words 0..1: (record index << 3 | rule) of the first bad record, atomicMin
    kCtlLiterals = 2,  // u64 at words 2..3: literal records
    kCtlComplement = 4,  // smallest position whose chain complements a non-nucleotide
    kCtlActive = 5,      // unresolved positions behind expand
    kCtlRound = 8,       // + r: unresolved positions behind jump round r
    kCtlWords = kCtlRound + kMaxRounds + 2,
};

__device__ __forceinline__ uint32_t complement(uint32_t c) {  // 0: not a nucleotide
    return c == 'A' ? 'T' : c == 'T' ? 'A' : c == 'C' ? 'G' : c == 'G' ? 'C' : 0u;
}

__device__ __forceinline__ uint64_t load_word(const uint64_t *p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void store_word(uint64_t *p, uint64_t v) {
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ bool is_literal(const Rec &f) { return f.ref == f.start; }

// The structural rules over the z records: tiling (start[0] = prefix_len, start[k + 1] = start[k] + length[k],
// length >= 1, the last record ends at n), literal length, source range.  flags[k] = 1 for a literal record.
__global__ __launch_bounds__(kThreads) void decode_check_kernel(const Rec *__restrict__ recs, uint64_t z, uint64_t prefix_len,
                                                                uint64_t n, uint32_t *__restrict__ flags,
                                                                unsigned long long *__restrict__ ctl) {
    unsigned long long bad = ~0ull, literals = 0;
    const uint64_t stride = (uint64_t)gridDim.x * kThreads;
    for (uint64_t k = (uint64_t)blockIdx.x * kThreads + threadIdx.x; k < z; k += stride) {
        const Rec f = recs[k];
        uint64_t expect = prefix_len;
        if (k) {
            const Rec p = recs[k - 1];
            expect = p.start + p.length;
        }
        uint32_t rule = kDecodeOk;
        const bool lit = is_literal(f);
        const uint64_t r = f.ref & ~kRcMask;
        if (f.start != expect || f.length == 0 || f.start > n || f.length > n - f.start ||
            (k == z - 1 && f.length != n - f.start))
            rule = kDecodeTiling;
        else if (lit && f.length != 1) rule = kDecodeLiteralLength;
        else if (!lit && (r > f.start || f.length > f.start - r)) rule = kDecodeSourceRange;
        if (rule != kDecodeOk) {
            const unsigned long long key = (k << 3) | rule;
            bad = key < bad ? key : bad;
        }
        flags[k] = lit ? 1u : 0u;
        literals += lit ? 1u : 0u;
    }
    if (bad != ~0ull) atomicMin(&ctl[kCtlBadLo / 2], bad);
    if (literals) atomicAdd(&ctl[kCtlLiterals / 2], literals);
}

// flags only (the records of a pipeline run need no check)
__global__ __launch_bounds__(kThreads) void literal_flag_kernel(const Rec *__restrict__ recs, uint64_t z,
                                                                uint32_t *__restrict__ flags) {
    const uint64_t stride = (uint64_t)gridDim.x * kThreads;
    for (uint64_t k = (uint64_t)blockIdx.x * kThreads + threadIdx.x; k < z; k += stride) flags[k] = is_literal(recs[k]) ? 1u : 0u;
}

// lit_index: the exclusive add-scan of the literal flags
__global__ __launch_bounds__(kThreads) void literal_gather_kernel(const Rec *__restrict__ recs, uint64_t z,
                                                                  const uint32_t *__restrict__ lit_index,
                                                                  const uint8_t *__restrict__ text,
                                                                  uint8_t *__restrict__ literals) {
    const uint64_t stride = (uint64_t)gridDim.x * kThreads;
    for (uint64_t k = (uint64_t)blockIdx.x * kThreads + threadIdx.x; k < z; k += stride) {
        const Rec f = recs[k];
        if (is_literal(f)) literals[lit_index[k]] = text[f.start];
    }
}

__device__ __forceinline__ int padded(int i) { return i + (i >> 4); }  // 16 consecutive items per lane, no bank conflict

// One workgroup per tile of kTile decoded positions: the record of every position, then its state word.
// The record that covers the tile's first position is found by binary search over the ascending starts; the heads of
// the records that start inside the tile are flagged in LDS with their index and a max-scan carries the index over
// the positions each record covers (a record may span many tiles: then the tile has no head but its first).
__global__ __launch_bounds__(kThreads) void decode_expand_kernel(const Rec *__restrict__ recs, uint32_t z,
                                                                 const uint32_t *__restrict__ lit_index,
                                                                 const uint8_t *__restrict__ literals,
                                                                 const uint8_t *__restrict__ prefix, uint32_t prefix_len,
                                                                 uint32_t n, uint64_t *__restrict__ state,
                                                                 uint32_t *__restrict__ tile_active,
                                                                 uint32_t *__restrict__ ctl) {
    __shared__ uint32_t head[kTile + kTile / 16];
    __shared__ uint32_t scan_lds[kThreads / 64];
    __shared__ uint32_t first_rec, active;
    const uint32_t tile_base = prefix_len + blockIdx.x * (uint32_t)kTile;  // (< n <= kMaxText: no wrap)
    const uint32_t tile_len = n - tile_base < (uint32_t)kTile ? n - tile_base : (uint32_t)kTile;
    const uint64_t tile_end = (uint64_t)tile_base + tile_len;
    for (int i = threadIdx.x; i < kTile + kTile / 16; i += kThreads) head[i] = 0;
    if (threadIdx.x == 0) {
        uint32_t lo = 0, hi = z;  // the last record with start <= tile_base (record 0 starts at prefix_len)
        while (hi - lo > 1) {
            const uint32_t mid = lo + ((hi - lo) >> 1);
            if (recs[mid].start <= tile_base) lo = mid;
            else hi = mid;
        }
        first_rec = lo;
        active = 0;
    }
    __syncthreads();
    const uint32_t lo = first_rec;
    for (uint64_t k = (uint64_t)lo + threadIdx.x; k < z; k += kThreads) {
        const uint64_t s = recs[k].start;
        if (s >= tile_end) break;
        head[padded(s <= tile_base ? 0 : (int)(s - tile_base))] = (uint32_t)(k - lo) + 1u;
    }
    __syncthreads();
    OpMax<uint32_t> op;
    uint32_t v[kPerThread];
    uint32_t run = 0;
#pragma unroll
    for (int j = 0; j < kPerThread; ++j) {
        run = op(run, head[padded((int)threadIdx.x * kPerThread + j)]);
        v[j] = run;
    }
    uint32_t total;
    const uint32_t carry = block_scan_exclusive<kThreads / 64>(run, op, scan_lds, total);
#pragma unroll
    for (int j = 0; j < kPerThread; ++j) head[padded((int)threadIdx.x * kPerThread + j)] = op(v[j], carry);
    __syncthreads();
    uint32_t unresolved = 0;
#pragma unroll 4
    for (int j = 0; j < kPerThread; ++j) {
        const uint32_t i = (uint32_t)j * kThreads + threadIdx.x;
        if (i >= tile_len) break;
        const uint32_t x = tile_base + i;
        const uint32_t k = lo + head[padded((int)i)] - 1u;
        const Rec f = recs[k];
        uint64_t w;
        if (is_literal(f)) {
            w = kResolved | literals[lit_index[k]];
        } else {
            const bool rc = (f.ref & kRcMask) != 0;
            const uint32_t r = (uint32_t)(f.ref & ~kRcMask), t = x - (uint32_t)f.start;
            const uint32_t y = rc ? r + (uint32_t)f.length - 1u - t : r + t;
            if (y < prefix_len) {
                uint32_t c = prefix[y];
                if (rc) {
                    const uint32_t cc = complement(c);
                    if (cc) c = cc;
                    else atomicMin(&ctl[kCtlComplement], x);
                }
                w = kResolved | c;
            } else {
                w = ((uint64_t)y << 32) | (rc ? kStrand : 0ull);
                ++unresolved;
            }
        }
        state[x - prefix_len] = w;
    }
    unresolved = wave_reduce(unresolved, OpAdd<uint32_t>());
    if (lane_id() == 0 && unresolved) atomicAdd(&active, unresolved);
    __syncthreads();
    if (threadIdx.x == 0) {
        tile_active[blockIdx.x] = active;
        if (active) atomicAdd(&ctl[kCtlActive], active);
    }
}

// One round: every unresolved x reads the word of its source y and takes y's symbol, or y's source with the strands
// composed.  A tile without unresolved positions returns at once (kSkip).
template <bool kSkip>
__global__ __launch_bounds__(kThreads) void decode_jump_kernel(uint64_t *__restrict__ state, uint32_t prefix_len, uint32_t n,
                                                               uint32_t *__restrict__ tile_active,
                                                               uint32_t *__restrict__ ctl, int round) {
    __shared__ uint32_t active;
    if (kSkip && tile_active[blockIdx.x] == 0) return;
    if (threadIdx.x == 0) active = 0;
    __syncthreads();
    const uint32_t decoded = n - prefix_len;
    const uint32_t base = blockIdx.x * (uint32_t)kTile;
    uint32_t unresolved = 0;
    // four positions per lane at a time: their own words first, then the four gathers, all in flight together
#pragma unroll 1
    for (int j0 = 0; j0 < kPerThread; j0 += kJumpBatch) {
        uint32_t idx[kJumpBatch];
        uint64_t w[kJumpBatch], wy[kJumpBatch];
#pragma unroll
        for (int b = 0; b < kJumpBatch; ++b) {
            idx[b] = base + (uint32_t)(j0 + b) * kThreads + threadIdx.x;
            w[b] = idx[b] < decoded ? load_word(state + idx[b]) : kResolved;
        }
#pragma unroll
        for (int b = 0; b < kJumpBatch; ++b)
            wy[b] = (w[b] & kResolved) ? 0ull : load_word(state + ((uint32_t)(w[b] >> 32) - prefix_len));
#pragma unroll
        for (int b = 0; b < kJumpBatch; ++b) {
            if (w[b] & kResolved) continue;
            uint64_t nw;
            if (wy[b] & kResolved) {
                uint32_t c = (uint32_t)(wy[b] & 0xffu);
                if (w[b] & kStrand) {
                    const uint32_t cc = complement(c);
                    if (cc) c = cc;
                    else atomicMin(&ctl[kCtlComplement], prefix_len + idx[b]);
                }
                nw = kResolved | c;
            } else {
                nw = (wy[b] & 0xffffffff00000000ull) | ((w[b] ^ wy[b]) & kStrand);
                ++unresolved;
            }
            store_word(state + idx[b], nw);
        }
    }
    unresolved = wave_reduce(unresolved, OpAdd<uint32_t>());
    if (lane_id() == 0 && unresolved) atomicAdd(&active, unresolved);
    __syncthreads();
    if (threadIdx.x == 0) {
        tile_active[blockIdx.x] = active;
        if (active) atomicAdd(&ctl[kCtlRound + round], active);
    }
}

// out[prefix_len + i] = symbol of state[i]: 8 positions per lane, one 8-byte store (out + prefix_len need not be aligned:
// the ragged head and tail go out byte by byte)
__global__ __launch_bounds__(kThreads) void decode_emit_kernel(const uint64_t *__restrict__ state, uint32_t decoded,
                                                               uint32_t head, uint8_t *__restrict__ out) {
    const uint64_t g = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (g == 0) {
        for (uint32_t i = 0; i < head; ++i) out[i] = (uint8_t)state[i];
        const uint32_t tail = head + ((decoded - head) & ~7u);
        for (uint32_t i = tail; i < decoded; ++i) out[i] = (uint8_t)state[i];
    }
    const uint64_t i = (uint64_t)head + g * 8;
    if (i + 8 > decoded) return;
    unsigned long long packed = 0;
#pragma unroll
    for (int b = 0; b < 8; ++b) packed |= (state[i + b] & 0xffull) << (8 * b);
    *reinterpret_cast<unsigned long long *>(out + i) = packed;
}

// differing positions of two byte arrays; kWide: both 8-byte aligned, eight positions per load
template <bool kWide>
__global__ __launch_bounds__(kThreads) void mismatch_kernel(const uint8_t *__restrict__ a, const uint8_t *__restrict__ b,
                                                            uint64_t n, unsigned long long *__restrict__ out) {
    unsigned long long count = 0, first = ~0ull;
    const uint64_t stride = (uint64_t)gridDim.x * kThreads;
    const uint64_t g = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    uint64_t bytes_from = 0;
    if (kWide) {
        const uint64_t words = n >> 3;
        const unsigned long long *wa = reinterpret_cast<const unsigned long long *>(a);
        const unsigned long long *wb = reinterpret_cast<const unsigned long long *>(b);
        for (uint64_t k = g; k < words; k += stride) {
            const unsigned long long d = wa[k] ^ wb[k];
            if (d == 0) continue;
#pragma unroll
            for (int e = 0; e < 8; ++e)
                if ((d >> (8 * e)) & 0xffull) {
                    ++count;
                    const unsigned long long at = k * 8 + e;
                    first = at < first ? at : first;
                }
        }
        bytes_from = words << 3;
    }
    for (uint64_t i = bytes_from + g; i < n; i += stride)
        if (a[i] != b[i]) {
            ++count;
            first = i < first ? i : first;
        }
    if (count) {
        atomicAdd(&out[0], count);
        atomicMin(&out[1], first);
    }
}

unsigned grid_for(uint64_t items) { return record_grid(items); }

const char *rule_text(uint32_t rule) {
    switch (rule) {
    case kDecodeTiling: return "tiling (start[0] = prefix_len, start[k + 1] = start[k] + length[k], length >= 1)";
    case kDecodeLiteralLength: return "literal length (a literal, ref == start, has length 1)";
    case kDecodeSourceRange: return "source range (ref + length must not exceed start)";
    default: return "unknown rule";
    }
}

}  // namespace

size_t decode_arena_bytes(size_t z, size_t decoded) {
    const size_t tiles = div_up(decoded, (size_t)kTile);
    // flags / literal indices with the scan's tile sums, state words, per-tile counts, control words; 256-byte rounding
    return 4 * z + 4 * (z / kTile + 2) * 2 + 8 * decoded + 4 * tiles + 4 * kCtlWords + 16 * 256;
}

size_t gather_literals(Context &ctx, const Rec *d_recs, size_t z, const uint8_t *d_text, uint8_t *d_literals) {
    if (z == 0) return 0;
    Arena &arena = ctx.arena;
    hipStream_t s = ctx.stream;
    const size_t mark = arena.mark();
    ProfScope ps(ctx.profiler(), "literal_gather", s, 28.0 * (double)z);
    uint32_t *idx = arena.alloc<uint32_t>(z);
    uint32_t *d_total = arena.alloc<uint32_t>(1);
    literal_flag_kernel<<<grid_for(z), kThreads, 0, s>>>(d_recs, z, idx);
    KERNEL_CHECK();
    scan_exclusive_add_u32(idx, idx, z, d_total, arena, s);
    literal_gather_kernel<<<grid_for(z), kThreads, 0, s>>>(d_recs, z, idx, d_text, d_literals);
    KERNEL_CHECK();
    uint32_t total = 0;
    ctx.read_back(d_total, &total, 1);
    arena.rewind(mark);
    return total;
}

DecodeStats decode_on_device(Context &ctx, const Rec *d_recs, size_t z, const uint8_t *d_literals, size_t n_literals,
                             uint8_t *d_out, size_t prefix_len, size_t n, bool tile_skip) {
    Arena &arena = ctx.arena;
    hipStream_t s = ctx.stream;
    const size_t mark = arena.mark();
    struct Rewind {
        Arena &a;
        size_t m;
        ~Rewind() { a.rewind(m); }
    } rewind{arena, mark};
    DecodeStats st;
    const size_t decoded = n - prefix_len;
    const size_t tiles = div_up(decoded, (size_t)kTile);

    uint32_t *ctl = arena.alloc<uint32_t>(kCtlWords);
    uint32_t *lit_index = arena.alloc<uint32_t>(z);
    uint32_t init[kCtlWords] = {0};
    init[kCtlBadLo] = init[kCtlBadLo + 1] = 0xffffffffu;
    init[kCtlComplement] = kNoPosition;
    HIP_CHECK(hipMemcpyAsync(ctl, init, sizeof init, hipMemcpyHostToDevice, s));
    {
        ProfScope ps(ctx.profiler(), "decode_check", s, 28.0 * (double)z);
        decode_check_kernel<<<grid_for(z), kThreads, 0, s>>>(d_recs, z, prefix_len, n, lit_index,
                                                              reinterpret_cast<unsigned long long *>(ctl));
        KERNEL_CHECK();
    }
    uint32_t h[kCtlRound];
    ctx.read_back(ctl, h, kCtlRound);  // (also waits for the copy of init, a local)
    const uint64_t bad = (uint64_t)h[kCtlBadLo] | ((uint64_t)h[kCtlBadLo + 1] << 32);
    if (bad != ~0ull) {
        const uint64_t k = bad >> 3;
        const uint32_t rule = (uint32_t)(bad & 7u);
        throw DecodeRefusal((DecodeRule)rule, k, 0, "decode: record " + std::to_string(k) + " breaks " + rule_text(rule));
    }
    st.n_literals = (uint64_t)h[kCtlLiterals] | ((uint64_t)h[kCtlLiterals + 1] << 32);
    if (st.n_literals != n_literals)
        throw DecodeRefusal(kDecodeLiteralCount, 0, 0, "");  // (the caller names the record: it knows where the records are)

    uint64_t *state = arena.alloc<uint64_t>(decoded);
    uint32_t *tile_active = arena.alloc<uint32_t>(tiles);
    {
        ProfScope ps(ctx.profiler(), "decode_expand", s, 24.0 * (double)z + 8.0 * (double)decoded);
        scan_exclusive_add_u32(lit_index, lit_index, z, nullptr, arena, s);
        decode_expand_kernel<<<(unsigned)tiles, kThreads, 0, s>>>(d_recs, (uint32_t)z, lit_index, d_literals, d_out,
                                                                   (uint32_t)prefix_len, (uint32_t)n, state, tile_active, ctl);
        KERNEL_CHECK();
    }
    uint32_t active = 0;
    ctx.read_back(ctl + kCtlActive, &active, 1);
    st.max_active = active;
    st.resolved_at_expand = decoded - active;
    while (active) {
        if (st.rounds == (uint64_t)kMaxRounds)
            throw std::runtime_error("decode: positions still unresolved after 34 jump rounds (internal error)");
        char name[32];
        snprintf(name, sizeof name, "decode_jump_%02d", (int)st.rounds + 1);
        {
            ProfScope whole(ctx.profiler(), "decode_jump", s, 24.0 * (double)active);
            ProfScope ps(ctx.profiler(), name, s, 24.0 * (double)active);
            if (tile_skip)
                decode_jump_kernel<true><<<(unsigned)tiles, kThreads, 0, s>>>(state, (uint32_t)prefix_len, (uint32_t)n,
                                                                              tile_active, ctl, (int)st.rounds);
            else
                decode_jump_kernel<false><<<(unsigned)tiles, kThreads, 0, s>>>(state, (uint32_t)prefix_len, (uint32_t)n,
                                                                               tile_active, ctl, (int)st.rounds);
            KERNEL_CHECK();
        }
        ctx.read_back(ctl + kCtlRound + st.rounds, &active, 1);
        ++st.rounds;
    }
    uint32_t complement_at = kNoPosition;
    ctx.read_back(ctl + kCtlComplement, &complement_at, 1);
    if (complement_at != kNoPosition)
        throw DecodeRefusal(kDecodeComplement, 0, complement_at, "");
    {
        ProfScope ps(ctx.profiler(), "decode_emit", s, 9.0 * (double)decoded);
        uint8_t *out = d_out + prefix_len;
        uint32_t head = (uint32_t)((8 - (reinterpret_cast<uintptr_t>(out) & 7)) & 7);
        if (head > decoded) head = (uint32_t)decoded;
        const uint64_t lanes = (decoded - head) / 8 + 1;
        decode_emit_kernel<<<(unsigned)div_up(lanes, (uint64_t)kThreads), kThreads, 0, s>>>(state, (uint32_t)decoded, head, out);
        KERNEL_CHECK();
    }
    HIP_CHECK(hipStreamSynchronize(s));
    ctx.prof.collect();
    return st;
}

void count_mismatches(Context &ctx, const uint8_t *d_a, const uint8_t *d_b, size_t n, uint64_t *count, uint64_t *first) {
    *count = 0;
    *first = ~0ull;
    if (n == 0) return;
    Arena &arena = ctx.arena;
    hipStream_t s = ctx.stream;
    const size_t mark = arena.mark();
    unsigned long long *d_out = arena.alloc<unsigned long long>(2);
    const unsigned long long init[2] = {0ull, ~0ull};
    HIP_CHECK(hipMemcpyAsync(d_out, init, sizeof init, hipMemcpyHostToDevice, s));
    {
        ProfScope ps(ctx.profiler(), "mismatch", s, 2.0 * (double)n);
        const bool wide = ((reinterpret_cast<uintptr_t>(d_a) | reinterpret_cast<uintptr_t>(d_b)) & 7) == 0;
        const unsigned grid = grid_for(wide ? div_up(n, (size_t)8) : n);
        if (wide) mismatch_kernel<true><<<grid, kThreads, 0, s>>>(d_a, d_b, n, d_out);
        else mismatch_kernel<false><<<grid, kThreads, 0, s>>>(d_a, d_b, n, d_out);
        KERNEL_CHECK();
    }
    unsigned long long h[2];
    HIP_CHECK(hipMemcpyAsync(h, d_out, sizeof h, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    arena.rewind(mark);
    *count = h[0];
    *first = h[1];
}

}  // namespace nolzss
