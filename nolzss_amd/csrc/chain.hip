// chain.hip -- resolves the reference's sequential greedy cursor on the device and emits factors.
//
// The reference advances one factor at a time: lambda = next_leaf(lambda, l)
// (/root/reference/src/cpp/factorizer_core.hpp:113-115).  With L*[i] known for every position,
// the cursor is the chain  p -> next(p) = p + max(1, L*[p])  from start_pos, and the factors are
// exactly the chain positions < n.  mark_chain first runs the speculative cursor (further down: one walk per tile from
// the tile's first position, a path over the tiles, a head fix per reached tile), which is exact on any codes but only
// delivers where the walks meet; where one does not, the exact stages run on the same codes.  They rest on next(p) > p,
// which makes the chain resolvable in O(n) work:
//
//   1. chain_exit_kernel   per 4096-position tile: in-LDS pointer jumping gives exit0[p] = first
//                          chain position at or beyond the tile end; every distinct exit target
//                          is recorded in a bitmap.
//   2. node graph          the marked targets (plus start_pos) are the only positions at which
//                          the chain can ENTER a tile.  They are compacted (bitmap rank) into a
//                          small node list with edges node -> node(exit0[node]).
//   3. wyllie_kernel       pointer doubling with a reached flag over the node list only
//                          (ceil(log2 K) rounds over K << n nodes): reached nodes = tile entries.
//   4. chain_mark_kernel   per entered tile: one lane walks the tile's chain from the entry in LDS
//                          point; the marks go out as one ballot word per wavefront row.
//   5. scan                per-tile counts are scanned: with the bitmap they are the marked chain (mark_chain).
// The outputs are taken from the mark, each by a function of its own (pipeline.hpp): chain_starts writes the marked
// positions in order, chain_records attaches length and leftmost-occurrence reference to them (factor_kernel),
// chain_lengths reads the codes at the marked positions.
#include "pipeline.hpp"
#include "pyramid.hpp"
#include "scan.hpp"

#include <cassert>

namespace nolzss {
namespace {

constexpr int kThreads = 256;
constexpr int kTile = 4096;
constexpr int kPerThread = kTile / kThreads;  // 16
constexpr uint32_t kNone = 0xffffffffu;

// L* codes: bit 31 flags a reverse-complement factor (RC mode only), bits 0..30 the length,
// 0 = literal.
constexpr uint32_t kLenMask = 0x7fffffffu;

__device__ __forceinline__ uint32_t next_pos(uint32_t p, uint32_t code, uint32_t n) {
    const uint32_t L = code & kLenMask;
    const uint64_t nx = (uint64_t)p + (L ? L : 1u);
    return nx > n ? n : (uint32_t)nx;
}

// CodeT = uint16_t (code16.hpp; the array is padded to an even count): two codes per load and lane, and the exit
// leaves as uint16_t too, exit0[p] = exit - tile_end.  That needs no escape: this form only runs when every code is
// below 0xffff, so a position of the tile jumps to less than tile_end + 0xffff (or to n).
template <typename CodeT>
__global__ __launch_bounds__(kThreads) void chain_exit_kernel(const CodeT *__restrict__ lstar, uint32_t n,
                                                              uint32_t start_pos, CodeT *__restrict__ exit0,
                                                              uint32_t *__restrict__ target_bits) {
    constexpr bool kNarrow = sizeof(CodeT) == 2;
    __shared__ __align__(8) uint32_t jump[kTile];
    const uint32_t base = blockIdx.x * (uint32_t)kTile;
    const uint32_t tile_end = (n - base < (uint32_t)kTile) ? n : base + kTile;
    const int tid = threadIdx.x;
    if constexpr (kNarrow) {
        const uint32_t *__restrict__ pairs = reinterpret_cast<const uint32_t *>(lstar);
        const uint32_t last_pair = (n - 1u) >> 1;
        uint32_t ls[kPerThread / 2];  // all loads of the tile in flight together
#pragma unroll
        for (int j = 0; j < kPerThread / 2; ++j) {
            const uint32_t pr = (base >> 1) + j * kThreads + tid;
            ls[j] = pairs[pr < last_pair ? pr : last_pair];  // (no branch around the load)
        }
#pragma unroll
        for (int j = 0; j < kPerThread / 2; ++j) {
            const uint32_t lp = 2u * (j * kThreads + tid);
            const uint32_t p = base + lp;
            uint2 v;
            v.x = (p < n) ? next_pos(p, ls[j] & 0xffffu, n) : n;
            v.y = (p + 1u < n) ? next_pos(p + 1u, ls[j] >> 16, n) : n;
            *reinterpret_cast<uint2 *>(&jump[lp]) = v;
        }
    } else {
        uint32_t ls[kPerThread];  // all loads of the tile in flight together
#pragma unroll
        for (int j = 0; j < kPerThread; ++j) {
            const uint32_t p = base + j * kThreads + tid;
            ls[j] = lstar[p < n ? p : n - 1u];  // (no branch around the load: guarded, each one was waited for on its own)
        }
#pragma unroll
        for (int j = 0; j < kPerThread; ++j) {
            const uint32_t lp = j * kThreads + tid;
            const uint32_t p = base + lp;
            jump[lp] = (p < n) ? next_pos(p, ls[j], n) : n;
        }
    }
    __syncthreads();
    // the thread's own pointers stay in registers through the rounds: a position that has left the tile costs no LDS
    // access any more, one that has not costs a read and a write instead of two reads and a write
    uint32_t own[kPerThread];
#pragma unroll
    for (int j = 0; j < kPerThread; ++j) own[j] = jump[j * kThreads + tid];
    for (int round = 0; round < 13; ++round) {
        int changed = 0;
#pragma unroll
        for (int j = 0; j < kPerThread; ++j) {
            if (own[j] < tile_end) {  // still inside the tile: hop through
                own[j] = jump[own[j] - base];
                jump[j * kThreads + tid] = own[j];
                changed = 1;
            }
        }
        if (!__syncthreads_or(changed)) break;
    }
    if constexpr (kNarrow) {
        uint32_t *__restrict__ exit_pairs = reinterpret_cast<uint32_t *>(exit0);  // (padded to an even count as well)
#pragma unroll
        for (int j = 0; j < kPerThread / 2; ++j) {
            const uint32_t lp = 2u * (j * kThreads + tid);
            const uint32_t p = base + lp;
            if (p < n) {
                const uint2 e = *reinterpret_cast<const uint2 *>(&jump[lp]);
                const bool second = p + 1u < n;
                exit_pairs[p >> 1] = ((e.x - tile_end) & 0xffffu) | (second ? (e.y - tile_end) << 16 : 0u);
                if (e.x < n && (!second || e.y != e.x)) atomicOr(&target_bits[e.x >> 5], 1u << (e.x & 31));
                if (second) {
                    const bool last = (lp + 2u == (uint32_t)kTile) || (p + 2u >= n);
                    if (e.y < n && (last || jump[lp + 2] != e.y)) atomicOr(&target_bits[e.y >> 5], 1u << (e.y & 31));
                }
            }
        }
    } else {
#pragma unroll
        for (int j = 0; j < kPerThread; ++j) {
            const uint32_t lp = j * kThreads + tid;
            const uint32_t p = base + lp;
            if (p < n) {
                const uint32_t e = jump[lp];
                exit0[p] = e;
                const bool last = (lp + 1 == (uint32_t)kTile) || (p + 1 >= n);
                if (e < n && (last || jump[lp + 1] != e)) atomicOr(&target_bits[e >> 5], 1u << (e & 31));
            }
        }
    }
    if (blockIdx.x == 0 && tid == 0 && start_pos < n) atomicOr(&target_bits[start_pos >> 5], 1u << (start_pos & 31));
}

__global__ __launch_bounds__(kThreads) void popcount_kernel(const uint32_t *__restrict__ bits, uint32_t nwords,
                                                            uint32_t *__restrict__ counts) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t w = (size_t)blockIdx.x * blockDim.x + threadIdx.x; w < nwords; w += stride)
        counts[w] = (uint32_t)__popc(bits[w]);
}

__global__ __launch_bounds__(kThreads) void node_fill_kernel(const uint32_t *__restrict__ bits,
                                                             const uint32_t *__restrict__ prefix, uint32_t nwords,
                                                             uint32_t *__restrict__ node_pos) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t w = (size_t)blockIdx.x * blockDim.x + threadIdx.x; w < nwords; w += stride) {
        uint32_t b = bits[w];
        uint32_t id = prefix[w];
        while (b) {
            const int bit = __ffs((int)b) - 1;
            node_pos[id++] = (uint32_t)(w * 32 + bit);
            b &= b - 1;
        }
    }
}

__device__ __forceinline__ uint32_t node_id(const uint32_t *bits, const uint32_t *prefix, uint32_t p) {
    return prefix[p >> 5] + (uint32_t)__popc(bits[p >> 5] & ((1u << (p & 31)) - 1u));
}

// nxt[k] = node reached by one exit0 hop; K = terminal.  reach[] initialised to "start node only".
// (ExitT = uint16_t: the exit counts from the end of the node's tile, chain_exit_kernel)
template <typename ExitT>
__global__ __launch_bounds__(kThreads) void node_edges_kernel(const uint32_t *__restrict__ node_pos, uint32_t K,
                                                              const ExitT *__restrict__ exit0, uint32_t n,
                                                              const uint32_t *__restrict__ bits,
                                                              const uint32_t *__restrict__ prefix,
                                                              uint32_t start_pos, uint32_t *__restrict__ nxt,
                                                              uint32_t *__restrict__ reach) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x; k <= K; k += stride) {
        if (k == K) {
            nxt[k] = K;
            reach[k] = 0;
            continue;
        }
        const uint32_t p = node_pos[k];
        uint32_t e = exit0[p];
        if constexpr (sizeof(ExitT) == 2) {
            const uint32_t tbase = p / (uint32_t)kTile * (uint32_t)kTile;
            e += (n - tbase < (uint32_t)kTile) ? n : tbase + kTile;
        }
        nxt[k] = (e >= n) ? K : node_id(bits, prefix, e);
        reach[k] = (p == start_pos) ? 1u : 0u;
    }
}

__global__ __launch_bounds__(kThreads) void wyllie_kernel(const uint32_t *__restrict__ nxt_in,
                                                          uint32_t *__restrict__ nxt_out, uint32_t K,
                                                          uint32_t *reach) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x; k < K; k += stride) {
        const uint32_t w = nxt_in[k];
        if (w < K) {
            if (reach[k]) reach[w] = 1u;  // monotone flag: races only ever add true chain nodes
            nxt_out[k] = nxt_in[w];
        } else {
            nxt_out[k] = K;
        }
    }
}

__global__ __launch_bounds__(kThreads) void tile_entries_kernel(const uint32_t *__restrict__ node_pos,
                                                                const uint32_t *__restrict__ reach, uint32_t K,
                                                                uint32_t *__restrict__ entry) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x; k < K; k += stride)
        if (reach[k]) {
            const uint32_t p = node_pos[k];
            entry[p / kTile] = p;
        }
}

// One wavefront per entered tile: the tile's local jump table goes to LDS (all loads in flight
// together), then ONE lane walks the chain from the entry position -- a tile holds about
// kTile / (mean factor length) factor starts, i.e. a few hundred dependent LDS reads, far cheaper
// than the log2(kTile) rounds of pointer doubling over all 4096 positions this replaced (3.9 ->
// 2.6 ms at 2^30 bases); many such single-wave workgroups share a CU.
template <typename CodeT>
__global__ __launch_bounds__(64) void chain_mark_kernel(const CodeT *__restrict__ lstar, uint32_t n,
                                                        const uint32_t *__restrict__ entry,
                                                        unsigned long long *__restrict__ chain_bits,
                                                        uint32_t *__restrict__ tile_count) {
    __shared__ __align__(4) uint16_t jmp[kTile];
    __shared__ unsigned long long bits[kTile / 64];
    const uint32_t base = blockIdx.x * (uint32_t)kTile;
    const uint32_t tile_end = (n - base < (uint32_t)kTile) ? n : base + kTile;
    const int lane = threadIdx.x;
    const uint32_t e = entry[blockIdx.x];
    const size_t word0 = (size_t)blockIdx.x * (kTile / 64);
    if (e == kNone) {  // the chain jumps over this tile
        chain_bits[word0 + lane] = 0ull;
        if (lane == 0) tile_count[blockIdx.x] = 0;
        return;
    }
    constexpr int kBatch = 16;
    auto local_next = [&](uint32_t p, uint32_t code) -> uint32_t {  // kTile: leaves the tile
        if (p >= n) return (uint32_t)kTile;
        const uint32_t nx = next_pos(p, code, n);
        return nx < tile_end ? nx - base : (uint32_t)kTile;
    };
    if constexpr (sizeof(CodeT) == 2) {  // two codes per load and lane (the array is padded to an even count)
        const uint32_t *__restrict__ pairs = reinterpret_cast<const uint32_t *>(lstar);
        const uint32_t last_pair = (n - 1u) >> 1;
        for (int j0 = 0; j0 < kTile / 128; j0 += kBatch) {
            uint32_t ls[kBatch];
#pragma unroll
            for (int j = 0; j < kBatch; ++j) {
                const uint32_t pr = (base >> 1) + (uint32_t)(j0 + j) * 64u + lane;
                ls[j] = pairs[pr < last_pair ? pr : last_pair];
            }
#pragma unroll
            for (int j = 0; j < kBatch; ++j) {
                const uint32_t lp = 2u * ((uint32_t)(j0 + j) * 64u + lane);
                const uint32_t p = base + lp;
                *reinterpret_cast<uint32_t *>(&jmp[lp]) = local_next(p, ls[j] & 0xffffu) | (local_next(p + 1u, ls[j] >> 16) << 16);
            }
        }
    } else {
        for (int j0 = 0; j0 < kTile / 64; j0 += kBatch) {
            uint32_t ls[kBatch];
#pragma unroll
            for (int j = 0; j < kBatch; ++j) {
                const uint32_t p = base + (uint32_t)(j0 + j) * 64u + lane;
                ls[j] = lstar[p < n ? p : n - 1u];
            }
#pragma unroll
            for (int j = 0; j < kBatch; ++j) {
                const uint32_t lp = (uint32_t)(j0 + j) * 64u + lane;
                jmp[lp] = (uint16_t)local_next(base + lp, ls[j]);
            }
        }
    }
    bits[lane] = 0ull;
    __syncthreads();  // (one wavefront: a fence)
    if (lane == 0) {
        uint32_t p = e - base, cnt = 0;
        while (p < (uint32_t)kTile) {
            bits[p >> 6] |= 1ull << (p & 63);
            ++cnt;
            p = jmp[p];
        }
        tile_count[blockIdx.x] = cnt;
    }
    __syncthreads();
    chain_bits[word0 + lane] = bits[lane];
}

// ---- the speculative cursor ("cursor") ----------------------------------------------------------------------
// next() is monotone on real codes (L*[i + 1] >= L*[i] - 1), so the chains from two positions of a tile merge within a
// few hops.  Every tile is therefore walked ONCE, from its first position, before its true entry is known; the exits of
// those walks give a path over the tiles, and a reached tile whose true entry is another position only walks from that
// entry until it lands on a marked position.  The result is exact whatever the codes are: a tile whose walk from the
// entry neither meets the speculative walk nor leaves at the same exit raises a flag, and mark_chain then runs the
// exact stages above on the same codes.
constexpr uint32_t kVisited = 0x8000u;  // on a jump table entry (<= kTile = 0x1000): the walk came past

// the tile's jump table: jmp[lp] = position behind lp within the tile, kTile: leaves it (or lp is no position).  Local
// positions [from, from + count), from and count multiples of 128; table index = lp - from.
// kBatch loads per lane are in flight together.
template <typename CodeT, int kBatch>
__device__ __forceinline__ void load_jumps(const CodeT *__restrict__ lstar, uint32_t n, uint32_t base, uint32_t tile_end,
                                           uint32_t from, uint32_t count, uint16_t *jmp, int lane) {
    auto local_next = [&](uint32_t p, uint32_t code) -> uint32_t {
        if (p >= n) return (uint32_t)kTile;
        const uint32_t nx = next_pos(p, code, n);
        return nx < tile_end ? nx - base : (uint32_t)kTile;
    };
    if constexpr (sizeof(CodeT) == 2) {  // two codes per load and lane (the array is padded to an even count)
        const uint32_t *__restrict__ pairs = reinterpret_cast<const uint32_t *>(lstar);
        const uint32_t last_pair = (n - 1u) >> 1;
        for (uint32_t j0 = 0; j0 < count / 128u; j0 += kBatch) {
            uint32_t ls[kBatch];
#pragma unroll
            for (int j = 0; j < kBatch; ++j) {
                const uint32_t pr = ((base + from) >> 1) + (j0 + j) * 64u + lane;
                ls[j] = pairs[pr < last_pair ? pr : last_pair];
            }
#pragma unroll
            for (int j = 0; j < kBatch; ++j) {
                const uint32_t i = 2u * ((j0 + j) * 64u + lane);
                if (i < count) {
                    const uint32_t p = base + from + i;
                    *reinterpret_cast<uint32_t *>(&jmp[i]) = local_next(p, ls[j] & 0xffffu) | (local_next(p + 1u, ls[j] >> 16) << 16);
                }
            }
        }
    } else {
        for (uint32_t j0 = 0; j0 < count / 64u; j0 += kBatch) {
            uint32_t ls[kBatch];
#pragma unroll
            for (int j = 0; j < kBatch; ++j) {
                const uint32_t p = base + from + (j0 + j) * 64u + lane;
                ls[j] = lstar[p < n ? p : n - 1u];
            }
#pragma unroll
            for (int j = 0; j < kBatch; ++j) {
                const uint32_t i = (j0 + j) * 64u + lane;
                if (i < count) jmp[i] = (uint16_t)local_next(base + from + i, ls[j]);
            }
        }
    }
}

// Step 1, one wavefront per tile: the walk from the tile's first position (in the tile of start_pos: from start_pos;
// the tiles in front of it hold no chain position and only report a terminal exit).  Writes the 64 bitmap words of the
// walk and spec_exit[t] = the first position of the walk at or behind the tile end (n: the walk ends the text).
// The walking lane only flags the table entries it passes -- a store nothing waits for -- and the 64 lanes collect the
// flags into words afterwards: a read-modify-write of a bitmap word per hop made every hop two dependent LDS accesses.
template <typename CodeT>
__global__ __launch_bounds__(64) void chain_spec_walk_kernel(const CodeT *__restrict__ lstar, uint32_t n, uint32_t start_pos,
                                                             unsigned long long *__restrict__ chain_bits,
                                                             uint32_t *__restrict__ spec_exit) {
    __shared__ __align__(16) uint16_t jmp[kTile];
    const uint32_t base = blockIdx.x * (uint32_t)kTile;
    const uint32_t tile_end = (n - base < (uint32_t)kTile) ? n : base + kTile;
    const int lane = threadIdx.x;
    if (tile_end <= start_pos) {
        if (lane == 0) spec_exit[blockIdx.x] = n;
        return;
    }
    load_jumps<CodeT, 16>(lstar, n, base, tile_end, 0u, (uint32_t)kTile, jmp, lane);
    __syncthreads();  // (one wavefront: a fence)
    if (lane == 0) {
        uint32_t p = start_pos > base ? start_pos - base : 0u, last;
        do {
            last = p;
            const uint32_t nx = jmp[p];
            jmp[p] = (uint16_t)(nx | kVisited);
            p = nx;
        } while (p < (uint32_t)kTile);
        spec_exit[blockIdx.x] = next_pos(base + last, lstar[base + last], n);
    }
    __syncthreads();
    // lane l gathers the flags of positions 64 l .. 64 l + 63, eight positions per 16-byte read; the lanes start at
    // different eighths, which spreads one instruction's reads over the banks
    const uint4 *rows = reinterpret_cast<const uint4 *>(jmp);
    unsigned long long word = 0ull;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int c = (k + lane) & 7;
        const uint4 v = rows[lane * 8 + c];
        auto two = [](uint32_t d) -> uint32_t { return ((d >> 15) & 1u) | ((d >> 30) & 2u); };
        const uint32_t b = two(v.x) | (two(v.y) << 2) | (two(v.z) << 4) | (two(v.w) << 6);
        word |= (unsigned long long)b << (8 * c);
    }
    chain_bits[(size_t)blockIdx.x * (kTile / 64) + lane] = word;
}

// Step 2 runs wyllie_kernel over the tiles: nxt[t] = tile of spec_exit[t] (num_tiles: none), reached from the tile of
// start_pos.
__global__ __launch_bounds__(kThreads) void spec_edges_kernel(const uint32_t *__restrict__ spec_exit, uint32_t n,
                                                              uint32_t num_tiles, uint32_t start_tile,
                                                              uint32_t *__restrict__ nxt, uint32_t *__restrict__ reach,
                                                              uint32_t *__restrict__ entry) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x; t <= num_tiles; t += stride) {
        const uint32_t e = t < num_tiles ? spec_exit[t] : n;
        nxt[t] = e >= n ? num_tiles : e / (uint32_t)kTile;
        reach[t] = t == start_tile ? 1u : 0u;
        if (t < num_tiles) entry[t] = kNone;
    }
}

// entry[t'] = spec_exit[t] for the reached tiles t: a path gives every tile one reached predecessor at the most
__global__ __launch_bounds__(kThreads) void spec_entries_kernel(const uint32_t *__restrict__ spec_exit,
                                                                const uint32_t *__restrict__ reach, uint32_t n,
                                                                uint32_t num_tiles, uint32_t start_pos,
                                                                uint32_t *__restrict__ entry) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x; t < num_tiles; t += stride) {
        if (!reach[t]) continue;
        if (t == start_pos / (uint32_t)kTile) entry[t] = start_pos;
        const uint32_t e = spec_exit[t];
        if (e < n) entry[e / (uint32_t)kTile] = e;
    }
}

// Step 3, one wavefront per tile.  Not reached: the words are cleared.  Entered where step 1 began its walk: the words
// stand.  Entered elsewhere: one lane walks from the entry (codes loaded kFixChunk positions at a time, from the entry
// on) until it lands on a position m that step 1 marked: from m on the two walks are one, so the words are the new
// marks plus the marks of step 1 at and behind m.  A walk that leaves the tile without landing on a mark is accepted if
// it leaves at spec_exit[t] -- no mark of step 1 survives then -- and counted in *failed otherwise.
constexpr uint32_t kFixChunk = 1024;
template <typename CodeT>
__global__ __launch_bounds__(64) void chain_spec_fix_kernel(const CodeT *__restrict__ lstar, uint32_t n, uint32_t start_pos,
                                                            const uint32_t *__restrict__ entry,
                                                            const uint32_t *__restrict__ spec_exit,
                                                            unsigned long long *__restrict__ chain_bits,
                                                            uint32_t *__restrict__ tile_count, uint32_t *__restrict__ failed,
                                                            uint32_t fail_tile) {
    __shared__ __align__(16) uint16_t jmp[kFixChunk];
    __shared__ unsigned long long spec[kTile / 64], mine[kTile / 64];
    __shared__ uint32_t state[3];  // where the walk stands, what ended it, the last position it marked
    enum : uint32_t { kGoOn = 0, kMerged = 1, kLeft = 2 };
    const uint32_t base = blockIdx.x * (uint32_t)kTile;
    const uint32_t tile_end = (n - base < (uint32_t)kTile) ? n : base + kTile;
    const int lane = threadIdx.x;
    const size_t word0 = (size_t)blockIdx.x * (kTile / 64);
    const uint32_t e = entry[blockIdx.x];
    if (lane == 0 && blockIdx.x == fail_tile) atomicAdd(failed, 1u);  // (tests: fail_tile is kNone otherwise)
    if (e == kNone) {
        chain_bits[word0 + lane] = 0ull;
        if (lane == 0) tile_count[blockIdx.x] = 0;
        return;
    }
    unsigned long long word = chain_bits[word0 + lane];
    const uint32_t walked_from = start_pos > base ? start_pos : base;
    if (e != walked_from) {
        spec[lane] = word;
        mine[lane] = 0ull;
        __syncthreads();  // (one wavefront: a fence)
        uint32_t p = e - base, status = kGoOn, last = p;
        while (status == kGoOn) {
            const uint32_t from = p & ~127u;
            const uint32_t count = (uint32_t)kTile - from < kFixChunk ? (uint32_t)kTile - from : kFixChunk;
            if (!((spec[p >> 6] >> (p & 63)) & 1ull)) load_jumps<CodeT, (int)(kFixChunk / 128u * sizeof(CodeT) / 2u)>(lstar, n, base, tile_end, from, count, jmp, lane);
            __syncthreads();
            if (lane == 0) {
                for (;;) {
                    if (p >= (uint32_t)kTile) {
                        status = kLeft;
                        break;
                    }
                    if ((spec[p >> 6] >> (p & 63)) & 1ull) {
                        status = kMerged;
                        break;
                    }
                    if (p >= from + count) break;  // the next chunk
                    mine[p >> 6] |= 1ull << (p & 63);
                    last = p;
                    p = jmp[p - from];
                }
                state[0] = p;
                state[1] = status;
                state[2] = last;
            }
            __syncthreads();
            p = state[0];
            status = state[1];
            last = state[2];
        }
        unsigned long long keep = 0ull;
        if (status == kMerged) {
            const uint32_t mw = p >> 6;
            keep = (uint32_t)lane > mw ? ~0ull : ((uint32_t)lane == mw ? ~0ull << (p & 63) : 0ull);
        } else if (lane == 0 && next_pos(base + last, lstar[base + last], n) != spec_exit[blockIdx.x]) {
            atomicAdd(failed, 1u);
        }
        word = mine[lane] | (word & keep);
        chain_bits[word0 + lane] = word;
    }
    const uint32_t c = (uint32_t)__popcll(word);
    const uint32_t total = wave_scan_inclusive(c, OpAdd<uint32_t>());
    if (lane == 63) tile_count[blockIdx.x] = total;
}

// one wavefront per tile: lane l owns bitmap word l of the tile
__global__ __launch_bounds__(64) void emit_positions_kernel(const unsigned long long *__restrict__ chain_bits,
                                                            const uint32_t *__restrict__ tile_off,
                                                            uint32_t *__restrict__ fpos) {
    const int lane = threadIdx.x;
    const size_t word = (size_t)blockIdx.x * (kTile / 64) + lane;
    unsigned long long b = chain_bits[word];
    const uint32_t c = (uint32_t)__popcll(b);
    uint32_t off = wave_scan_inclusive(c, OpAdd<uint32_t>()) - c + tile_off[blockIdx.x];
    const uint32_t p0 = blockIdx.x * (uint32_t)kTile + lane * 64u;
    while (b) {
        const int bit = __ffsll((long long)b) - 1;
        fpos[off++] = p0 + (uint32_t)bit;
        b &= b - 1;
    }
}

// Factor lengths straight from the marked chain (ChainLengthsOut, pipeline.hpp): length = max(1, code & kLenMask),
// bit 31 = reverse-complement strand (kRC only).  Each workgroup walks words of chain_bits grid-stride and counts in
// LDS; at the end it makes one global atomic add per non-zero bin (integer counts: the result does not depend on the
// order of the adds).  Lengths >= T go to the tail list, which cannot overflow: the lengths of the factors sum to at
// most n, so at most floor(n / T) of them reach T.
template <bool kRC>
__global__ __launch_bounds__(kThreads) void length_hist_kernel(const unsigned long long *__restrict__ chain_bits,
                                                               uint32_t nwords, const uint32_t *__restrict__ lstar,
                                                               uint32_t *__restrict__ hist,
                                                               uint64_t *__restrict__ tail,
                                                               uint32_t *__restrict__ tail_count, uint32_t tail_cap) {
    constexpr uint32_t T = kLengthHistBins;
    constexpr uint32_t kBins = kRC ? 2 * T : T;
    __shared__ uint32_t h[kBins];
    for (uint32_t b = threadIdx.x; b < kBins; b += kThreads) h[b] = 0;
    __syncthreads();
    const uint32_t stride = gridDim.x * kThreads;
    for (uint32_t w = blockIdx.x * kThreads + threadIdx.x; w < nwords; w += stride) {
        unsigned long long b = chain_bits[w];
        while (b) {
            const int bit = __ffsll((long long)b) - 1;
            b &= b - 1;
            const uint32_t code = lstar[(size_t)w * 64 + (uint32_t)bit];
            const uint32_t strand = kRC ? (code >> 31) : 0u;
            uint32_t L = code & kLenMask;
            L = L ? L : 1u;
            if (L < T) {
                atomicAdd(&h[strand * T + L], 1u);
            } else {
                const uint32_t slot = atomicAdd(tail_count, 1u);
                assert(slot < tail_cap);
                if (slot < tail_cap) tail[slot] = (uint64_t)L | ((uint64_t)strand << 32);
            }
        }
    }
    __syncthreads();
    for (uint32_t b = threadIdx.x; b < kBins; b += kThreads)
        if (h[b]) atomicAdd(&hist[b], h[b]);
}

// fpos[k] (a factor start) -> the length of factor k, in place
__global__ __launch_bounds__(kThreads) void gather_lengths_kernel(uint32_t *__restrict__ fpos, uint32_t z,
                                                                  const uint32_t *__restrict__ lstar) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x; k < z; k += stride) {
        const uint32_t L = lstar[fpos[k]] & kLenMask;
        fpos[k] = L ? L : 1u;
    }
}

// ranks the factor kernel walks one by one around ISA[i] before it asks the pyramids: the interval
// of a short factor holds all occurrences of a 12- to 14-mer, dozens to hundreds of ranks, and every
// step of the walk is a dependent load (48 -> 4: 14.5 -> 11 ms per 52 M factors)
constexpr uint32_t kEmitScan = 4;

struct FactorRec {
    uint64_t start, length, ref;
};

// (start, length, ref) per factor.
//   forward factor: ref = leftmost occurrence of the factor string = min SA over I(L)
//     (the reference reports v_min / u_min, factorizer_core.hpp:91,100,105; in RC mode
//     best_fwd_start, :284,360 -- the minimum over I(L) in both of the cases DESIGN.md 3 lists);
//   reverse-complement factor (kRC): the reference keeps the smallest T-coordinate END among the
//     rc-strand suffixes of the node (rc_ends = 2N - SA, factorizer_core.hpp:226-228, 270,
//     294-296), i.e. the LARGEST SA value in I(L); ref = RC_MASK | (end - L + 1)  (:362-364).
// kRebase (merged batch, plain mode): start and ref leave relative to the first position of the factor's
// record (a separate pass over the records cost 2.3 ms per 7*10^7 factors).
// CodeT = uint16_t: the 16-bit codes of plain mode (code16.hpp; no flag, and every code below the saturation value).
template <bool kRC, bool kRebase, typename CodeT = uint32_t>
__global__ __launch_bounds__(kThreads) void factor_kernel(const uint32_t *__restrict__ fpos, uint32_t z,
                                                          const CodeT *__restrict__ lstar,
                                                          const uint32_t *__restrict__ isa,
                                                          const uint32_t *__restrict__ sa,
                                                          const uint32_t *__restrict__ lcp, Pyramid Psa,
                                                          Pyramid Plcp, Pyramid Pmax, uint32_t rcN,
                                                          FactorRec *__restrict__ out, TermTable terms, uint32_t n) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x; k < z; k += stride) {
        const uint32_t i = fpos[k];
        // the factors tile the text: the length is the distance to the next factor (a coalesced read) -- the
        // length code itself is needed only to tell a literal from a match of one symbol, and for the
        // reverse-complement flag
        const uint32_t nxt = k + 1 < z ? fpos[k + 1] : n;
        uint32_t code = nxt - i;
        if (kRC || code == 1u) code = lstar[i];
        const uint32_t L = code & kLenMask;
        const bool is_rc = kRC && (code >> 31);
        FactorRec f;
        f.start = i;
        if (L == 0) {  // literal: factorizer_core.hpp:83-88 / :305-316, 354-357
            f.length = 1;
            f.ref = i;
        } else {
            const uint32_t r = isa[i] - 1u;  // (1-based, pipeline.hpp)
            uint32_t lo = r, hi = r + 1, steps = 0;
            while (lcp[lo] >= L) {  // lcp[0] = 0 stops the scan
                --lo;
                if (++steps == kEmitScan) {
                    lo = (uint32_t)pyr_nearest_left<false>(Plcp, lo, L);
                    break;
                }
            }
            steps = 0;
            while (lcp[hi] >= L) {  // lcp[n] = 0 stops the scan
                ++hi;
                if (++steps == kEmitScan) {
                    hi = pyr_nearest_right<false>(Plcp, hi, L);
                    break;
                }
            }
            hi -= 1;
            f.length = L;
            if (!is_rc) {
                uint32_t mn;
                if (hi - lo < 2 * kEmitScan) {
                    mn = kNone;
                    for (uint32_t q = lo; q <= hi; ++q) {
                        const uint32_t v = sa[q];
                        mn = v < mn ? v : mn;
                    }
                } else {
                    mn = pyr_range<false>(Psa, lo, hi);
                }
                f.ref = mn;
            } else {
                uint32_t mx;
                if (hi - lo < 2 * kEmitScan) {
                    mx = 0;
                    for (uint32_t q = lo; q <= hi; ++q) {
                        const uint32_t v = sa[q];
                        mx = v > mx ? v : mx;
                    }
                } else {
                    mx = pyr_range<true>(Pmax, lo, hi);
                }
                const uint64_t end = 2ull * rcN - mx;  // T-coordinate of the last matched base
                f.ref = (1ull << 63) | (end - L + 1);
            }
        }
        if (kRebase) {
            const uint32_t t = term_lower_bound(terms, i);
            const uint64_t base = t ? (uint64_t)terms.pos[t - 1] + 1 : 0;
            f.start -= base;
            f.ref -= base;
        }
        out[k] = f;
    }
}

// The blocks of a wavefront's 64 factors, read by the wavefront together.  A lane that read its own block would ask for
// one line with eight 16-byte loads, and every such instruction would touch 64 different lines: the first form of
// factor_block_kernel did that and was bound by the requests, not by the fills (363 B of fills per factor instead of
// 610, and 10 % SLOWER than factor_kernel; profiles/factor_rank_blocks_ab.txt).  Here eight consecutive lanes read the
// eight quads of ONE line per instruction -- round j brings the block of the j-th factor of every group of eight --
// and the quads change lanes through LDS: every line is requested once.
constexpr uint32_t kNoBlock = 0xffffffffu;
struct BlockQuads {
    uint4 q[8];
};
// round j: quad (lane & 7) of the block that lane (lane & ~7) + j wants (kNoBlock: nothing is read)
__device__ __forceinline__ BlockQuads request_blocks(const RankBlock *__restrict__ blocks, uint32_t want) {
    const int p = lane_id() & 7, g8 = lane_id() & ~7;
    BlockQuads Q;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const uint32_t b = (uint32_t)__shfl((int)want, g8 + j);
        Q.q[j] = make_uint4(0u, 0u, 0u, 0u);
        if (b != kNoBlock) Q.q[j] = reinterpret_cast<const uint4 *>(blocks + b)[p];
    }
    return Q;
}
// rows: 64 x 8 quads of the wavefront's own LDS; quad k of row w sits at slot k ^ (w & 7), so that the eight lanes that
// write one row and the eight that read eight rows each meet eight different quads of the banks
__device__ __forceinline__ RankBlock exchange_blocks(uint4 *rows, const BlockQuads &Q) {
    const int lane = lane_id(), p = lane & 7, g8 = lane & ~7;
#pragma unroll
    for (int j = 0; j < 8; ++j) rows[(g8 + j) * 8 + (p ^ j)] = Q.q[j];
    __builtin_amdgcn_wave_barrier();  // (one wavefront: its LDS accesses execute in order)
    RankBlock B;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const uint4 x = rows[lane * 8 + (k ^ p)], y = rows[lane * 8 + ((4 + k) ^ p)];
        B.sa[4 * k] = x.x;
        B.sa[4 * k + 1] = x.y;
        B.sa[4 * k + 2] = x.z;
        B.sa[4 * k + 3] = x.w;
        B.lcp[4 * k] = y.x;
        B.lcp[4 * k + 1] = y.y;
        B.lcp[4 * k + 2] = y.z;
        B.lcp[4 * k + 3] = y.w;
    }
    __builtin_amdgcn_wave_barrier();
    return B;
}

// factor_kernel of plain mode over the rank blocks (rank_blocks.hpp): the same records, entry for entry.  A look-up
// touches isa[i] and the line of rank r; one line more on a side whose interval leaves the block (the lines of both
// sides are requested together); the pyramids only for an interval that leaves three blocks.  A wavefront keeps its 64
// factors together through the three steps, so the loop runs over wavefront-sized pieces of the factor list.
template <typename CodeT>
__global__ __launch_bounds__(kThreads) void factor_block_kernel(const uint32_t *__restrict__ fpos, uint32_t z,
                                                                const CodeT *__restrict__ lstar,
                                                                const uint32_t *__restrict__ isa,
                                                                const RankBlock *__restrict__ blocks, Pyramid Psa,
                                                                Pyramid Plcp, FactorRec *__restrict__ out, uint32_t n) {
    __shared__ uint4 s_rows[kThreads / 64][64 * 8];
    uint4 *rows = s_rows[threadIdx.x >> 6];
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t k0 = (size_t)blockIdx.x * blockDim.x + (threadIdx.x & ~63u); k0 < z; k0 += stride) {
        const size_t k = k0 + (size_t)lane_id();
        const bool valid = k < z;
        uint32_t i = 0, L = 0;
        if (valid) {
            i = fpos[k];
            const uint32_t nxt = k + 1 < z ? fpos[k + 1] : n;  // (the length, as in factor_kernel)
            uint32_t code = nxt - i;
            if (code == 1u) code = lstar[i];
            L = code & kLenMask;
        }
        const bool search = valid && L != 0;  // (a literal looks nothing up)
        const uint32_t r = search ? isa[i] - 1u : 0u;
        const uint32_t b = r >> kRankBlockShift;
        RankInterval S{};
        {
            const RankBlock C = exchange_blocks(rows, request_blocks(blocks, search ? b : kNoBlock));
            if (search) S = rb_centre(C, r, L);
        }
        const bool left = search && S.need_left, right = search && S.need_right;
        if (__any(left || right)) {
            const auto far_left = [&](uint32_t q, uint32_t x) { return (uint32_t)pyr_nearest_left<false>(Plcp, q, x); };
            const auto far_right = [&](uint32_t q, uint32_t x) { return pyr_nearest_right<false>(Plcp, q, x); };
            const auto range_min = [&](uint32_t a, uint32_t c) { return pyr_range<false>(Psa, a, c); };
            const BlockQuads QL = request_blocks(blocks, left ? b - 1u : kNoBlock);
            const BlockQuads QR = request_blocks(blocks, right ? b + 1u : kNoBlock);
            {
                const RankBlock Lb = exchange_blocks(rows, QL);
                if (left) rb_left(S, Lb, b - 1u, L, far_left, range_min);
            }
            {
                const RankBlock Rb = exchange_blocks(rows, QR);
                if (right) rb_right(S, Rb, b + 1u, L, far_right, range_min);
            }
        }
        if (valid) {
            FactorRec f;
            f.start = i;
            f.length = L ? L : 1u;
            f.ref = L ? S.mn : i;  // literal: (i, 1, i)
            out[k] = f;
        }
    }
}

inline unsigned grid_for(size_t items, unsigned cap = 256u * 16u) {
    size_t g = div_up(items, (size_t)kThreads);
    if (g < 1) g = 1;
    return (unsigned)(g > cap ? cap : g);
}

// The one place that launches factor_kernel: picks the instantiation from what the lookup carries and the code width.
void launch_factor_kernel(Context &ctx, const uint32_t *starts, uint32_t z, uint32_t n, const LstarCodes &codes,
                          const RecordLookup &lk, FactorRec *out) {
    hipStream_t s = ctx.stream;
    const bool narrow = codes.width == 16;
    if (narrow && (lk.Pmax || lk.rebase)) throw HipError("factor records: 16-bit codes are for plain records only");
    if (lk.Pmax && lk.rebase) throw HipError("factor records: record-relative output exists in plain mode only");
    const unsigned g = grid_for(z);
    if (lk.Pmax)
        factor_kernel<true, false><<<g, kThreads, 0, s>>>(starts, z, codes.wide, lk.isa, lk.sa, lk.lcp, lk.Psa, lk.Plcp, *lk.Pmax,
                                                          lk.rcN, out, TermTable{}, n);
    else if (lk.rebase)
        factor_kernel<false, true><<<g, kThreads, 0, s>>>(starts, z, codes.wide, lk.isa, lk.sa, lk.lcp, lk.Psa, lk.Plcp, lk.Psa, 0u,
                                                          out, *lk.rebase, n);
    else if (lk.blocks && narrow)
        factor_block_kernel<uint16_t><<<g, kThreads, 0, s>>>(starts, z, codes.narrow, lk.isa, lk.blocks, lk.Psa, lk.Plcp, out, n);
    else if (lk.blocks)
        factor_block_kernel<uint32_t><<<g, kThreads, 0, s>>>(starts, z, codes.wide, lk.isa, lk.blocks, lk.Psa, lk.Plcp, out, n);
    else if (narrow)
        factor_kernel<false, false, uint16_t><<<g, kThreads, 0, s>>>(starts, z, codes.narrow, lk.isa, lk.sa, lk.lcp, lk.Psa,
                                                                     lk.Plcp, lk.Psa, 0u, out, TermTable{}, n);
    else
        factor_kernel<false, false><<<g, kThreads, 0, s>>>(starts, z, codes.wide, lk.isa, lk.sa, lk.lcp, lk.Psa, lk.Plcp, lk.Psa, 0u,
                                                           out, TermTable{}, n);
    KERNEL_CHECK();
}

}  // namespace

namespace {

// The exact cursor (stages 1 to 5 of the header): right on any codes without a condition; the speculative cursor falls
// back on it.  Fills cbits and tile_count (scanned); returns z.  Its temporaries are released before it returns.
uint32_t mark_chain_exact(Context &ctx, uint32_t n, uint32_t start_pos, const LstarCodes &codes, unsigned long long *cbits,
                          uint32_t *tile_count) {
    hipStream_t s = ctx.stream;
    Arena &arena = ctx.arena;
    const bool narrow = codes.width == 16;
    const uint32_t *lstar = codes.wide;       // !narrow
    const uint16_t *lstar16 = codes.narrow;  // narrow
    const uint32_t num_tiles = (uint32_t)div_up(n, kTile);
    const uint32_t tbits_words = (uint32_t)div_up((size_t)n + 1, 32);

    const size_t tmp = arena.mark();
    uint32_t *exit0 = narrow ? nullptr : arena.alloc<uint32_t>(n);
    uint16_t *exit16 = narrow ? arena.alloc<uint16_t>((size_t)n + 2) : nullptr;
    uint32_t *tbits = arena.alloc<uint32_t>(tbits_words);
    uint32_t *tprefix = arena.alloc<uint32_t>(tbits_words);
    uint32_t *d_total = arena.alloc<uint32_t>(2);
    HIP_CHECK(hipMemsetAsync(tbits, 0, sizeof(uint32_t) * tbits_words, s));
    {
        ProfScope ps(ctx.profiler(), "chain_exit", s, (narrow ? 4.0 : 8.0) * (double)n);
        if (narrow)
            chain_exit_kernel<uint16_t><<<num_tiles, kThreads, 0, s>>>(lstar16, n, start_pos, exit16, tbits);
        else
            chain_exit_kernel<uint32_t><<<num_tiles, kThreads, 0, s>>>(lstar, n, start_pos, exit0, tbits);
        KERNEL_CHECK();
    }
    {
        ProfScope ps(ctx.profiler(), "chain_nodes", s);
        popcount_kernel<<<grid_for(tbits_words), kThreads, 0, s>>>(tbits, tbits_words, tprefix);
        KERNEL_CHECK();
        scan_exclusive_add_u32(tprefix, tprefix, tbits_words, d_total, arena, s);
    }
    uint32_t K = 0;
    ctx.read_back(d_total, &K, 1);

    uint32_t *node_pos = arena.alloc<uint32_t>(K + 1);
    uint32_t *nxt[2] = {arena.alloc<uint32_t>(K + 1), arena.alloc<uint32_t>(K + 1)};
    uint32_t *reach = arena.alloc<uint32_t>(K + 1);
    uint32_t *entry = arena.alloc<uint32_t>(num_tiles);
    {
        ProfScope ps(ctx.profiler(), "chain_nodes", s);
        node_fill_kernel<<<grid_for(tbits_words), kThreads, 0, s>>>(tbits, tprefix, tbits_words, node_pos);
        KERNEL_CHECK();
        if (narrow)
            node_edges_kernel<uint16_t><<<grid_for((size_t)K + 1), kThreads, 0, s>>>(node_pos, K, exit16, n, tbits, tprefix,
                                                                                     start_pos, nxt[0], reach);
        else
            node_edges_kernel<uint32_t><<<grid_for((size_t)K + 1), kThreads, 0, s>>>(node_pos, K, exit0, n, tbits, tprefix,
                                                                                     start_pos, nxt[0], reach);
        KERNEL_CHECK();
    }
    {
        ProfScope ps(ctx.profiler(), "chain_wyllie", s);
        int rounds = 1;
        while ((1ull << rounds) < (uint64_t)K + 1) ++rounds;
        int cur = 0;
        for (int r = 0; r < rounds; ++r) {
            wyllie_kernel<<<grid_for(K), kThreads, 0, s>>>(nxt[cur], nxt[cur ^ 1], K, reach);
            KERNEL_CHECK();
            cur ^= 1;
        }
        HIP_CHECK(hipMemsetAsync(entry, 0xff, sizeof(uint32_t) * num_tiles, s));
        tile_entries_kernel<<<grid_for(K), kThreads, 0, s>>>(node_pos, reach, K, entry);
        KERNEL_CHECK();
    }
    {
        ProfScope ps(ctx.profiler(), "chain_mark", s, (narrow ? 2.0 : 4.0) * (double)n);
        if (narrow)
            chain_mark_kernel<uint16_t><<<num_tiles, 64, 0, s>>>(lstar16, n, entry, cbits, tile_count);
        else
            chain_mark_kernel<uint32_t><<<num_tiles, 64, 0, s>>>(lstar, n, entry, cbits, tile_count);
        KERNEL_CHECK();
        scan_exclusive_add_u32(tile_count, tile_count, num_tiles, d_total + 1, arena, s);
    }
    uint32_t z = 0;
    ctx.read_back(d_total + 1, &z, 1);  // (waits for the stream: the temporaries are no longer read)
    arena.rewind(tmp);
    return z;
}

// The speculative cursor (the kernels above): cbits and tile_count (scanned) are right and *z is set if it returns 0;
// otherwise it returns the number of tiles whose walk from the entry did not meet the walk from the tile start, and
// nothing it wrote counts.  One read-back, of z and that number.  force_fail (NOLZSS_TEST_SPEC_CURSOR_FAILS): the tile of
// start_pos raises the flag on top of what it finds.
uint32_t mark_chain_spec(Context &ctx, uint32_t n, uint32_t start_pos, const LstarCodes &codes, unsigned long long *cbits,
                         uint32_t *tile_count, bool force_fail, uint32_t *z) {
    hipStream_t s = ctx.stream;
    Arena &arena = ctx.arena;
    const bool narrow = codes.width == 16;
    const uint32_t num_tiles = (uint32_t)div_up(n, kTile);
    const uint32_t start_tile = start_pos / (uint32_t)kTile;

    const size_t tmp = arena.mark();
    uint32_t *spec_exit = arena.alloc<uint32_t>(num_tiles);
    uint32_t *nxt[2] = {arena.alloc<uint32_t>(num_tiles + 1), arena.alloc<uint32_t>(num_tiles + 1)};
    uint32_t *reach = arena.alloc<uint32_t>(num_tiles + 1);
    uint32_t *entry = arena.alloc<uint32_t>(num_tiles);
    uint32_t *d_result = arena.alloc<uint32_t>(2);  // z, failed tiles
    const uint32_t fail_tile = force_fail ? start_tile : kNone;
    HIP_CHECK(hipMemsetAsync(d_result, 0, 2 * sizeof(uint32_t), s));
    {
        ProfScope ps(ctx.profiler(), "chain_spec_walk", s, (narrow ? 2.0 : 4.0) * (double)n);
        if (narrow)
            chain_spec_walk_kernel<uint16_t><<<num_tiles, 64, 0, s>>>(codes.narrow, n, start_pos, cbits, spec_exit);
        else
            chain_spec_walk_kernel<uint32_t><<<num_tiles, 64, 0, s>>>(codes.wide, n, start_pos, cbits, spec_exit);
        KERNEL_CHECK();
    }
    {
        ProfScope ps(ctx.profiler(), "chain_spec_path", s);
        spec_edges_kernel<<<grid_for((size_t)num_tiles + 1), kThreads, 0, s>>>(spec_exit, n, num_tiles, start_tile, nxt[0], reach,
                                                                             entry);
        KERNEL_CHECK();
        int rounds = 1;
        while ((1ull << rounds) < (uint64_t)num_tiles + 1) ++rounds;
        int cur = 0;
        for (int r = 0; r < rounds; ++r) {
            wyllie_kernel<<<grid_for(num_tiles), kThreads, 0, s>>>(nxt[cur], nxt[cur ^ 1], num_tiles, reach);
            KERNEL_CHECK();
            cur ^= 1;
        }
        spec_entries_kernel<<<grid_for(num_tiles), kThreads, 0, s>>>(spec_exit, reach, n, num_tiles, start_pos, entry);
        KERNEL_CHECK();
    }
    {
        ProfScope ps(ctx.profiler(), "chain_spec_fix", s);
        if (narrow)
            chain_spec_fix_kernel<uint16_t><<<num_tiles, 64, 0, s>>>(codes.narrow, n, start_pos, entry, spec_exit, cbits, tile_count,
                                                                    d_result + 1, fail_tile);
        else
            chain_spec_fix_kernel<uint32_t><<<num_tiles, 64, 0, s>>>(codes.wide, n, start_pos, entry, spec_exit, cbits, tile_count,
                                                                    d_result + 1, fail_tile);
        KERNEL_CHECK();
        scan_exclusive_add_u32(tile_count, tile_count, num_tiles, d_result, arena, s);
    }
    uint32_t result[2] = {0, 0};
    ctx.read_back(d_result, result, 2);  // (waits for the stream: the temporaries are no longer read)
    arena.rewind(tmp);
    *z = result[0];
    return result[1];
}

}  // namespace

// NOLZSS_NO_SPEC_CURSOR: the exact stages only (A/B runs).  NOLZSS_TEST_SPEC_CURSOR_FAILS: the speculative cursor reports
// a failed tile, so that the fall-back runs on any input (tests).
Chain mark_chain(Context &ctx, uint32_t n, uint32_t start_pos, const LstarCodes &codes) {
    Arena &arena = ctx.arena;
    Chain chain;
    chain.n = n;
    chain.codes = codes;
    ctx.cursor_path = kCursorNone;
    ctx.cursor_failed_tiles = 0;
    if (start_pos >= n) return chain;
    static const bool no_spec = getenv("NOLZSS_NO_SPEC_CURSOR") != nullptr;
    static const bool force_fail = getenv("NOLZSS_TEST_SPEC_CURSOR_FAILS") != nullptr;
    static const bool trace = getenv("NOLZSS_TRACE") != nullptr;

    const uint32_t num_tiles = (uint32_t)div_up(n, kTile);
    // the mark first: everything behind it is released before the caller takes an output
    unsigned long long *cbits = arena.alloc<unsigned long long>((size_t)num_tiles * (kTile / 64));
    uint32_t *tile_count = arena.alloc<uint32_t>(num_tiles);
    uint32_t failed = 0;
    if (!no_spec) failed = mark_chain_spec(ctx, n, start_pos, codes, cbits, tile_count, force_fail, &chain.z);
    if (no_spec || failed) chain.z = mark_chain_exact(ctx, n, start_pos, codes, cbits, tile_count);
    ctx.cursor_path = no_spec ? kCursorExact : (failed ? kCursorFailedOver : kCursorSpeculative);
    ctx.cursor_failed_tiles = failed;
    if (trace)
        fprintf(stderr, "[nolzss] cursor: %s, %u of %u tiles failed\n",
                no_spec ? "exact stages" : (failed ? "speculative walk, then the exact stages" : "speculative walk"), failed,
                num_tiles);
    chain.bits = cbits;
    chain.tile_off = tile_count;
    chain.num_tiles = num_tiles;
    return chain;
}

uint32_t *chain_starts(Context &ctx, const Chain &chain) {
    if (chain.z == 0) return nullptr;
    uint32_t *starts = ctx.arena.alloc<uint32_t>(chain.z);
    ProfScope ps(ctx.profiler(), "factor_emit", ctx.stream);
    emit_positions_kernel<<<chain.num_tiles, 64, 0, ctx.stream>>>(chain.bits, chain.tile_off, starts);
    KERNEL_CHECK();
    return starts;
}

void *chain_records(Context &ctx, const Chain &chain, const uint32_t *starts, const RecordLookup &lookup) {
    if (chain.z == 0) return nullptr;
    FactorRec *recs = ctx.arena.alloc<FactorRec>(chain.z);
    ProfScope ps(ctx.profiler(), "factor_emit", ctx.stream);
    launch_factor_kernel(ctx, starts, chain.z, chain.n, chain.codes, lookup, recs);
    return recs;
}

void *position_factors(Context &ctx, uint32_t n, const LstarCodes &codes, const RecordLookup &lookup) {
    if (n == 0) return nullptr;
    hipStream_t s = ctx.stream;
    uint32_t *fpos = ctx.arena.alloc<uint32_t>(n);
    FactorRec *recs = ctx.arena.alloc<FactorRec>(n);
    std::vector<uint32_t> iota(n);
    for (uint32_t i = 0; i < n; ++i) iota[i] = i;
    HIP_CHECK(hipMemcpyAsync(fpos, iota.data(), (size_t)n * sizeof(uint32_t), hipMemcpyHostToDevice, s));
    HIP_CHECK(hipStreamSynchronize(s));  // iota is a local vector
    launch_factor_kernel(ctx, fpos, n, n, codes, lookup, recs);
    return recs;
}

void chain_lengths(Context &ctx, const Chain &chain, const ChainLengthsOut &out, bool with_strand) {
    hipStream_t s = ctx.stream;
    if (out.order) *out.order = nullptr;
    if (chain.z == 0) return;
    if (chain.codes.width != 32) throw HipError("factor lengths: the length kernels read 32-bit codes");
    const uint32_t *lstar = chain.codes.wide;
    if (out.hist) {
        ProfScope ps(ctx.profiler(), "length_hist", s);
        const uint32_t nwords = chain.num_tiles * (uint32_t)(kTile / 64);
        const unsigned g = grid_for(nwords, 1024);
        if (with_strand)
            length_hist_kernel<true><<<g, kThreads, 0, s>>>(chain.bits, nwords, lstar, out.hist, out.tail, out.tail_count,
                                                            out.tail_cap);
        else
            length_hist_kernel<false><<<g, kThreads, 0, s>>>(chain.bits, nwords, lstar, out.hist, out.tail, out.tail_count,
                                                             out.tail_cap);
        KERNEL_CHECK();
    }
    if (!out.order) return;
    uint32_t *lens = ctx.arena.alloc<uint32_t>(chain.z);  // the starts first, then the lengths in their place
    ProfScope ps(ctx.profiler(), "length_emit", s);
    emit_positions_kernel<<<chain.num_tiles, 64, 0, s>>>(chain.bits, chain.tile_off, lens);
    KERNEL_CHECK();
    gather_lengths_kernel<<<grid_for(chain.z), kThreads, 0, s>>>(lens, chain.z, lstar);
    KERNEL_CHECK();
    *out.order = lens;
}

void chain_outputs(Context &ctx, const Chain &chain, const RecordLookup &lookup, bool with_strand, ChainRequest &rq) {
    rq.z = chain.z;
    rq.d_records = nullptr;
    rq.d_starts = nullptr;
    if (rq.lengths) chain_lengths(ctx, chain, *rq.lengths, with_strand);
    if (!rq.records && !rq.starts) return;
    rq.d_starts = chain_starts(ctx, chain);
    if (rq.records) rq.d_records = chain_records(ctx, chain, rq.d_starts, lookup);
}

}  // namespace nolzss
