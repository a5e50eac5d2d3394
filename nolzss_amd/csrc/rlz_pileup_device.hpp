// rlz_pileup_device.hpp -- what the kernels of rlz_pileup.hip and rlz_consensus.hip share: a base of a packed text, the
// record of a block position, and the eight channels of a position after a resolve.
#pragma once
#include "rlz_index.hpp"

namespace nolzss {

__device__ __forceinline__ uint32_t base_of(uint64_t word, uint32_t pos) {  // big-endian 2-bit codes, 32 per word
    return (uint32_t)(word >> (62u - 2u * (pos & 31u))) & 3u;
}

// first and record of block position p < B, and whether p is a separator
__device__ __forceinline__ uint32_t block_record_of(const TermTable &t, uint32_t p, uint32_t &first, bool &separator) {
    uint32_t k = term_lower_bound(t, p);
    k = k < t.count ? k : t.count - 1;
    separator = t.pos[k] == p;
    first = k ? t.pos[k - 1] + 1u : 0u;
    return k;
}

// The eight channels of position p < B after a resolve; returns the block's base there.  A separator: all zero.
__device__ __forceinline__ uint32_t channels_of(const PileupView &v, const uint64_t *__restrict__ xwords, bool separator,
                                                uint32_t p, uint32_t ch[kPileupChannels]) {
    const uint32_t b = base_of(xwords[p >> 5], p);
    if (separator) {
#pragma unroll
        for (uint32_t c = 0; c < kPileupChannels; ++c) ch[c] = 0u;
        return b;
    }
    const uint4 x = *reinterpret_cast<const uint4 *>(v.xbase + 4ull * p);
    const uint32_t eq = v.depth_eq[p + 1u];
    ch[0] = x.x + (b == 0u ? eq : 0u);
    ch[1] = x.y + (b == 1u ? eq : 0u);
    ch[2] = x.z + (b == 2u ? eq : 0u);
    ch[3] = x.w + (b == 3u ? eq : 0u);
    ch[4] = v.del[p];
    ch[5] = v.ins[p];
    ch[6] = v.depth_rev[p + 1u];
    ch[7] = v.brk[p];
    return b;
}

}  // namespace nolzss
