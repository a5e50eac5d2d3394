// rlz_pileup_device.hpp -- what the kernels of rlz_pileup.hip and rlz_consensus.hip share: a base of a packed text, the
// record of a block position, the eight channels of a position after a resolve, and the base call of a position (also
// read by rlz_cohort.hip).
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

__device__ __forceinline__ uint32_t depth_of(const uint32_t ch[kPileupChannels]) {  // (below 2^32: rlz_pileup_api.hip)
    return ch[0] + ch[1] + ch[2] + ch[3] + ch[4];
}

// The base call of a non-separator position with block base b (the rule: include/nolzss_hip.h,
// nolzss_rlz_pileup_consensus), shared by the consensus (rlz_consensus.hip) and the pack of a cohort (rlz_cohort.hip):
// d = the depth; true: the position is LOW and `call` means nothing; else call = b if b's counter equals the largest of
// A, C, G, T, DEL, else the smallest channel that attains it (4: DEL).  Loop: the five channels.
__device__ __forceinline__ bool base_call_of(const uint32_t ch[kPileupChannels], uint32_t b, const ConsensusRule &rule,
                                             uint32_t &call, uint64_t &d) {
    d = depth_of(ch);
    uint32_t M = ch[0], arg = 0;
#pragma unroll
    for (uint32_t a = 1; a < 5u; ++a)
        if (ch[a] > M) {  // (strictly: the smallest channel that attains the maximum)
            M = ch[a];
            arg = a;
        }
    call = ch[b] == M ? b : arg;
    return d < rule.min_depth || (uint64_t)M * rule.den < rule.num * d;
}

}  // namespace nolzss
