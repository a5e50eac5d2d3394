// code16.hpp -- the handle on the factor-length codes L* in text order, and the 16-bit form of them.
//
// Between the candidate kernels and the cursor every position's code is written once or twice and read two or three
// times, and on ordinary texts no code comes near 2^16.  Where the packed text-order permutation runs (plain mode,
// up to 2^30 symbols, text_order.hpp) the codes are therefore kept as uint16_t: code16[i] = min(L*[i], max).  A stored
// `max` says "max or more": the true value is in the wide-code list, as (position, code) pairs.  One position may be
// listed twice -- the lower bound the exact search starts from, later its result -- and the larger entry counts.
// Behind the far and exact kernels the host reads the list's count (build_lstar, lpnf.hip): none and the cursor runs
// on the 16-bit array; a few and the array is widened with the list applied; more than the list holds and the stage is
// run again with 32-bit codes.  Everything else keeps 32-bit codes throughout.
#pragma once
#include "common.hpp"

namespace nolzss {

struct WideCodes {
    uint64_t *items = nullptr;  // position | code << 32
    uint32_t *count = nullptr;  // entries appended; beyond cap they are counted but not stored
    uint32_t cap = 0;
    uint32_t max = 0xffffu;  // the saturated code (NOLZSS_CODE16_MAX lowers it)
};

struct LstarCodes {
    uint32_t *wide = nullptr;    // n codes of 32 bits, or null while the 16-bit form is being tried
    uint16_t *narrow = nullptr;  // n codes of 16 bits (the array is padded to a multiple of 8), or null
    WideCodes list;              // with narrow only
    int width = 32;              // of the array the cursor reads: set by build_lstar

    static LstarCodes of(uint32_t *codes) {
        LstarCodes c;
        c.wide = codes;
        return c;
    }
};

// (position, code) to the list for the lanes with `big`: one atomic per wavefront.  May be called under divergence
// (the ballot counts the lanes that are there).
__device__ __forceinline__ void append_wide_code(const WideCodes &wl, uint32_t i, uint32_t code, bool big) {
    const uint64_t bal = __ballot(big);
    if (bal == 0) return;  // (the common case; uniform over the lanes present)
    const int leader = __builtin_ctzll(bal);
    uint32_t slot = 0;
    if (lane_id() == leader) slot = atomicAdd(wl.count, (uint32_t)__popcll(bal));
    slot = (uint32_t)__shfl((int)slot, leader, 64) + (uint32_t)__popcll(bal & lanemask_lt());
    if (big && slot < wl.cap) wl.items[slot] = (uint64_t)i | ((uint64_t)code << 32);
}

// the one way a kernel behind the candidate kernel writes the code of position i
__device__ __forceinline__ void store_code(const LstarCodes &c, uint32_t i, uint32_t code) {
    if (c.narrow == nullptr) {
        c.wide[i] = code;
        return;
    }
    const bool big = code >= c.list.max;
    c.narrow[i] = (uint16_t)(big ? c.list.max : code);
    append_wide_code(c.list, i, code, big);
}
// ... and reads it back as the lower bound of the exact search: a saturated value is a smaller bound, and still one
// at which the predicate holds (it is monotone, nearest.hpp: lpnf_search)
__device__ __forceinline__ uint32_t load_code_bound(const LstarCodes &c, uint32_t i) {
    return c.narrow ? (uint32_t)c.narrow[i] : c.wide[i];
}

}  // namespace nolzss
