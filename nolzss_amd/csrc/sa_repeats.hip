// sa_repeats.hip -- the two arithmetic passes of the suffix-array construction over highly repetitive texts, behind the
// direct rounds: long exact repeats (pair runs) and runs of a short period (periodic runs).  Both order tied suffixes
// from ranks and LCP values that are already decided, without reading the text (the argument stands above each set of
// kernels).  Shared declarations: sa_internal.hpp.
#include "sa_internal.hpp"

#include "scan.hpp"

#include <algorithm>

namespace nolzss {

namespace {

// ---------------------------------------------------------------------------------------
// Long exact repeats.  After the direct round a text with long repeats (similar genomes, a duplicated
// region) is left with millions of small groups of suffixes -- i and i + d for two copies -- that agree
// on more than the cap.  Doubling would need log2(repeat length) rounds over all of them although the
// answer is arithmetic: LCP(i, j) = 1 + LCP(i + 1, j + 1), and the order of (i, j) is the order of
// (i + 1, j + 1).  Along a RUN of text positions i, i + 1, ... whose groups keep the same shape (the same
// distances between the members), everything follows from the group behind the end of the run, and that
// one is already separated (its members carry different rank codes): the order is the order of the codes,
// the LCP of neighbours 1 + the range minimum of the LCP values decided so far -- the rule a doubling step
// applies, with h = 1.  Runs are contiguous in TEXT order, so "where does my run end" is one prefix scan,
// not pointer jumping.  Groups of up to kRunGroupMax members are handled; runs whose end group is only
// partly separated are left to the doubling rounds.
// ---------------------------------------------------------------------------------------

// members of the undecided group with head slot g: k = its size (0: decided or too large)
__device__ __forceinline__ uint32_t run_group_size(const uint32_t *__restrict__ lcp, uint32_t n, uint32_t g) {
    uint32_t k = 1;
    while (k <= kRunGroupMax && g + k < n && lcp[g + k] >= kLcpPendingMin) ++k;
    return (k >= 2 && k <= kRunGroupMax) ? k : 0u;
}

// link[i] = (next member of my group in text order, cyclically) - i, gsz[i] = size of my group; 0 / 0 if
// suffix i is decided or its group is too large
__global__ __launch_bounds__(kThreads) void group_link_kernel(const uint32_t *__restrict__ rank,
                                                              const uint32_t *__restrict__ sa,
                                                              const uint32_t *__restrict__ lcp, uint32_t n,
                                                              uint32_t *__restrict__ link, uint32_t *__restrict__ gsz) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const uint32_t g = rank[i] - 1u;  // head slot of my group
        const uint32_t k = run_group_size(lcp, n, g);
        uint32_t d = 0;
        if (k) {
            uint32_t above = 0xffffffffu, lowest = 0xffffffffu;
            for (uint32_t x = 0; x < k; ++x) {
                const uint32_t m = sa[g + x];
                lowest = m < lowest ? m : lowest;
                if (m > (uint32_t)i && m < above) above = m;
            }
            d = (above != 0xffffffffu ? above : lowest) - (uint32_t)i;
        }
        link[i] = d;
        gsz[i] = d ? k : 0u;
    }
}

// does the chain of position t go on at t + 1?
__device__ __forceinline__ bool run_goes_on(const uint32_t *__restrict__ link, const uint32_t *__restrict__ gsz,
                                            uint32_t n, size_t t) {
    const uint32_t d = link[t];
    return d != 0 && t + 1 < n && link[t + 1] == d && gsz[t + 1] == gsz[t];
}

// rev[n - 1 - t] = (n - 1 - t) + 1 where the chain of t ends at t (or t is in no group), else 0: an
// inclusive max-scan over rev then names, for every t, the nearest such end at or behind it
__global__ __launch_bounds__(kThreads) void run_breaks_kernel(const uint32_t *__restrict__ link,
                                                              const uint32_t *__restrict__ gsz, uint32_t n,
                                                              uint32_t *__restrict__ rev) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x; t < n; t += stride)
        rev[n - 1 - t] = run_goes_on(link, gsz, n, t) ? 0u : (uint32_t)(n - 1 - t) + 1u;
}

// togo[i] = steps until the run of my GROUP ends: the shortest chain of its members (the group one
// step further on is my group shifted by one only while every member's chain goes on)
__global__ __launch_bounds__(kThreads) void group_run_kernel(const uint32_t *__restrict__ gsz,
                                                             const uint32_t *__restrict__ rank,
                                                             const uint32_t *__restrict__ sa,
                                                             const uint32_t *__restrict__ end_of, uint32_t n,
                                                             uint32_t *__restrict__ togo) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const uint32_t k = gsz[i];
        if (k <= 2) continue;  // (a pair's two chains are equally long: run_steps takes its own)
        const uint32_t g = rank[i] - 1u;
        uint32_t best = 0xffffffffu;
        for (uint32_t x = 0; x < k; ++x) {
            const uint32_t m = sa[g + x];
            const uint32_t e = (uint32_t)(n - 1) - (end_of[n - 1 - m] - 1u);  // where the chain of m ends (>= m)
            best = e - m < best ? e - m : best;
        }
        togo[i] = best;
    }
}

// steps from position i to the end of its group's run
__device__ __forceinline__ uint32_t run_steps(uint32_t k, size_t i, uint32_t n, const uint32_t *__restrict__ end_of,
                                              const uint32_t *__restrict__ togo) {
    if (k > 2) return togo[i];
    return ((uint32_t)(n - 1) - (end_of[n - 1 - i] - 1u)) - (uint32_t)i;
}

constexpr uint32_t kRunDeferred = 0xffffffffu;

// Members of a group at the end of its run.  One symbol further on the members carry rank codes; equal
// codes mean "still tied".  The group splits into classes of equal code, in code order: my slot inside
// the group, the first slot of my class (my new group head), and -- if I am the first of a class that is
// not the first -- the LCP to the class in front (decided now).  A class of one is a finished suffix.
__global__ __launch_bounds__(kThreads) void group_end_kernel(const uint32_t *__restrict__ gsz,
                                                             const uint32_t *__restrict__ togo,
                                                             const uint32_t *__restrict__ end_of,
                                                             const uint32_t *__restrict__ rank,
                                                             const uint32_t *__restrict__ sa, uint32_t n, Pyramid Plcp,
                                                             uint32_t *__restrict__ end_place,
                                                             uint32_t *__restrict__ end_head,
                                                             uint32_t *__restrict__ end_lcp) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x; t < n; t += stride) {
        const uint32_t k = gsz[t];
        if (!k || run_steps(k, t, n, end_of, togo) != 0) continue;
        const uint32_t g = rank[t] - 1u;
        uint32_t below = 0, same_before = 0, pred = 0, l = kRunDeferred;
        bool off_end = t + 1 >= n;
        const uint32_t mine = off_end ? 0u : rank[t + 1];  // rank code (head slot + 1) one symbol further on
        for (uint32_t x = 0; x < k; ++x) {
            const uint32_t m = sa[g + x];
            if (m == (uint32_t)t) continue;
            if ((size_t)m + 1 >= n) {  // (every member sees this: the group is left alone as a whole)
                off_end = true;
                continue;
            }
            const uint32_t c = rank[m + 1];
            if (c < mine) {
                ++below;
                pred = c > pred ? c : pred;
            } else if (c == mine && m < (uint32_t)t) {
                ++same_before;
            }
        }
        if (!off_end && same_before == 0 && below > 0) l = 1u + pyr_range<false>(Plcp, pred, mine - 1u);
        end_place[t] = off_end ? kRunDeferred : below + same_before;
        end_head[t] = below;
        end_lcp[t] = l;
    }
}

// every member of every group of a run does what its counterpart in the end group does
__global__ __launch_bounds__(kThreads) void group_members_kernel(const uint32_t *__restrict__ gsz,
                                                                 const uint32_t *__restrict__ togo,
                                                                 const uint32_t *__restrict__ end_of, uint32_t n,
                                                                 const uint32_t *__restrict__ end_place,
                                                                 const uint32_t *__restrict__ end_head,
                                                                 const uint32_t *__restrict__ end_lcp,
                                                                 uint32_t *__restrict__ rank, uint32_t *__restrict__ sa,
                                                                 uint32_t *__restrict__ lcp) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const uint32_t k = gsz[i];
        if (!k) continue;
        const uint32_t steps = run_steps(k, i, n, end_of, togo);
        const size_t e = i + steps;  // my position in the end group of the run
        const uint32_t place = end_place[e];
        if (place == kRunDeferred) continue;
        const uint32_t g = rank[i] - 1u;
        sa[g + place] = (uint32_t)i;
        const uint32_t le = end_lcp[e];
        if (le != kRunDeferred) lcp[g + place] = le + steps;
        rank[i] = g + end_head[e] + 1u;
    }
}

// the active list after a pass: head slot of every element's (new) group, 1 if that group is still undecided
// (the head is the nearest slot at or in front of mine whose boundary is decided; only groups of up to
// kRunGroupMax members were touched, so the walk back is that short -- the list is in slot order, the
// LCP entries it reads are neighbours in memory)
__global__ __launch_bounds__(kThreads) void still_tied_kernel(const uint32_t *__restrict__ act_slot,
                                                              const uint32_t *__restrict__ act_grp, uint32_t m,
                                                              const uint32_t *__restrict__ lcp, uint32_t n,
                                                              uint32_t *__restrict__ head, uint32_t *__restrict__ keep) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t a = (size_t)blockIdx.x * blockDim.x + threadIdx.x; a < m; a += stride) {
        const uint32_t s = act_slot[a], g0 = act_grp[a];
        uint32_t h = g0;
        if (s - g0 < kRunGroupMax) {
            h = s;
            while (h > g0 && lcp[h] >= kLcpPendingMin) --h;
        }
        head[a] = h;
        keep[a] = (h + 1u < n && lcp[h + 1] >= kLcpPendingMin) ? 1u : 0u;
    }
}

__global__ __launch_bounds__(kThreads) void compact_active_kernel(const uint32_t *__restrict__ act_slot,
                                                                  const uint32_t *__restrict__ head,
                                                                  const uint32_t *__restrict__ keep,
                                                                  const uint32_t *__restrict__ pos, uint32_t m,
                                                                  uint32_t *__restrict__ new_slot,
                                                                  uint32_t *__restrict__ new_grp) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t a = (size_t)blockIdx.x * blockDim.x + threadIdx.x; a < m; a += stride)
        if (keep[a]) {
            new_slot[pos[a]] = act_slot[a];
            new_grp[pos[a]] = head[a];
        }
}

// ---------------------------------------------------------------------------------------
// Periodic runs.  On a text with long runs of a short period (a poly-A tract, a tandem repeat, a period-1000
// text) the suffixes of a run tie on whatever depth h has been compared, in groups far larger than the
// pair-run pass takes, and prefix doubling peels only h of them off per round: log2(run length) rounds over
// everything.  The order inside such a group is arithmetic.  Let q be the smallest distance between two
// members of a group in the text, q <= h: the h symbols every member starts with then have period q (two
// members q apart agree on h symbols, so h + q symbols have that period, and every other member starts with
// the same h symbols), a prefix of u^inf for one word u that those h >= q symbols determine.  For a member x let rho(x) = q + lcp(x, x + q): the text keeps that period
// for exactly rho(x) symbols from x; at x + rho(x) it breaks -- with a symbol smaller than the periodic
// continuation ("down", also when the text ends there) or larger ("up").  Two members with different rho
// agree on min(rho) symbols and the one that breaks first goes down below / up above the other; so the group
// in suffix order is: the down members by ascending rho, then the up members by descending rho, the LCP of
// neighbours with different keys being the smaller rho.  Members with the same key stay tied (a smaller
// group for the next pass or the doubling rounds).
// lcp(x, x + q) needs no text: along a run of text positions t, t + 1, .. whose suffixes all have their next
// group member q behind them, lcp(t, t + q) = 1 + lcp(t + 1, t + 1 + q), so it is the distance to the end E
// of that run of positions plus lcp(E, E + q), and suffixes E and E + q are in DIFFERENT groups: their order
// is the order of their rank codes and their LCP the range minimum of the decided LCP entries between them.
// A group with a member for which that fails (E and E + q tied with each other) is left alone as a whole.
// A group whose q exceeds the depth h compared so far (after the 17-base key sort a large group has only
// been compared to depth 17: a 171-base satellite monomer, a period-1000 text) is taken if the TEXT shows
// that its members agree on q symbols -- every member is compared with the next member of its group in text
// order, q symbols deep (per_verify_kernel; q <= kPerVerifyMax) -- and left to the doubling rounds otherwise.
// ---------------------------------------------------------------------------------------
constexpr uint32_t kPerNone = 0xffffffffu;   // gq: no distance seen yet
constexpr uint32_t kPerBad = 0x80000000u;    // gq: flag "leave this group alone" (positions are below 2^31 here)

// count[0] += members beyond the first `limit` of their group, count[1] += groups with more than `limit` members,
// count[2] += groups (the list is in slot order: a member's index inside its group is slot - head), count[3] +=
// members whose successor in the list belongs to the same group and starts at most `near` symbols away in the text
// (tied members keep the order of their text positions through every stable step of the construction, so these are
// -- as an estimate, used to decide whether a pass is worth its sorts -- the members of periodic runs): one atomic
// per counter and workgroup
__global__ __launch_bounds__(kThreads) void per_count_large_kernel(const uint32_t *__restrict__ act_slot,
                                                                   const uint32_t *__restrict__ act_grp, uint32_t m,
                                                                   const uint32_t *__restrict__ sa, uint32_t limit,
                                                                   uint32_t near, uint32_t *__restrict__ count) {
    uint32_t c[4] = {0, 0, 0, 0};
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t a = (size_t)blockIdx.x * blockDim.x + threadIdx.x; a < m; a += stride) {
        const uint32_t slot = act_slot[a], g = act_grp[a];
        const uint32_t j = slot - g;
        c[0] += j >= limit ? 1u : 0u;
        c[1] += j == limit ? 1u : 0u;
        c[2] += j == 0 ? 1u : 0u;
        if (a + 1 < m && act_grp[a + 1] == g) {
            const uint32_t p = sa[slot], q = sa[act_slot[a + 1]];
            const uint32_t d = p < q ? q - p : p - q;
            c[3] += d <= near ? 1u : 0u;
        }
    }
    __shared__ uint32_t s_part[4][kThreads / 64];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const uint32_t r = wave_reduce(c[k], OpAdd<uint32_t>());
        if (lane_id() == 0) s_part[k][threadIdx.x >> 6] = r;
    }
    __syncthreads();
    if (threadIdx.x < 4) {
        uint32_t t = 0;
        for (int i = 0; i < kThreads / 64; ++i) t += s_part[threadIdx.x][i];
        if (t) atomicAdd(count + threadIdx.x, t);
    }
}

// members of groups whose smallest distance between neighbours is at most `limit` (the candidates of the periodic
// pass): one atomic per workgroup
__global__ __launch_bounds__(kThreads) void per_candidates_kernel(const uint64_t *__restrict__ keys, uint32_t m,
                                                                  const uint32_t *__restrict__ gq, uint32_t limit,
                                                                  uint32_t *__restrict__ count) {
    uint32_t mine = 0;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x; j < m; j += stride)
        mine += gq[(uint32_t)(keys[j] >> 32)] <= limit ? 1u : 0u;
    mine = wave_reduce(mine, OpAdd<uint32_t>());
    __shared__ uint32_t s_part[kThreads / 64];
    if (lane_id() == 0) s_part[threadIdx.x >> 6] = mine;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t t = 0;
        for (int i = 0; i < kThreads / 64; ++i) t += s_part[i];
        if (t) atomicAdd(count, t);
    }
}

__global__ __launch_bounds__(kThreads) void per_keys_kernel(const uint32_t *__restrict__ act_slot,
                                                            const uint32_t *__restrict__ act_grp, uint32_t m,
                                                            const uint32_t *__restrict__ sa,
                                                            uint64_t *__restrict__ keys, uint32_t *__restrict__ vals) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t a = (size_t)blockIdx.x * blockDim.x + threadIdx.x; a < m; a += stride) {
        const uint32_t pos = sa[act_slot[a]];
        keys[a] = ((uint64_t)act_grp[a] << 32) | pos;
        vals[a] = pos;
    }
}

// list sorted by (group, position): gq[group] = smallest distance between neighbours.  One atomic per
// workgroup / wavefront where it holds one group only (a giant group would otherwise send every lane to
// one address, 13 ns each).  The grid covers the list exactly once (no stride loop: barriers inside).
__global__ __launch_bounds__(kThreads) void per_link_kernel(const uint64_t *__restrict__ keys, uint32_t m,
                                                            uint32_t *__restrict__ gq) {
    const size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool in = j < m;
    const uint64_t k = in ? keys[j] : 0;
    const uint32_t g = (uint32_t)(k >> 32);
    uint32_t link = kPerNone;
    if (in && j + 1 < m) {
        const uint64_t k2 = keys[j + 1];
        if ((uint32_t)(k2 >> 32) == g) link = (uint32_t)k2 - (uint32_t)k;
    }
    __shared__ uint32_t s_g0, s_min[kThreads / 64];
    if (threadIdx.x == 0) s_g0 = g;
    __syncthreads();
    const int uniform = __syncthreads_and(in && g == s_g0);
    if (uniform) {
        const uint32_t w = wave_reduce(link, OpMinU32x());
        if (lane_id() == 0) s_min[threadIdx.x >> 6] = w;
        __syncthreads();
        if (threadIdx.x == 0) {
            uint32_t b = s_min[0];
            for (int i = 1; i < kThreads / 64; ++i) b = s_min[i] < b ? s_min[i] : b;
            if (b != kPerNone) atomicMin(&gq[g], b);
        }
        return;
    }
    const uint32_t g_first = (uint32_t)__builtin_amdgcn_readfirstlane((int)g);
    if (__ballot(!in || g != g_first) == 0) {  // the wavefront holds one group
        const uint32_t w = wave_reduce(link, OpMinU32x());
        if (lane_id() == 0 && w != kPerNone) atomicMin(&gq[g], w);
    } else if (in && link != kPerNone) {
        atomicMin(&gq[g], link);
    }
}

// PQ[pos] = q for a member whose next group member is exactly q behind it, q = the group's distance (0 for
// everything else; the array was cleared).  Groups whose q exceeds half the depth compared so far are
// flagged; the smallest such q is reported (hint: try again when the depth has passed twice that).

// members of groups with depth < q <= kPerVerifyMax: do I agree with the next member of my group (in text
// order) on q symbols?  If every such pair does, all members agree on q symbols.  Pairs exactly q apart need
// no text: lcp(x, x + q) = (E - x) + lcp(E, E + q) is known from the run of positions (per_rho_kernel).
template <int BITS>
__global__ __launch_bounds__(kThreads) void per_verify_kernel(const uint64_t *__restrict__ keys, uint32_t m,
                                                              uint32_t *__restrict__ gq, uint32_t depth, uint32_t n,
                                                              const uint64_t *__restrict__ words, TermTable terms) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x; j + 1 < m; j += stride) {
        const uint64_t k = keys[j], k2 = keys[j + 1];
        const uint32_t g = (uint32_t)(k >> 32);
        if ((uint32_t)(k2 >> 32) != g) continue;
        const uint32_t gv = *reinterpret_cast<volatile uint32_t *>(&gq[g]);
        if (gv & kPerBad) continue;
        const uint32_t q = gv;
        if (q <= depth || q > kPerVerifyMax) continue;
        // (plain texts only: the later member is the shorter suffix, so "agrees on min(q, what the later one has
        // left)" carries from pair to pair -- every member starts with the group's period word as far as it goes)
        const uint32_t b = (uint32_t)k2, left = n - b, need = q < left ? q : left;
        // (a pair exactly q apart is checked without the text, from the length of its run of positions:
        // per_rho_kernel; what is compared here are the few pairs that join two runs)
        if (b - (uint32_t)k == q) continue;
        if (suffix_lcp<BITS>(words, terms, (uint32_t)k, b, 0u, q) < need) atomicOr(&gq[g], kPerBad);
    }
}

__global__ __launch_bounds__(kThreads) void per_flags_kernel(const uint64_t *__restrict__ keys, uint32_t m,
                                                             uint32_t *__restrict__ gq, uint32_t half_depth,
                                                             uint32_t *__restrict__ PQ, uint32_t *__restrict__ hint) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x; j < m; j += stride) {
        const uint64_t k = keys[j];
        const uint32_t g = (uint32_t)(k >> 32), pos = (uint32_t)k;
        const uint32_t q = *reinterpret_cast<volatile uint32_t *>(&gq[g]) & ~kPerBad;
        const bool head = j == 0 || (uint32_t)(keys[j - 1] >> 32) != g;
        if (q > half_depth) {  // (also kPerNone & ~kPerBad)
            if (head) {
                atomicOr(&gq[g], kPerBad);
                if (q != (kPerNone & ~kPerBad)) lower_min(hint, q);
            }
            continue;
        }
        uint32_t link = 0;
        if (j + 1 < m) {
            const uint64_t k2 = keys[j + 1];
            if ((uint32_t)(k2 >> 32) == g) link = (uint32_t)k2 - pos;
        }
        if (link == q) PQ[pos] = q;
    }
}

// rev[n - 1 - t] = (n - 1 - t) + 1 unless the run of positions goes on from t to t + 1 (both carry the same
// distance): the inclusive max-scan of rev names, for every t, the last position of its run
__global__ __launch_bounds__(kThreads) void per_breaks_kernel(const uint32_t *__restrict__ PQ, uint32_t n,
                                                              uint32_t *__restrict__ rev) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x; t < n; t += stride) {
        const uint32_t q = PQ[t];
        const bool on = q != 0 && t + 1 < n && PQ[t + 1] == q;
        rev[n - 1 - t] = on ? 0u : (uint32_t)(n - 1 - t) + 1u;
    }
}

// sort key of every member: rho for the down members, ~rho for the up members (0 is never a key)
__global__ __launch_bounds__(kThreads) void per_rho_kernel(const uint64_t *__restrict__ keys, uint32_t m,
                                                           uint32_t *__restrict__ gq, const uint32_t *__restrict__ PQ,
                                                           const uint32_t *__restrict__ end_of,
                                                           const uint32_t *__restrict__ rank, uint32_t n, Pyramid Plcp,
                                                           uint32_t depth, uint32_t *__restrict__ kraw) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x; j < m; j += stride) {
        const uint64_t k = keys[j];
        const uint32_t g = (uint32_t)(k >> 32), pos = (uint32_t)k;
        const uint32_t gv = *reinterpret_cast<volatile uint32_t *>(&gq[g]);
        kraw[j] = 0;
        if (gv & kPerBad) continue;
        const uint32_t q = gv;
        // E: the first position at or behind pos whose suffix does NOT have its next group member q behind it
        uint32_t E = pos;
        if (PQ[pos] == q) E = ((n - 1) - (end_of[n - 1 - pos] - 1u)) + 1u;
        bool ok = E < n;
        uint32_t lam = 0, c1 = 0, c2 = 0;
        if (ok && (uint64_t)E + q >= n) {
            // the text ends before suffix E has seen a whole period (only a member without a next member:
            // E = pos): periodic as far as it goes, and the end sorts first
            const uint32_t full = (E - pos) + q, left = n - pos;
            kraw[j] = full < left ? full : left;
            continue;
        }
        if (ok) {
            c1 = rank[E];
            const uint64_t e2 = (uint64_t)E + q;
            c2 = e2 < n ? rank[e2] : 0u;  // (e2 < n here)
            if (c1 == c2) {
                ok = false;  // tied with each other: nothing is known about them yet
            } else if (c2 != 0) {
                const uint32_t a = c1 < c2 ? c1 : c2, b = c1 < c2 ? c2 : c1;
                lam = pyr_range<false>(Plcp, a, b - 1u);  // decided entries between the two groups
                if (lam >= kLcpPendingMin) ok = false;
            }
        }
        if (!ok) {
            atomicOr(&gq[g], kPerBad);
            continue;
        }
        // a group taken on a period longer than the depth compared so far: this member and the next one
        // (q behind it) must agree on q symbols, or as far as the later one goes
        if (q > depth && E != pos) {
            const uint32_t left = n - (pos + q), need = q < left ? q : left;
            if ((E - pos) + lam < need) {
                atomicOr(&gq[g], kPerBad);
                continue;
            }
        }
        const uint32_t rho = (E - pos) + lam + q;  // <= n - pos
        kraw[j] = c2 < c1 ? rho : ~rho;            // down (suffix E + q is the smaller one) : up
    }
}

// second sort key (group, K): K = 0 for every member of a group that is left alone
__global__ __launch_bounds__(kThreads) void per_keys2_kernel(const uint64_t *__restrict__ keys, uint32_t m,
                                                             const uint32_t *__restrict__ gq,
                                                             const uint32_t *__restrict__ kraw,
                                                             uint64_t *__restrict__ keys2, uint32_t *__restrict__ vals2) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x; j < m; j += stride) {
        const uint64_t k = keys[j];
        const uint32_t g = (uint32_t)(k >> 32);
        const uint32_t K = (gq[g] & kPerBad) ? 0u : kraw[j];
        keys2[j] = ((uint64_t)g << 32) | K;
        vals2[j] = (uint32_t)k;
    }
}

// the sorted view the regroup kernel takes, and the LCP of every boundary that appears inside an old group
__global__ __launch_bounds__(kThreads) void per_view_kernel(const uint64_t *__restrict__ keys2,
                                                            const uint32_t *__restrict__ vals2, uint32_t m,
                                                            uint32_t *__restrict__ grp, uint32_t *__restrict__ lo,
                                                            uint32_t *__restrict__ vals, uint32_t *__restrict__ lcp_list) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x; j < m; j += stride) {
        const uint64_t k = keys2[j];
        const uint32_t g = (uint32_t)(k >> 32), K = (uint32_t)k;
        grp[j] = g;
        lo[j] = K;
        vals[j] = vals2[j];
        uint32_t l = kLcpPending;
        if (j > 0) {
            const uint64_t kp = keys2[j - 1];
            const uint32_t Kp = (uint32_t)kp;
            if ((uint32_t)(kp >> 32) == g && Kp != K) {
                const uint32_t ra = (Kp & 0x80000000u) ? ~Kp : Kp, rb = (K & 0x80000000u) ? ~K : K;
                l = ra < rb ? ra : rb;
            }
        }
        lcp_list[j] = l;
    }
}

}  // namespace

// how the tied suffixes are grouped decides which passes can do anything (per_count_large_kernel)
void count_large_groups(SaBuild &b, uint32_t limit, uint32_t *d_cnt, uint32_t out[4]) {
    hipStream_t s = b.stream();
    HIP_CHECK(hipMemsetAsync(d_cnt, 0, 4 * sizeof(uint32_t), s));
    per_count_large_kernel<<<grid_for(b.m, kThreads), kThreads, 0, s>>>(b.slot(), b.grp(), b.m, b.sa, limit, kPerVerifyMax, d_cnt);
    KERNEL_CHECK();
    b.ctx.read_back(d_cnt, out, 4);
}

// ---- periodic runs: groups whose members lie one short period apart are ordered arithmetically ----
// (kernels and the argument above, "Periodic runs".  Tried when a large part of the text is still tied:
// once behind the direct round, and again in the doubling rounds when the depth has reached the
// shortest distance that was too long for it.)  true: the pass finished a good part of what was tied.
bool periodic_pass(SaBuild &b) {
    const bool trace = sa_knobs().trace;
    const PackedText &text = b.text;
    hipStream_t s = b.stream();
    Arena &arena = b.arena();
    const uint32_t n = b.n, m = b.m;
    if (sa_knobs().no_periodic || m == 0 || n >= 0x80000000u || b.wlen < n || b.per_attempts >= 3) return false;
    ProfScope ps(b.ctx.profiler(), "sa_periodic", s);
    if (b.per_attempts == 0 && (b.in_large < m / 8 || b.near_members < m / 32)) {
        // worth its two sorts only where large groups hold a good part of what is tied: copies of long
        // regions tie in groups of a few members (the pair-run pass takes those), runs of a short period
        // in groups as large as the runs are long -- and only where tied suffixes lie close to each other in
        // the text: two dozen copies of a genome tie in groups of two dozen members a genome apart (the
        // first sort of the pass, 28 of 212 ms on 24 genomes of 2^28 bases in all, found that out before)
        b.per_attempts = 3;  // (never again for this text)
        return false;
    }
    ++b.per_attempts;
    uint32_t *PQ = b.tmp_a, *rev = b.tmp_b, *end_of = b.tmp_c, *gq = b.lo, *kraw = b.rank_val;
    uint32_t *d_hint = b.d_total + 3;
    const size_t lmark = arena.mark();
    uint64_t *pk[2] = {arena.alloc<uint64_t>(m), arena.alloc<uint64_t>(m)};
    uint32_t *pv[2] = {arena.alloc<uint32_t>(m), arena.alloc<uint32_t>(m)};
    HIP_CHECK(hipMemsetAsync(gq, 0xff, (size_t)n * sizeof(uint32_t), s));
    HIP_CHECK(hipMemsetAsync(PQ, 0, (size_t)n * sizeof(uint32_t), s));
    HIP_CHECK(hipMemsetAsync(d_hint, 0xff, sizeof(uint32_t), s));
    per_keys_kernel<<<grid_for(m, kThreads), kThreads, 0, s>>>(b.slot(), b.grp(), m, b.sa, pk[0], pv[0]);
    KERNEL_CHECK();
    const int c = radix_sort_pairs(pk, pv, m, b.shifts, b.npasses, arena, s, b.ctx.profiler());
    per_link_kernel<<<(unsigned)div_up(m, kThreads), kThreads, 0, s>>>(pk[c], m, gq);
    KERNEL_CHECK();
    const uint32_t depth = (uint32_t)std::min<uint64_t>(b.h, 0x7ffffffeu);
    // longer periods than the depth are taken if the text confirms them (one segment: see per_verify_kernel)
    const bool verify = text.terms.count == 1 && depth < kPerVerifyMax;
    const uint32_t qmax = verify ? kPerVerifyMax : depth;
    {
        // Large groups are not always periodic runs: two dozen copies of a genome tie in groups of two dozen
        // members that lie a genome apart.  When next to nothing can be taken, the pass stops here, before
        // its scans and its second sort (49 of 300 ms on 24 genomes of 2^28 bases in all).
        HIP_CHECK(hipMemsetAsync(b.d_large, 0, sizeof(uint32_t), s));
        per_candidates_kernel<<<grid_for(m, kThreads), kThreads, 0, s>>>(pk[c], m, gq, qmax, b.d_large);
        KERNEL_CHECK();
        uint32_t cand = 0;
        b.ctx.read_back(b.d_large, &cand, 1);
        if (cand < m / 16) {
            arena.rewind(lmark);
            b.per_attempts = 3;
            if (trace) fprintf(stderr, "[nolzss]   periodic runs (depth %llu): %u of %u tied suffixes in groups that could be runs -- skipped\n",
                               (unsigned long long)b.h, cand, m);
            return false;
        }
    }
    if (verify) {
        const unsigned gv = grid_for(m, kThreads, 256u * 64u);
        dispatch_bits(text.bits, [&](auto B) {
            per_verify_kernel<decltype(B)::value><<<gv, kThreads, 0, s>>>(pk[c], m, gq, depth, n, text.words, text.terms);
        });
        KERNEL_CHECK();
    }
    // (groups the text check has flagged are out; the others pass up to kPerVerifyMax, beyond it up to the depth)
    per_flags_kernel<<<grid_for(m, kThreads), kThreads, 0, s>>>(pk[c], m, gq, qmax, PQ, d_hint);
    KERNEL_CHECK();
    per_breaks_kernel<<<grid_for(n, kThreads, 256u * 64u), kThreads, 0, s>>>(PQ, n, rev);
    KERNEL_CHECK();
    scan_inclusive_max_u32(rev, end_of, n, arena, s);
    per_rho_kernel<<<grid_for(m, kThreads), kThreads, 0, s>>>(pk[c], m, gq, PQ, end_of, b.rank, n, b.Plcp, depth, kraw);
    KERNEL_CHECK();
    per_keys2_kernel<<<grid_for(m, kThreads), kThreads, 0, s>>>(pk[c], m, gq, kraw, pk[c ^ 1], pv[c ^ 1]);
    KERNEL_CHECK();
    uint64_t *pk2[2] = {pk[c ^ 1], pk[c]};
    uint32_t *pv2[2] = {pv[c ^ 1], pv[c]};
    const int c2 = radix_sort_pairs(pk2, pv2, m, b.shifts, b.npasses, arena, s, b.ctx.profiler());
    uint32_t *grp_sorted = b.tmp_a, *lcp_list = b.tmp_b;  // (PQ and rev are done)
    per_view_kernel<<<grid_for(m, kThreads), kThreads, 0, s>>>(pk2[c2], pv2[c2], m, grp_sorted, b.out_lo, b.out_vals, lcp_list);
    KERNEL_CHECK();
    arena.rewind(lmark);
    uint32_t hint = 0;
    b.ctx.read_back(d_hint, &hint, 1);
    b.per_hint = hint == 0xffffffffu ? 0u : hint;
    RegroupIn in;
    in.grp = grp_sorted;
    in.lo = b.out_lo;
    in.vals = b.out_vals;
    in.lcp_list = lcp_list;
    regroup<false>(b, in);
    if (trace) fprintf(stderr, "[nolzss]   periodic runs (depth %llu): %u of %u tied suffixes finished%s\n",
                       (unsigned long long)b.h, m - b.m, m, b.per_hint ? " (a longer period waits for more depth)" : "");
    return b.m < m - m / 8;
}

namespace {

// one sweep over the text: the groups along every run, from the group behind its end
void pair_run_sweep(SaBuild &b) {
    hipStream_t s = b.stream();
    Profiler *prof = b.ctx.profiler();
    const uint32_t n = b.n;
    uint32_t *link = b.tmp_a, *gsz = b.rank_val, *rev = b.tmp_b, *end_of = b.tmp_c, *togo = b.scratch_idx;
    uint32_t *end_place = b.scratch_val, *end_lcp = b.lo;
    uint32_t *end_head = b.out_lo;
    const unsigned g = grid_for(n, kThreads, 256u * 64u);
    {
        ProfScope p1(prof, "runs_link", s);
        group_link_kernel<<<g, kThreads, 0, s>>>(b.rank, b.sa, b.lcp, n, link, gsz);
        KERNEL_CHECK();
    }
    {
        ProfScope p2(prof, "runs_scan", s);
        run_breaks_kernel<<<g, kThreads, 0, s>>>(link, gsz, n, rev);
        KERNEL_CHECK();
        scan_inclusive_max_u32(rev, end_of, n, b.arena(), s);
        group_run_kernel<<<g, kThreads, 0, s>>>(gsz, b.rank, b.sa, end_of, n, togo);
        KERNEL_CHECK();
    }
    {
        ProfScope p3(prof, "runs_end", s);
        group_end_kernel<<<g, kThreads, 0, s>>>(gsz, togo, end_of, b.rank, b.sa, n, b.Plcp, end_place, end_head, end_lcp);
        KERNEL_CHECK();
    }
    {
        ProfScope p4(prof, "runs_members", s);
        group_members_kernel<<<g, kThreads, 0, s>>>(gsz, togo, end_of, n, end_place, end_head, end_lcp, b.rank, b.sa, b.lcp);
        KERNEL_CHECK();
    }
}

}  // namespace

// ---- long exact repeats: small groups along runs of text positions are finished arithmetically ---
// (worth its passes over the text only when a large part of it is still tied; a pass that splits
// groups without finishing them -- three copies, one of which differs behind the run -- is followed by
// another one over the smaller groups)
// (the pass takes groups of up to kRunGroupMax members: where most of what is tied sits in larger groups -- 17
// and more copies of a genome -- its four sweeps over the text finish next to nothing: 120 of 300 ms on 24 genomes)
// (and a group of k copies is finished by about k - 1 passes, each a sweep over the whole text that costs as much as
// two doubling rounds: 168 ms for the four passes of five genomes, 120 ms for one pass of twelve that finished 5 %
// of what was tied, where the doubling rounds from the depth the direct round reached take 85 ms; three genomes:
// 115 ms with two passes, 92 ms with the doubling rounds; two genomes: 72 against 82 ms, two exact copies 79 against
// 279 ms -- the passes run where the tied suffixes sit in pairs: mean group size at most 2.5)
bool pair_run_pass(SaBuild &b) {
    hipStream_t s = b.stream();
    const uint32_t n = b.n;
    ProfScope ps(b.ctx.profiler(), "sa_pair_runs", s);
    pair_run_sweep(b);
    ProfScope p5(b.ctx.profiler(), "runs_compact", s);
    // the active list without the suffixes that are done, with the new group heads of the others
    const uint32_t m = b.m;
    uint32_t *keep = b.tmp_a, *pos = b.tmp_b, *head = b.tmp_c;
    still_tied_kernel<<<grid_for(m, kThreads), kThreads, 0, s>>>(b.slot(), b.grp(), m, b.lcp, n, head, keep);
    KERNEL_CHECK();
    scan_exclusive_add_u32(keep, pos, m, b.d_total, b.arena(), s);
    compact_active_kernel<<<grid_for(m, kThreads), kThreads, 0, s>>>(b.slot(), head, keep, pos, m, b.next_slot(), b.next_grp());
    KERNEL_CHECK();
    uint32_t left = 0;
    b.ctx.read_back(b.d_total, &left, 1);
    if (sa_knobs().trace) fprintf(stderr, "[nolzss]   pair runs: %u of %u tied suffixes finished\n", m - left, m);
    b.m = left;
    b.a_cur ^= 1;
    if (left > 0) {
        b.arena().rewind(b.pyr_mark);
        b.Plcp = build_pyramid(b.lcp, n + 1, false, b.arena(), s);
    }
    return left < m - m / 8;  // (else: no progress)
}

void pair_run_passes(SaBuild &b) {
    const SaKnobs &knobs = sa_knobs();
    const uint32_t n = b.n;
    const bool runs_can_help = knobs.pair_runs_min >= 0 ||
                               (b.large_members <= b.m / 2 && (uint64_t)b.m * 4 <= (uint64_t)b.tied_groups * knobs.runs_avg4);
    for (int pass = 0; b.pair_runs && runs_can_help && pass < 10 && b.m > 0 &&
                       (knobs.pair_runs_min >= 0 ? (long long)b.m >= knobs.pair_runs_min : b.m >= n / 16); ++pass)
        if (!pair_run_pass(b)) break;
}

}  // namespace nolzss
