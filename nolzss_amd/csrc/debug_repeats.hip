// debug_repeats.hip -- test hook for the two arithmetic passes of sa_repeats.hip (pair runs, periodic runs) and the counts
// in front of them: the caller's partial state of a suffix-array construction -- sa, lcp, rank and the active list, as
// they stand behind write_all_ranks -- goes into arena memory, an SaBuild is made of it the way the driver makes one
// (set_up_late_rounds, the driver's own function: work arrays, counts, LCP pyramid, radix shifts) and the chosen pass
// runs on the context's stream: periodic_pass and pair_run_pass themselves, with their gates.  No product path calls
// this (part of the C ABI layer of libnolzss_hip.so, include/nolzss_hip.h).
#include "api_internal.hpp"
#include "sa_internal.hpp"

using namespace nolzss;
using namespace nolzss::api;

extern "C" {

int nolzss_debug_repeat_pass(const uint8_t *text, size_t n, uint32_t *sa, uint32_t *lcp, uint32_t *rank, const uint32_t *slot,
                             const uint32_t *grp, size_t m, uint32_t h, int which, int arg, int device, uint32_t *new_slot,
                             uint32_t *new_grp, uint32_t *new_m, uint32_t *counts, uint32_t *info, uint32_t *periodic) {
    return guarded([&] {
        if (!text || !sa || !lcp || !rank || !new_m || !counts || !periodic || (m && (!slot || !grp || !new_slot || !new_grp)))
            throw std::invalid_argument("null argument");
        // (positions carry a flag in bit 31, sa_repeats.hip: kPerBad)
        if (n == 0 || n >= (size_t(1) << 31)) throw std::invalid_argument("1 .. 2^31 - 1 symbols");
        if (m > n) throw std::invalid_argument("more list entries than suffixes");
        if (which < NOLZSS_REPEAT_PASS_COUNTS || which > NOLZSS_REPEAT_PASS_PAIR_RUNS) throw std::invalid_argument("which: 0 counts, 1 periodic pass, 2 pair-run passes");
        if (which == NOLZSS_REPEAT_PASS_COUNTS && arg != 0) throw std::invalid_argument("the counts take no argument");
        if (which == NOLZSS_REPEAT_PASS_PERIODIC && (arg < 0 || arg > 3)) throw std::invalid_argument("periodic pass: 0 .. 3 attempts on entry");
        if (which == NOLZSS_REPEAT_PASS_PAIR_RUNS && (arg < 1 || arg > 10)) throw std::invalid_argument("pair-run passes: 1 .. 10 of them");
        // the list as the kernels rely on it: ascending slots, every group on consecutive list positions and on the slots
        // from its head slot on, at least two members
        for (size_t a = 0, first = 0; a < m; ++a) {
            const uint32_t g = grp[a], s = slot[a];
            if (g > s || s >= n) throw std::invalid_argument("a list entry with grp <= slot < n violated");
            const bool head = a == 0 || grp[a - 1] != g;
            if (a > 0 && s <= slot[a - 1]) throw std::invalid_argument("the list is not in ascending slot order");
            if (head) first = a;
            if (s != g + (a - first)) throw std::invalid_argument("a group does not hold the slots from its head slot on");
            if ((a + 1 == m || grp[a + 1] != g) && a == first) throw std::invalid_argument("a listed group of one member");
        }
        // sa is a permutation; the groups are what lcp says they are (a decided entry starts one, a pending code goes on
        // with it), the list holds exactly the slots of the groups of more than one, and rank names the head slot + 1
        {
            std::vector<bool> seen(n, false);
            for (size_t s = 0; s < n; ++s) {
                if (sa[s] >= n || seen[sa[s]]) throw std::invalid_argument("sa is not a permutation of the positions");
                seen[sa[s]] = true;
            }
            if (lcp[0] >= kLcpPendingMin) throw std::invalid_argument("lcp[0] is pending");
            size_t a = 0;
            uint32_t head = 0;
            for (size_t s = 0; s < n; ++s) {
                const bool inside = lcp[s] >= kLcpPendingMin;
                if (!inside) head = (uint32_t)s;
                if (rank[sa[s]] != head + 1u) throw std::invalid_argument("rank is not the head slot of the suffix's group + 1");
                const bool tied = inside || (s + 1 < n && lcp[s + 1] >= kLcpPendingMin);
                if (!tied) continue;
                if (a >= m || slot[a] != s) throw std::invalid_argument("a slot inside a group (by lcp) is not listed");
                if (grp[a] != head) throw std::invalid_argument(inside ? "a decided LCP entry is missing at the head of a listed group"
                                                                       : "a boundary inside a listed group holds no pending code");
                ++a;
            }
            if (a != m) throw std::invalid_argument("a listed slot is a group of its own (by lcp)");
        }
        *new_m = 0;
        std::fill(counts, counts + 4, 0u);
        std::fill(periodic, periodic + 3, 0u);
        Session ses(device, nullptr);
        Context &ctx = ses.ctx();
        hipStream_t s = ctx.stream;
        // text and packed text, sa / rank / lcp, the two lists and rank_by_slot, nine work arrays, the pyramid; the
        // periodic pass: two sorts of 12-byte records over the list, the scans, the scatter of the changed ranks
        ctx.arena.reserve(n * 176 + (size_t(64) << 20));
        ArenaRewind rewind(ctx.arena);
        uint8_t *d_text = ctx.arena.alloc<uint8_t>(n);
        upload_bytes(ctx, d_text, text, n);
        const PackedText packed = pack_text(ctx, d_text, n);
        if (info) {
            info[0] = (uint32_t)packed.bits;
            info[1] = packed.terms.count;
            info[2] = packed.segmented;
        }
        uint32_t *d_sa = ctx.arena.alloc<uint32_t>(n), *d_rank = ctx.arena.alloc<uint32_t>(n), *d_lcp = ctx.arena.alloc<uint32_t>(n + 1);
        HIP_CHECK(hipMemcpyAsync(d_sa, sa, n * 4, hipMemcpyHostToDevice, s));
        HIP_CHECK(hipMemcpyAsync(d_rank, rank, n * 4, hipMemcpyHostToDevice, s));
        // (lcp[n]: the driver has arena memory there that nothing has written yet -- it clears the entry when the
        // construction is over -- so the caller's word goes in as it is, and the tests send more than one)
        HIP_CHECK(hipMemcpyAsync(d_lcp, lcp, (n + 1) * 4, hipMemcpyHostToDevice, s));
        SaBuild b{ctx, packed, (uint32_t)n, d_sa, d_rank, d_lcp};
        for (uint32_t **a : {&b.act_slot[0], &b.act_slot[1], &b.act_grp[0], &b.act_grp[1], &b.rank_by_slot}) *a = ctx.arena.alloc<uint32_t>(n);
        b.d_total = ctx.arena.alloc<uint32_t>(4);
        HIP_CHECK(hipMemcpyAsync(b.act_slot[0], slot, m * 4, hipMemcpyHostToDevice, s));
        HIP_CHECK(hipMemcpyAsync(b.act_grp[0], grp, m * 4, hipMemcpyHostToDevice, s));
        b.m = (uint32_t)m;
        b.h = h;
        set_up_late_rounds(b, /*force_pair_runs=*/true);
        if (which == NOLZSS_REPEAT_PASS_PERIODIC) b.per_attempts = arg;
        if (m > 0) {
            count_large_groups(b, kRunGroupMax, b.d_large, counts);
            if (b.in_large != counts[0] || b.large_members != counts[0] + kRunGroupMax * counts[1] || b.tied_groups != counts[2] ||
                b.near_members != counts[3] || !b.pair_runs || b.wlen != n)
                throw std::logic_error("repeat pass: the set-up holds other counts than a second count");
            if (which == NOLZSS_REPEAT_PASS_PERIODIC) {
                periodic[0] = periodic_pass(b) ? 1u : 0u;
            } else if (which == NOLZSS_REPEAT_PASS_PAIR_RUNS) {
                for (int pass = 0; pass < arg && b.m > 0; ++pass) pair_run_pass(b);
            }
            if (b.m > m) throw HipError("repeat pass: more suffixes tied than before");
            HIP_CHECK(hipMemcpyAsync(new_slot, b.slot(), (size_t)b.m * 4, hipMemcpyDeviceToHost, s));
            HIP_CHECK(hipMemcpyAsync(new_grp, b.grp(), (size_t)b.m * 4, hipMemcpyDeviceToHost, s));
        }
        *new_m = b.m;
        periodic[1] = b.per_hint;
        periodic[2] = (uint32_t)b.per_attempts;
        HIP_CHECK(hipMemcpyAsync(sa, d_sa, n * 4, hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipMemcpyAsync(rank, d_rank, n * 4, hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipMemcpyAsync(lcp, d_lcp, (n + 1) * 4, hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipStreamSynchronize(s));
        ctx.prof.collect();
    });
}

}  // extern "C"
