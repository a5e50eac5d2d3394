// Host program for tests/test_rank_blocks_host.py: the interval search over rank blocks (nolzss_amd/csrc/rank_blocks.hpp)
// against the entry-by-entry scans of factor_kernel, on random arrays.  No device, no HIP header.
//
// Arrays: sa = a random permutation of 0 .. n - 1, lcp[0] = lcp[n] = 0 and the entries between drawn so that intervals
// of every width occur (inside one block, over two, over three, wider).  The blocks are built as the candidate kernel
// builds them, padding included.  Every rank is queried with every L from 1 to the largest LCP entry + 1.
#include "rank_blocks.hpp"

#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

using nolzss::RankBlock;

namespace {

struct Case {
    uint32_t n;
    std::vector<uint32_t> sa, lcp;
    std::vector<RankBlock> blocks;
    unsigned long far_calls = 0, range_calls = 0;
};

void build_blocks(Case &c) {
    c.blocks.assign(nolzss::rank_block_count(c.n), RankBlock{});
    for (size_t b = 0; b < c.blocks.size(); ++b)
        for (uint32_t j = 0; j < nolzss::kRankBlock; ++j) {
            const size_t r = b * nolzss::kRankBlock + j;
            c.blocks[b].sa[j] = r < c.n ? c.sa[r] : 0xffffffffu;
            c.blocks[b].lcp[j] = r <= c.n ? c.lcp[r] : 0u;
        }
}

// factor_kernel's loops without the step limit
void plain(const Case &c, uint32_t r, uint32_t L, uint32_t &lo, uint32_t &hi, uint32_t &mn) {
    lo = r;
    hi = r + 1;
    while (c.lcp[lo] >= L) --lo;
    while (c.lcp[hi] >= L) ++hi;
    hi -= 1;
    mn = 0xffffffffu;
    for (uint32_t q = lo; q <= hi; ++q) mn = c.sa[q] < mn ? c.sa[q] : mn;
}

int check(Case &c, const char *what) {
    build_blocks(c);
    uint32_t top = 0;
    for (uint32_t v : c.lcp) top = v > top ? v : top;
    for (uint32_t r = 0; r < c.n; ++r)
        for (uint32_t L = 1; L <= top + 1; ++L) {
            uint32_t elo, ehi, emn;
            plain(c, r, L, elo, ehi, emn);
            const nolzss::RankInterval S = nolzss::rank_block_interval(
                r, L, [&](uint32_t b) { return c.blocks.at(b); },
                [&](uint32_t q, uint32_t x) {
                    ++c.far_calls;
                    while (c.lcp.at(q) >= x) --q;
                    return q;
                },
                [&](uint32_t q, uint32_t x) {
                    ++c.far_calls;
                    while (c.lcp.at(q) >= x) ++q;
                    return q;
                },
                [&](uint32_t a, uint32_t b) {
                    ++c.range_calls;
                    if (a > b || b >= c.n) {
                        fprintf(stderr, "%s: range_min(%u, %u) outside the array (n = %u)\n", what, a, b, c.n);
                        exit(1);
                    }
                    uint32_t m = 0xffffffffu;
                    for (uint32_t q = a; q <= b; ++q) m = c.sa[q] < m ? c.sa[q] : m;
                    return m;
                });
            const uint32_t lo = S.lo, hi = S.hi, mn = S.mn;
            if (lo != elo || hi != ehi || mn != emn) {
                fprintf(stderr, "%s: n = %u r = %u L = %u: blocks (%u, %u, %u), scans (%u, %u, %u)\n", what, c.n, r, L, lo, hi, mn,
                        elo, ehi, emn);
                return 1;
            }
        }
    return 0;
}

Case make(uint32_t n, std::mt19937 &rng, uint32_t max_lcp, double p_low) {
    Case c;
    c.n = n;
    c.sa.resize(n);
    for (uint32_t k = 0; k < n; ++k) c.sa[k] = k;
    for (uint32_t k = n; k > 1; --k) std::swap(c.sa[k - 1], c.sa[rng() % k]);
    c.lcp.assign((size_t)n + 1, 0u);
    std::uniform_real_distribution<double> u(0.0, 1.0);
    for (uint32_t k = 1; k < n; ++k) c.lcp[k] = u(rng) < p_low ? rng() % 2 : 1 + rng() % max_lcp;
    return c;
}

}  // namespace

int main() {
    std::mt19937 rng(0x5EED0003u);
    unsigned long far_calls = 0, range_calls = 0;
    // lengths around the block size and its multiples; low entries rare enough for intervals of 1 to > 48 ranks
    const uint32_t lengths[] = {1, 2, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 65, 255, 256, 257, 1000};
    const double p_lows[] = {0.5, 0.1, 0.02};
    for (uint32_t n : lengths)
        for (double p : p_lows)
            for (int rep = 0; rep < 3; ++rep) {
                Case c = make(n, rng, 6, p);
                if (check(c, "random")) return 1;
                far_calls += c.far_calls;
                range_calls += c.range_calls;
            }
    // one run: every entry between the ends is large (the whole array is one interval for small L)
    for (uint32_t n : {16u, 48u, 300u}) {
        Case c = make(n, rng, 1, 0.0);
        for (uint32_t k = 1; k < n; ++k) c.lcp[k] = n - k;
        if (check(c, "run")) return 1;
        far_calls += c.far_calls;
        range_calls += c.range_calls;
    }
    if (far_calls == 0 || range_calls == 0) {
        fprintf(stderr, "the cases never left three blocks (%lu far searches, %lu range minima)\n", far_calls, range_calls);
        return 1;
    }
    printf("ok: %lu far searches, %lu range minima\n", far_calls, range_calls);
    return 0;
}
