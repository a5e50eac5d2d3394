// debug_rlz.hip -- test hooks of the relative-LZ index (part of the C ABI layer of libnolzss_hip.so, include/nolzss_hip.h,
// the debug section): nolzss_debug_rlz_seed_chain, the seed-chain stages on a caller's anchors (the kernels:
// rlz_seed_chain.hip; DESIGN.md 5, "Relative-LZ index: colinear seed chains").
#include "rlz_handles.hpp"

using namespace nolzss;
using namespace nolzss::api;

namespace {

// The debug hook: the checks of the caller's anchors, then rlz_seed_chain_run on them.
void debug_seed_chain(const uint32_t *target, const uint32_t *group, const uint32_t *y, const uint32_t *q, const uint32_t *length,
                      size_t n, const nolzss_rlz_chain_params *params, uint64_t B, uint32_t m, int device, uint32_t *f,
                      uint32_t *pred, nolzss_rlz_seed_chains_result *out) {
    if (!out) throw std::invalid_argument("output pointer is null");
    std::memset(out, 0, sizeof *out);
    if (!params || (n && (!target || !group || !y || !q || !length || !f || !pred))) throw std::invalid_argument("null argument");
    if (n >= (size_t(1) << 31)) throw std::invalid_argument("too many anchors");
    if (m == 0 || m > 128 || B > 0xffffffffull) throw std::invalid_argument("1 .. 128 records in a block below 2^32 bases");
    for (size_t i = 0; i < n; ++i) {
        const std::string at = "anchor " + std::to_string(i);
        if (target[i] >= kChainMaxTargets) throw std::invalid_argument(at + ": the target is beyond 2^24");
        if (group[i] >= 2 * m) throw std::invalid_argument(at + ": the group is beyond 2 m");
        if (length[i] == 0) throw std::invalid_argument(at + ": a length of 0");
        if ((uint64_t)q[i] + length[i] >= (1ull << 31)) throw std::invalid_argument(at + ": q + length reaches 2^31");
        if (group[i] >= m && (uint64_t)y[i] + length[i] > 2 * B + 1)
            throw std::invalid_argument(at + ": a reverse-strand anchor in front of the block");
        if (i == 0) continue;
        const size_t j = i - 1;
        const bool same = target[j] == target[i] && group[j] == group[i];
        const uint64_t a = ((uint64_t)target[j] << 40) | ((uint64_t)group[j] << 32) | y[j];
        const uint64_t c = ((uint64_t)target[i] << 40) | ((uint64_t)group[i] << 32) | y[i];
        if (a > c || (a == c && q[j] > q[i])) throw std::invalid_argument(at + ": the anchors do not ascend by (target, group, y, q)");
        if (same && a == c && q[j] == q[i]) throw std::invalid_argument(at + ": (y, q) occurs twice in its group");
    }
    nolzss_rlz_seed_chains_result res;
    std::memset(&res, 0, sizeof res);
    try {
        if (n == 0) {
            res.anchor_offsets = static_cast<uint64_t *>(std::calloc(1, sizeof(uint64_t)));
        } else {
            constexpr size_t kPad = 64;  // entries behind every array, filled with 0xff bytes
            std::vector<uint64_t> keys(n + kPad, ~0ull);
            std::vector<uint32_t> hq(n + kPad, 0xffffffffu), hl(n + kPad, 0xffffffffu);
            for (size_t i = 0; i < n; ++i) {
                keys[i] = ((uint64_t)target[i] << 40) | ((uint64_t)group[i] << 32) | y[i];
                hq[i] = q[i];
                hl[i] = length[i];
            }
            Session ses(device, nullptr);
            Context &ctx = ses.ctx();
            hipStream_t s = ctx.stream;
            ctx.arena.reserve((16 + 152) * (n + kPad) + (size_t(64) << 20));
            ArenaRewind rewind(ctx.arena);
            uint64_t *d_keys = ctx.arena.alloc<uint64_t>(n + kPad);
            uint32_t *d_q = ctx.arena.alloc<uint32_t>(n + kPad), *d_len = ctx.arena.alloc<uint32_t>(n + kPad);
            HIP_CHECK(hipMemcpyAsync(d_keys, keys.data(), (n + kPad) * 8, hipMemcpyHostToDevice, s));
            HIP_CHECK(hipMemcpyAsync(d_q, hq.data(), (n + kPad) * 4, hipMemcpyHostToDevice, s));
            HIP_CHECK(hipMemcpyAsync(d_len, hl.data(), (n + kPad) * 4, hipMemcpyHostToDevice, s));
            HIP_CHECK(hipStreamSynchronize(s));  // (local vectors)
            ChainAnchors a;
            a.keys = d_keys;
            a.q = d_q;
            a.len = d_len;
            a.n = (uint32_t)n;
            const ChainsOut run = rlz_seed_chain_run(ctx, a, chain_rules(*params, m, B));
            HIP_CHECK(hipMemcpyAsync(f, run.f, n * 4, hipMemcpyDeviceToHost, s));
            HIP_CHECK(hipMemcpyAsync(pred, run.pred, n * 4, hipMemcpyDeviceToHost, s));
            deliver_chains(ctx, run, res);
            HIP_CHECK(hipStreamSynchronize(s));
            HIP_CHECK(hipGetLastError());
            ctx.prof.collect();
        }
    } catch (...) {
        nolzss_free_rlz_seed_chains_result(&res);
        throw;
    }
    *out = res;
}

}  // namespace

extern "C" {

int nolzss_debug_rlz_seed_chain(const uint32_t *target, const uint32_t *group, const uint32_t *y, const uint32_t *q,
                                const uint32_t *length, size_t n, const nolzss_rlz_chain_params *params, uint64_t B,
                                uint32_t m, int device, uint32_t *f, uint32_t *pred, nolzss_rlz_seed_chains_result *res) {
    return guarded([&] { debug_seed_chain(target, group, y, q, length, n, params, B, m, device, f, pred, res); });
}

}  // extern "C"
