// debug_rlz.hip -- test hooks of the relative-LZ index (part of the C ABI layer of libnolzss_hip.so, include/nolzss_hip.h,
// the debug section): nolzss_debug_rlz_seed_chain, the seed-chain stages on a caller's anchors (the kernels:
// rlz_seed_chain.hip; DESIGN.md 5, "Relative-LZ index: colinear seed chains"), nolzss_debug_rlz_align_jobs, the
// alignment stages on a caller's jobs (the kernels: rlz_align.hip; DESIGN.md 5, "Relative-LZ index: base-level
// alignments"), and nolzss_debug_rlz_pileup, the pileup stages on a caller's alignments (the kernels: rlz_pileup.hip;
// DESIGN.md 5, "Relative-LZ index: pileup").
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

// text s, upper-cased, as a batch of one target: uploaded and packed as production packs a batch
PackedText pack_debug_text(Context &ctx, const char *text, size_t len, const char *what) {
    HostBytes bytes(len + 1);
    for (size_t i = 0; i < len; ++i) bytes[i] = (uint8_t)text[i] & 0xdfu;  // (the caller has checked the bases)
    bytes[len] = kSeparator;
    uint8_t *d_text = ctx.arena.alloc<uint8_t>(len + 1);
    upload_bytes(ctx, d_text, bytes.data(), len + 1);
    HIP_CHECK(hipStreamSynchronize(ctx.stream));  // (bytes is a local)
    PackedText t;
    if (!pack_independent_text(ctx, d_text, len + 1, std::vector<uint32_t>{(uint32_t)len}, t))
        throw std::runtime_error(std::string(what) + ": bytes that are neither bases nor the separator");
    t.n = (uint32_t)len;  // (the jobs end in front of the separator)
    return t;
}

// The debug hook: the checks of the caller's jobs, then the production stages from the sizes to the traceback.
void debug_align_jobs(const char *query, size_t query_len, const char *reference, size_t reference_len, const uint32_t *kind,
                      const uint32_t *q0, const uint32_t *nq, const uint32_t *y0, const uint32_t *ny, size_t n, uint32_t band,
                      int device, uint32_t *cost, uint32_t *end_col, uint64_t *col_offsets, uint8_t **cols) {
    if (!cols || !col_offsets) throw std::invalid_argument("output pointer is null");
    *cols = nullptr;
    col_offsets[0] = 0;
    if ((query_len && !query) || (reference_len && !reference)) throw std::invalid_argument("null argument");
    if (n && (!kind || !q0 || !nq || !y0 || !ny || !cost || !end_col)) throw std::invalid_argument("null argument");
    if (n >= (size_t(1) << 24)) throw std::invalid_argument("too many jobs");
    if (query_len >= kAlignMaxTarget || reference_len >= kAlignMaxTarget) throw std::invalid_argument("a text of 2^28 bases or more");
    if (2 * (uint64_t)band + 1 > kAlignLanes) throw std::invalid_argument("2 band + 1 is more than 64 diagonals");
    for (size_t i = 0; i < query_len + reference_len; ++i) {
        const uint8_t c = (uint8_t)(i < query_len ? query[i] : reference[i - query_len]) & 0xdfu;
        if (c != 'A' && c != 'C' && c != 'G' && c != 'T')
            throw std::invalid_argument(i < query_len ? "query: an invalid base at " + std::to_string(i)
                                                      : "reference: an invalid base at " + std::to_string(i - query_len));
    }
    constexpr size_t kPad = 64;  // entries behind the job array, filled with 0xff bytes
    std::vector<AlignJob> jobs(n + kPad);
    std::memset(jobs.data() + n, 0xff, sizeof(AlignJob) * kPad);
    uint64_t rows = 0, slots = 0;
    for (size_t i = 0; i < n; ++i) {
        const std::string at = "job " + std::to_string(i);
        if (kind[i] > kAlignLeft) throw std::invalid_argument(at + ": a kind above 2");
        const uint64_t q = q0[i], y = y0[i], a = nq[i], c = ny[i];
        const bool inside = kind[i] == kAlignLeft ? (q <= query_len && a <= q && y <= reference_len && c <= y)
                                                  : (q <= query_len && a <= query_len - q && y <= reference_len && c <= reference_len - y);
        if (!inside) throw std::invalid_argument(at + ": leaves a text");
        if (kind[i] == kAlignGap) {
            const uint64_t delta = a > c ? a - c : c - a;
            if (delta + 2 * (uint64_t)band + 1 > kAlignLanes) throw std::invalid_argument(at + ": more than 64 diagonals");
            jobs[i] = align_gap_job(q0[i], nq[i], y0[i], ny[i], band);
        } else {
            jobs[i] = align_flank_job(kind[i], q0[i], nq[i], y0[i], ny[i], band, ~0ull);
        }
        rows += jobs[i].dp ? jobs[i].nq : 0;
        slots += (uint64_t)jobs[i].nq + jobs[i].ny + 1;
    }
    if (rows > 0xffffffffull || slots > 0xffffffffull) throw std::invalid_argument("DP rows or column slots beyond 2^32 - 1");
    if (n == 0) return;
    Session ses(device, nullptr);
    Context &ctx = ses.ctx();
    hipStream_t s = ctx.stream;
    ctx.arena.reserve(2 * (query_len + reference_len) + (48 + 12 + 20) * (n + kPad) + 16 * (size_t)rows + (size_t)slots + (size_t(64) << 20));
    ArenaRewind rewind(ctx.arena);
    const PackedText qt = pack_debug_text(ctx, query, query_len, "query");
    const PackedText xt = pack_debug_text(ctx, reference, reference_len, "reference");
    AlignJob *d_jobs = ctx.arena.alloc<AlignJob>(n + kPad);
    HIP_CHECK(hipMemcpyAsync(d_jobs, jobs.data(), sizeof(AlignJob) * (n + kPad), hipMemcpyHostToDevice, s));
    HIP_CHECK(hipStreamSynchronize(s));  // (a local vector)
    AlignJobs a;
    a.J = (uint32_t)n;
    a.jobs = d_jobs;
    rlz_align_sizes(ctx, a);
    if (a.total_rows != rows || a.total_slots != slots) throw HipError("rlz align: the sizes of the jobs differ from the host's");
    rlz_align_layout(ctx, a);
    rlz_align_dp(ctx, a, qt, xt);
    rlz_align_traceback(ctx, a);
    std::vector<uint32_t> col_off(n), ncols(n);
    std::vector<uint8_t> codes((size_t)slots);
    HIP_CHECK(hipMemcpyAsync(cost, a.cost, n * 4, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipMemcpyAsync(end_col, a.endj, n * 4, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipMemcpyAsync(col_off.data(), a.col_off, n * 4, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipMemcpyAsync(ncols.data(), a.ncols, n * 4, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipMemcpyAsync(codes.data(), a.codes, (size_t)slots, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    HIP_CHECK(hipGetLastError());
    ctx.prof.collect();
    // the used slots of every job, in ascending q: the first ncols of a left flank, the last ncols of the others
    uint64_t total = 0;
    for (size_t i = 0; i < n; ++i) {
        const uint64_t room = (uint64_t)jobs[i].nq + jobs[i].ny;
        if (ncols[i] > room || (uint64_t)col_off[i] + room + 1 > slots) throw HipError("rlz align: a job's columns leave its slots");
        total += ncols[i];
        col_offsets[i + 1] = total;
    }
    if (total == 0) return;
    uint8_t *flat = static_cast<uint8_t *>(std::malloc(total));
    if (!flat) throw std::bad_alloc();
    for (size_t i = 0; i < n; ++i) {
        const size_t room = (size_t)jobs[i].nq + jobs[i].ny;
        const size_t first = kind[i] == kAlignLeft ? 0 : room - ncols[i];
        std::memcpy(flat + col_offsets[i], codes.data() + col_off[i] + first, ncols[i]);
    }
    *cols = flat;
}

// The debug hook: the host's checks of the caller's alignments, then the production accumulate and read-out of the
// pileup on them, with counters taken from the arena.
void debug_pileup(const char *block, size_t B, const char *const *targets, const size_t *target_lens, size_t k,
                  const nolzss_rlz_alignment *alignments, const uint64_t *op_offsets, size_t C, const uint32_t *ops, size_t N,
                  bool primary_only, int device, uint32_t *counts, uint32_t flags = 0, const ConsensusRule *rule = nullptr,
                  nolzss_rlz_insertions_result *ins = nullptr, nolzss_rlz_consensus_result *cons = nullptr) {
    if ((B && (!block || !counts)) || (k && (!targets || !target_lens)) || !op_offsets || (C && !alignments) || (N && !ops))
        throw std::invalid_argument("null argument");
    if (B >= kAlignMaxTarget || C >= (size_t(1) << 24) || N >= kAlignMaxTarget) throw std::invalid_argument("a block, alignments or ops beyond 2^28");
    Batch b;
    size_t bases = 0;
    for (size_t j = 0; j < k; ++j) {
        if (target_lens[j] && !targets[j]) throw std::invalid_argument("null argument");
        if (target_lens[j] >= kAlignMaxTarget || bases + target_lens[j] + k >= kAlignMaxTarget)
            throw std::invalid_argument("a batch of 2^28 positions or more");
        const size_t bad = first_invalid_nucleotide(targets[j], target_lens[j]);
        if (bad < target_lens[j]) throw std::invalid_argument("target " + std::to_string(j) + ": an invalid base at " + std::to_string(bad));
        bases += target_lens[j];
    }
    // the block: bases upper-cased, every other byte a separator; one more separator behind it, as a batch ends
    HostBytes xbytes(B + 1);
    std::vector<uint32_t> xseps;
    for (size_t i = 0; i < B; ++i) {
        const uint8_t c = (uint8_t)block[i] & 0xdfu;
        const bool base = c == 'A' || c == 'C' || c == 'G' || c == 'T';
        xbytes[i] = base ? c : kSeparator;
        if (!base) xseps.push_back((uint32_t)i);
    }
    xbytes[B] = kSeparator;
    xseps.push_back((uint32_t)B);
    if (op_offsets[0] != 0 || op_offsets[C] != N) throw std::invalid_argument("op_offsets do not run from 0 to num_ops");
    for (size_t c = 0; c < C; ++c) {
        const std::string at = "alignment " + std::to_string(c);
        const nolzss_rlz_alignment &a = alignments[c];
        if (op_offsets[c] >= op_offsets[c + 1] || op_offsets[c + 1] > N) throw std::invalid_argument(at + ": no ops, or offsets that do not ascend");
        if (a.target >= k) throw std::invalid_argument(at + ": the target is beyond the batch");
        if (a.t_start > a.t_end || a.t_end > target_lens[a.target]) throw std::invalid_argument(at + ": leaves its target");
        if (a.r_start >= a.r_end || a.r_end > B) throw std::invalid_argument(at + ": leaves the block, or covers no base of it");
        const auto sep = std::lower_bound(xseps.begin(), xseps.end(), (uint32_t)a.r_start);
        if (*sep < a.r_end) throw std::invalid_argument(at + ": covers a separator");
        uint64_t t = 0, r = 0;
        for (uint64_t i = op_offsets[c]; i < op_offsets[c + 1]; ++i) {
            const uint32_t code = ops[i] & 0xfu, len = ops[i] >> 4;
            if (len == 0 || (code != kAlignI && code != kAlignD && code != kAlignEq && code != kAlignX))
                throw std::invalid_argument(at + ": an op of length 0 or of an unknown code");
            t += code == kAlignD ? 0 : len;
            r += code == kAlignI ? 0 : len;
        }
        if (t != a.t_end - a.t_start || r != a.r_end - a.r_start)
            throw std::invalid_argument(at + ": the ops do not consume exactly [t_start, t_end) and [r_start, r_end)");
    }
    if (B) std::memset(counts, 0, sizeof(uint32_t) * kPileupChannels * B);
    if (B == 0 || (C == 0 && !rule)) return;
    b.tcat.resize(bases + k);
    b.separators.resize(k);
    b.offsets.resize(k);
    size_t at = 0;
    for (size_t j = 0; j < k; ++j) {
        b.offsets[j] = at;
        copy_upper(b.tcat.data() + at, targets[j], target_lens[j]);
        at += target_lens[j];
        b.separators[j] = (uint32_t)at;
        b.tcat[at++] = kSeparator;
    }
    constexpr size_t kPad = 64;  // entries behind the record and op arrays, filled with 0xff bytes
    std::vector<AlignRec> recs(C + kPad);
    std::memcpy(recs.data(), alignments, sizeof(AlignRec) * C);
    std::memset(recs.data() + C, 0xff, sizeof(AlignRec) * kPad);
    std::vector<uint32_t> hops(N + kPad, 0xffffffffu);
    if (N) std::memcpy(hops.data(), ops, sizeof(uint32_t) * N);
    const size_t foot = rlz_pileup_footprint((uint32_t)B);
    DeviceRestore restore;
    Session ses(device, nullptr);
    Context &ctx = ses.ctx();
    hipStream_t s = ctx.stream;
    ctx.arena.reserve(foot + 3 * (B + 1 + b.tcat.size()) + sizeof(AlignRec) * (C + kPad) + 8 * (C + 1) + 24 * (N + kPad) +
                      sizeof(uint32_t) * kPileupChannels * B + (size_t(64) << 20) +
                      (rule ? (sizeof(PileupEvent) + kAllelesArenaPerEvent + kInsertionsArenaPerAllele + sizeof(PileupInsertionRec)) * (N + 1) +
                                  (kConsensusArenaPerBase + 8 * (1 + (size_t)NOLZSS_RLZ_PILEUP_INS_BASES)) * (B + 1) + 8 * (xseps.size() + 1)
                            : 0));
    ArenaRewind rewind(ctx.arena);
    uint8_t *d_block = ctx.arena.alloc<uint8_t>(B + 1);
    upload_bytes(ctx, d_block, xbytes.data(), B + 1);
    HIP_CHECK(hipStreamSynchronize(s));  // (xbytes is a local)
    PackedText xt;
    if (!pack_independent_text(ctx, d_block, B + 1, xseps, xt)) throw std::runtime_error("block: the separators were miscounted");
    PackedText qt;
    upload_and_pack(ctx, b, qt);
    AlignRec *d_recs = ctx.arena.alloc<AlignRec>(C + kPad);
    uint64_t *d_off = ctx.arena.alloc<uint64_t>(C + 1);
    uint32_t *d_ops = ctx.arena.alloc<uint32_t>(N + kPad);
    void *d_counters = ctx.arena.alloc<uint8_t>(foot);
    uint32_t *d_out = ctx.arena.alloc<uint32_t>(kPileupChannels * B);
    unsigned long long *d_stats = ctx.arena.alloc<unsigned long long>(kPileupStats);
    PileupLog log;  // without a rule: no room, every event is dropped at the clamp
    log.flags = flags;
    if (rule) {
        log.events = ctx.arena.alloc<PileupEvent>(N + 1);  // an alignment's I ops are among its ops
        log.capacity = N;
    }
    HIP_CHECK(hipMemcpyAsync(d_recs, recs.data(), sizeof(AlignRec) * (C + kPad), hipMemcpyHostToDevice, s));
    HIP_CHECK(hipMemcpyAsync(d_off, op_offsets, 8 * (C + 1), hipMemcpyHostToDevice, s));
    HIP_CHECK(hipMemcpyAsync(d_ops, hops.data(), 4 * (N + kPad), hipMemcpyHostToDevice, s));
    HIP_CHECK(hipMemsetAsync(d_counters, 0, foot, s));
    HIP_CHECK(hipStreamSynchronize(s));  // (local vectors)
    const PileupView view = rlz_pileup_view(d_counters, (uint32_t)B);
    AlignOut a;
    a.num_alignments = (uint32_t)C;
    a.num_ops = (uint32_t)N;
    a.recs = d_recs;
    a.op_offsets = d_off;
    a.ops = d_ops;
    rlz_pileup_accumulate(ctx, view, a, qt, xt, primary_only, log, d_stats);
    rlz_pileup_resolve(ctx, view);
    rlz_pileup_compose(ctx, view, xt, 0, (uint32_t)B, d_out);
    HIP_CHECK(hipMemcpyAsync(counts, d_out, sizeof(uint32_t) * kPileupChannels * B, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    if (rule) {  // the allele table in full (count >= 1, fraction 0 / 1), then the consensus with its map
        unsigned long long stats[kPileupStats];
        download_bytes(ctx, stats, d_stats, sizeof stats);
        const uint32_t E = (uint32_t)(stats[3] < N ? stats[3] : N);
        uint32_t G = 0;
        const PileupAllele *d_alleles = rlz_pileup_alleles(ctx, log.events, E, &G);
        deliver_insertions(ctx, view, xt, d_alleles, G, PileupRule(), *ins);
        deliver_consensus(ctx, view, xt, (uint32_t)xseps.size(), d_alleles, G, *rule, true, *cons);
    }
    HIP_CHECK(hipGetLastError());
    ctx.prof.collect();
}

}  // namespace

extern "C" {

int nolzss_debug_rlz_pileup(const char *block, size_t B, const char *const *targets, const size_t *target_lens, size_t k,
                            const nolzss_rlz_alignment *alignments, const uint64_t *op_offsets, size_t num_alignments,
                            const uint32_t *ops, size_t num_ops, int primary_only, int device, uint32_t *counts) {
    return guarded([&] {
        debug_pileup(block, B, targets, target_lens, k, alignments, op_offsets, num_alignments, ops, num_ops, primary_only != 0,
                     device, counts);
    });
}

int nolzss_debug_rlz_pileup_consensus(const char *block, size_t B, const char *const *targets, const size_t *target_lens, size_t k,
                                      const nolzss_rlz_alignment *alignments, const uint64_t *op_offsets, size_t num_alignments,
                                      const uint32_t *ops, size_t num_ops, int primary_only, uint32_t flags,
                                      const nolzss_rlz_consensus_params *params, int device, uint32_t *counts,
                                      nolzss_rlz_insertions_result *insertions, nolzss_rlz_consensus_result *consensus) {
    return guarded([&] {
        if (!insertions || !consensus) throw std::invalid_argument("output pointer is null");
        std::memset(insertions, 0, sizeof *insertions);
        std::memset(consensus, 0, sizeof *consensus);
        if (flags & ~NOLZSS_RLZ_PILEUP_NORMALIZE) throw std::invalid_argument("rlz pileup: unknown flag bits");
        const ConsensusRule rule = check_consensus_params(params);
        try {
            debug_pileup(block, B, targets, target_lens, k, alignments, op_offsets, num_alignments, ops, num_ops, primary_only != 0,
                         device, counts, flags, &rule, insertions, consensus);
        } catch (...) {
            nolzss_free_rlz_insertions_result(insertions);
            nolzss_free_rlz_consensus_result(consensus);
            throw;
        }
    });
}

int nolzss_debug_rlz_align_jobs(const char *query, size_t query_len, const char *reference, size_t reference_len,
                                const uint32_t *kind, const uint32_t *q0, const uint32_t *nq, const uint32_t *y0,
                                const uint32_t *ny, size_t n, uint32_t band, int device, uint32_t *cost, uint32_t *end_col,
                                uint64_t *col_offsets, uint8_t **cols) {
    return guarded([&] {
        debug_align_jobs(query, query_len, reference, reference_len, kind, q0, nq, y0, ny, n, band, device, cost, end_col,
                         col_offsets, cols);
    });
}

int nolzss_debug_rlz_seed_chain(const uint32_t *target, const uint32_t *group, const uint32_t *y, const uint32_t *q,
                                const uint32_t *length, size_t n, const nolzss_rlz_chain_params *params, uint64_t B,
                                uint32_t m, int device, uint32_t *f, uint32_t *pred, nolzss_rlz_seed_chains_result *res) {
    return guarded([&] { debug_seed_chain(target, group, y, q, length, n, params, B, m, device, f, pred, res); });
}

}  // extern "C"
