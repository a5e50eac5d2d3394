// rlz_index_seeds_api.hip -- the seed queries of the relative-LZ index handle (part of the C ABI layer of
// libnolzss_hip.so, include/nolzss_hip.h; the handle and its match: rlz_index_api.hip).  nolzss_rlz_index_seeds: the
// maximal exact matches of a target batch and their occurrences (the kernels: rlz_seeds.hip; DESIGN.md 5, "Relative-LZ
// index: maximal match seeds"); nolzss_rlz_index_seed_chains: the seeds of every target chained into placements on the
// device (the kernels: rlz_seed_chain.hip; DESIGN.md 5, "Relative-LZ index: colinear seed chains");
// nolzss_rlz_index_align: every such chain aligned base by base on the device (the kernels: rlz_align.hip; DESIGN.md 5,
// "Relative-LZ index: base-level alignments").
#include "rlz_handles.hpp"

using namespace nolzss;
using namespace nolzss::api;

namespace {

// device memory of a seed query over a batch of n positions and k targets: per position the byte, the packed word
// (1/4), len, rank, flag and slot (4 each), and -- every position can be a seed (a run of one base against a record of
// one base), so the seeds' arrays are reserved with the batch and their number never moves the arena -- the list,
// first, rep and off (4 each): 34; the terminator table; the seed records of a download chunk.  Per hit: as a locate.
size_t seed_batch_bytes(size_t n, size_t k, size_t chunk) {
    return 34 * n + 16 * k + sizeof(SeedRec) * chunk + (size_t(4) << 20);
}

// device memory per hit of a seed-chain query, on top of the 25 of the expanded and sorted hits: the anchors in group
// order (two key and two value arrays of the second sort, q and L by slot and by anchor: 40, the histograms 1) and what
// rlz_seed_chain_run states (152); every group and every chain anchor is at most one per hit
constexpr size_t kChainBytesPerHit = 40 + 1 + 152;

// device memory of the align stages, on top of a seed-chain query.  Per hit -- a chain has at least one anchor and an
// anchor is a hit, so the jobs, one per anchor and one more per chain, are at most two per hit --: the jobs with their
// sizes, offsets and results (48 + 12 + 20 each), L' per anchor (4) and the record and op offset of a chain (88): at most 264.
// Per DP row the two direction words: 16.  Per column slot the code byte, flag, weight and their scans (17) and, an op
// being at most one per slot, its start, code and word (12), rounded up for the scans' tile sums: 32.
constexpr size_t kAlignBytesPerHit = 264, kAlignBytesPerRow = 16, kAlignBytesPerSlot = 32;

static_assert(sizeof(nolzss_rlz_seed) == sizeof(SeedRec) && sizeof(SeedRec) == 32, "the kernels write nolzss_rlz_seed");
static_assert(sizeof(nolzss_rlz_hit) == sizeof(LocateHit) && sizeof(LocateHit) == 16, "the kernels write nolzss_rlz_hit");
static_assert(sizeof(nolzss_rlz_chain) == sizeof(ChainRec) && sizeof(ChainRec) == 64, "the kernels write nolzss_rlz_chain");
static_assert(sizeof(nolzss_rlz_chain_anchor) == sizeof(ChainAnchorRec) && sizeof(ChainAnchorRec) == 24,
              "the kernels write nolzss_rlz_chain_anchor");
static_assert(NOLZSS_RLZ_CHAIN_LOOKBACK == kChainLookback, "the look-back is a constant of the ABI");
static_assert(sizeof(nolzss_rlz_alignment) == sizeof(AlignRec) && sizeof(AlignRec) == 80, "the kernels write nolzss_rlz_alignment");
static_assert(NOLZSS_RLZ_ALIGN_LANES == kAlignLanes, "the diagonals of a job are a constant of the ABI");
static_assert(sizeof(AlignJob) == 48, "the arena accounting counts 48 bytes per job");

// min_length as the kernels take it: 0 means 1, anything beyond 32 bits no seed at all
uint32_t seed_min_len(uint64_t min_length) {
    return min_length >= 0xffffffffull ? 0xffffffffu : (uint32_t)(min_length ? min_length : 1);
}

// The front end of every seed query: the batch up, packed and searched as a match does, the seeds flagged and listed
// -- their number S comes down as one word -- and, with_intervals, the interval of every seed looked up with no record
// written (the seeds query looks them up chunk by chunk with its records instead).
struct SeedFront {
    Searched m;
    uint32_t *d_seeds = nullptr, *d_first = nullptr, *d_rep = nullptr;
    uint32_t S = 0, cap, min_len;
    SeedFront(uint64_t min_length, uint64_t max_hits) : cap(hit_cap(max_hits)), min_len(seed_min_len(min_length)) {}
    // the sort key of a hit holds its seed in the 31 bits above (position, strand)
    bool too_many() const { return S > 0x7fffffffu; }
    void refuse_too_many() const {
        if (too_many())
            throw std::invalid_argument("rlz index: a batch may report at most 2^31 - 1 seeds, this one has " + std::to_string(S) +
                                        ": raise min_length or send fewer targets");
    }
    void intervals(Context &ctx, const nolzss_rlz_index &h, size_t first, size_t count, SeedRec *d_recs) {
        rlz_index_seed_intervals(ctx, h.view, m.batch, d_seeds, (uint32_t)first, (uint32_t)count, cap, m.d_len, m.d_rank, d_first,
                                 d_rep, d_recs);
    }
    void run(Context &ctx, const nolzss_rlz_index &h, const Batch &b, bool with_intervals) {
        const size_t n = b.tcat.size();
        m = search_batch(ctx, h, b);
        uint32_t *d_flag = ctx.arena.alloc<uint32_t>(n), *d_slot = ctx.arena.alloc<uint32_t>(n);
        d_seeds = ctx.arena.alloc<uint32_t>(n);
        uint32_t *d_total = ctx.arena.alloc<uint32_t>(1);
        rlz_index_seed_list(ctx, m.d_len, (uint32_t)n, min_len, d_flag, d_slot, d_seeds, d_total);
        download_bytes(ctx, &S, d_total, sizeof(uint32_t));
        if (S > n) throw HipError("rlz index: more seeds than batch positions");
        d_first = ctx.arena.alloc<uint32_t>(S ? S : 1);
        d_rep = ctx.arena.alloc<uint32_t>(S ? S : 1);
        if (with_intervals && !too_many()) intervals(ctx, h, 0, S, nullptr);
    }
    // ... again, in an arena that regrow_arena has emptied
    void rerun(Context &ctx, const nolzss_rlz_index &h, const Batch &b, bool with_intervals) {
        const uint32_t before = S;
        run(ctx, h, b, with_intervals);
        if (S != before) throw HipError("rlz index: the seeds of a batch changed between two searches");
    }
    // the hits to expand, summed in 64 bits on the device: one word comes down
    uint64_t hit_total(Context &ctx) {
        uint64_t total = 0;
        if (S) {
            uint64_t *d_sum = ctx.arena.alloc<uint64_t>(1);
            rlz_index_rep_total(ctx, d_rep, S, d_sum);
            download_bytes(ctx, &total, d_sum, sizeof(uint64_t));
        }
        return total;
    }
    LocateSorted hits(Context &ctx, const nolzss_rlz_index &h, size_t n, size_t T) {
        return rlz_index_seed_hits(ctx, h.view, (uint32_t)h.m, (uint32_t)n, d_seeds, m.d_len, S, d_rep, d_first, (uint32_t)T);
    }
};

// What a seed query answers when its hits do not fit the pipeline; empty when they do.
std::string hits_refusal(uint64_t total, uint64_t max_hits, uint64_t min_length) {
    if (total <= kMaxText) return std::string();
    return "rlz index: seeds would report " + std::to_string(total) + " hits, more than the " + std::to_string(kMaxText) +
           " the 32-bit device pipeline takes: lower max_hits (it is " + std::to_string(max_hits) +
           "; 0 means no cap), raise min_length (it is " + std::to_string(min_length) + ") or send fewer targets";
}

// The shell of a seed query behind its checks.  No target, or none with a base: one zeroed word for `offsets`, and the
// device is not touched.  Otherwise `query` in a session under `scope`.  `release` frees the result on any throw.
void run_seed_query(const nolzss_rlz_index &h, const Batch &b, size_t k, const char *scope, uint64_t *&offsets,
                    const std::function<void()> &release, const std::function<void(Context &)> &query) {
    try {
        if (b.tcat.size() == k)
            offsets = calloc_array<uint64_t>(1);
        else
            with_index_session(h.device, scope, query);
    } catch (...) {
        release();
        throw;
    }
}

// ---- maximal match seeds -------------------------------------------------------------------------------------------
// One batch of k >= 1 targets with at least one base against the handle, inside a session.  res is filled as the
// results arrive: the seed records and hit_offsets once the counts are known, the hits last.  Returns the refusal when
// the hit total is beyond the pipeline: res then holds the seeds, their counts and the offsets.
std::string query_seeds(Context &ctx, const nolzss_rlz_index &h, const Batch &b, size_t k, uint64_t min_length, uint64_t max_hits,
                        nolzss_rlz_seeds_result &res) {
    const size_t n = b.tcat.size();
    const size_t chunk_max = chunk_knob("NOLZSS_RLZ_LOCATE_CHUNK");
    const size_t seed_chunk = n < chunk_max ? n : chunk_max;
    SeedFront front(min_length, max_hits);
    reserve_arena_for(ctx, 0, seed_batch_bytes(n, k, seed_chunk));
    front.run(ctx, h, b, false);
    const uint32_t S = front.S;
    res.hit_offsets = calloc_array<uint64_t>((size_t)S + 1);
    if (S == 0) return std::string();
    front.refuse_too_many();
    res.seeds = static_cast<nolzss_rlz_seed *>(alloc_factor_block(sizeof(nolzss_rlz_seed) * S));
    if (!res.seeds) throw std::bad_alloc();
    {
        const size_t chunk = S < chunk_max ? S : chunk_max;
        SeedRec *d_recs = ctx.arena.alloc<SeedRec>(chunk);
        download_produced(ctx, "seeds_d2h", res.seeds, d_recs, S, sizeof(SeedRec), chunk,
                          [&](size_t c0, size_t c) { front.intervals(ctx, h, c0, c, d_recs); });
    }
    res.num_seeds = S;
    uint64_t total = 0;  // the hits to report, summed in 64 bits
    for (size_t j = 0; j < S; ++j) {
        res.hit_offsets[j] = total;
        if (res.seeds[j].count <= front.cap) total += res.seeds[j].count;
    }
    res.hit_offsets[S] = total;
    const std::string refusal = hits_refusal(total, max_hits, min_length);
    if (total == 0 || !refusal.empty()) return refusal;
    const size_t T = (size_t)total, chunk = T < chunk_max ? T : chunk_max;
    // the arena for the hits (regrow_arena): in a slab that was replaced the batch is searched again, its seeds listed
    // and their intervals looked up -- the records have come down and are not written a second time
    if (regrow_arena(ctx, seed_batch_bytes(n, k, seed_chunk) + kLocateBytesPerHit * T + sizeof(LocateHit) * chunk))
        front.rerun(ctx, h, b, true);
    const LocateSorted sorted = front.hits(ctx, h, n, T);
    res.hits = static_cast<nolzss_rlz_hit *>(alloc_factor_block(sizeof(nolzss_rlz_hit) * T));
    if (!res.hits) throw std::bad_alloc();
    LocateHit *d_recs = ctx.arena.alloc<LocateHit>(chunk);
    download_produced(ctx, "hits_d2h", res.hits, d_recs, T, sizeof(LocateHit), chunk,
                      [&](size_t c0, size_t c) { rlz_index_hit_records(ctx, sorted, c0, (uint32_t)c, d_recs); });
    res.num_hits = T;
    return std::string();
}

void index_seeds(const nolzss_rlz_index *h, const char *const *targets, const size_t *target_lens, size_t k,
                 uint64_t min_length, uint64_t max_hits, nolzss_rlz_seeds_result *out) {
    if (!out) throw std::invalid_argument("output pointer is null");
    std::memset(out, 0, sizeof *out);
    if (!h) throw std::invalid_argument("handle is null");
    Batch b;
    prepare_batch(*h, targets, target_lens, k, b);
    nolzss_rlz_seeds_result res;
    std::memset(&res, 0, sizeof res);
    std::string refusal;
    run_seed_query(*h, b, k, "rlz_index_seeds", res.hit_offsets, [&] { nolzss_free_rlz_seeds_result(&res); },
                   [&](Context &ctx) { refusal = query_seeds(ctx, *h, b, k, min_length, max_hits, res); });
    *out = res;  // ownership moves to the caller: the seeds, their counts and the offsets also with the refusal
    if (!refusal.empty()) throw std::invalid_argument(refusal);
}

// ---- colinear seed chains ------------------------------------------------------------------------------------------
// One batch of k >= 1 targets with at least one base against the handle, inside a session: the path of query_seeds up to
// the sorted hits, which stay on the device, then the chain stages.  Returns the refusal when the hit total is beyond
// the pipeline: the caller then hands back an empty result.
std::string query_seed_chains(Context &ctx, const nolzss_rlz_index &h, const Batch &b, size_t k, const nolzss_rlz_chain_params &p,
                              nolzss_rlz_seed_chains_result &res) {
    const size_t n = b.tcat.size();
    SeedFront front(p.min_length, p.max_hits);
    reserve_arena_for(ctx, 0, seed_batch_bytes(n, k, 0));
    front.run(ctx, h, b, true);
    front.refuse_too_many();
    res.num_seeds = front.S;
    const uint64_t total = front.hit_total(ctx);
    const std::string refusal = hits_refusal(total, p.max_hits, p.min_length);
    if (!refusal.empty()) return refusal;
    if (total == 0) {
        res.anchor_offsets = calloc_array<uint64_t>(1);
        return refusal;
    }
    const size_t T = (size_t)total;
    // the arena for the hits and the per-hit and per-group arrays of the chain stages (regrow_arena)
    if (regrow_arena(ctx, seed_batch_bytes(n, k, 0) + (kLocateBytesPerHit + kChainBytesPerHit) * T)) front.rerun(ctx, h, b, true);
    const LocateSorted sorted = front.hits(ctx, h, n, T);
    res.num_seed_hits = T;
    const ChainAnchors anchors =
        rlz_seed_chain_anchors(ctx, h.view, (uint32_t)h.m, front.m.batch, front.d_seeds, front.m.d_len, front.S, sorted, (uint32_t)T);
    const ChainsOut run = rlz_seed_chain_run(ctx, anchors, chain_rules(p, h.m, h.view.B));
    deliver_chains(ctx, run, res);
    return refusal;
}

void index_seed_chains(const nolzss_rlz_index *h, const char *const *targets, const size_t *target_lens, size_t k,
                       const nolzss_rlz_chain_params *params, nolzss_rlz_seed_chains_result *out) {
    if (!out) throw std::invalid_argument("output pointer is null");
    std::memset(out, 0, sizeof *out);
    if (!h) throw std::invalid_argument("handle is null");
    if (!params) throw std::invalid_argument("rlz index: seed chains need their parameters: params is null");
    if (k > kChainMaxTargets)
        throw std::invalid_argument("rlz index: seed chains take at most 2^24 targets per batch, this one has " + std::to_string(k) +
                                    " (the group sort key keeps the target in 24 bits): send fewer targets");
    for (size_t j = 0; target_lens && j < k; ++j)  // (the lengths alone decide; a null array is the batch's refusal below)
        if (target_lens[j] >= (size_t(1) << 31))
            throw std::invalid_argument("rlz index: seed chains take targets below 2^31 bases, target " + std::to_string(j) +
                                        " has " + std::to_string(target_lens[j]) + " (a chain's score is kept in 32 bits)");
    Batch b;
    prepare_batch(*h, targets, target_lens, k, b);
    nolzss_rlz_seed_chains_result res;
    std::memset(&res, 0, sizeof res);
    std::string refusal;
    run_seed_query(*h, b, k, "rlz_index_seed_chains", res.anchor_offsets, [&] { nolzss_free_rlz_seed_chains_result(&res); },
                   [&](Context &ctx) { refusal = query_seed_chains(ctx, *h, b, k, *params, res); });
    if (!refusal.empty()) {  // an empty result and the status
        nolzss_free_rlz_seed_chains_result(&res);
        throw std::invalid_argument(refusal);
    }
    *out = res;  // ownership moves to the caller
}

// ---- base-level alignments -----------------------------------------------------------------------------------------
// the alignments of a run into the host blocks of a result (op_offsets: allocated here)
void deliver_alignments(Context &ctx, const AlignOut &run, nolzss_rlz_align_result &res) {
    const size_t C = run.num_alignments, N = run.num_ops;
    res.op_offsets = calloc_array<uint64_t>(C + 1);
    if (C == 0) return;
    res.alignments = static_cast<nolzss_rlz_alignment *>(alloc_factor_block(sizeof(nolzss_rlz_alignment) * C));
    if (!res.alignments) throw std::bad_alloc();
    res.ops = static_cast<uint32_t *>(alloc_factor_block(sizeof(uint32_t) * N));
    if (!res.ops) throw std::bad_alloc();
    download_records(ctx, "align_records_d2h", res.alignments, run.recs, C, sizeof(nolzss_rlz_alignment));
    download_records(ctx, "align_offsets_d2h", res.op_offsets, run.op_offsets, C + 1, sizeof(uint64_t));
    download_records(ctx, "align_ops_d2h", res.ops, run.ops, N, sizeof(uint32_t));
    res.num_alignments = C;
    res.num_ops = N;
}

void index_align(const nolzss_rlz_index *h, const char *const *targets, const size_t *target_lens, size_t k,
                 const nolzss_rlz_align_params *params, nolzss_rlz_align_result *out) {
    if (!out) throw std::invalid_argument("output pointer is null");
    std::memset(out, 0, sizeof *out);
    if (!h) throw std::invalid_argument("handle is null");
    if (!params) throw std::invalid_argument("rlz index: alignments need their parameters: params is null");
    if (k > kChainMaxTargets) check_align_batch_shape(nullptr, k);  // (the number of targets before the parameters)
    check_align_params(params);
    check_align_batch_shape(target_lens, k);
    Batch b;
    prepare_batch(*h, targets, target_lens, k, b);
    nolzss_rlz_align_result res;
    std::memset(&res, 0, sizeof res);
    std::string refusal;
    run_seed_query(*h, b, k, "rlz_index_align", res.op_offsets, [&] { nolzss_free_rlz_align_result(&res); }, [&](Context &ctx) {
        AlignRun run;
        refusal = align_batch(ctx, *h, b, k, *params, 0, run);
        if (!refusal.empty()) return;
        res.num_jobs = run.num_jobs;
        res.num_rows = run.num_rows;
        deliver_alignments(ctx, run.out, res);
    });
    if (!refusal.empty()) {  // an empty result and the status
        nolzss_free_rlz_align_result(&res);
        throw std::invalid_argument(refusal);
    }
    *out = res;  // ownership moves to the caller
}

}  // namespace

// ---- what the align query shares with the pileup (rlz_handles.hpp) ---------------------------------------------------
void nolzss::api::check_align_params(const nolzss_rlz_align_params *params) {
    if (!params) throw std::invalid_argument("rlz index: alignments need their parameters: params is null");
    if (params->bandwidth >= kAlignLanes || params->band >= kAlignLanes || params->bandwidth + 2 * params->band + 1 > kAlignLanes)
        throw std::invalid_argument("rlz index: an alignment job has at most 64 diagonals, one per lane of a wavefront: bandwidth + 2 "
                                    "band + 1 is " + std::to_string(params->bandwidth) + " + 2 * " + std::to_string(params->band) +
                                    " + 1: lower bandwidth or band");
}

void nolzss::api::check_align_batch_shape(const size_t *target_lens, size_t k) {
    if (k > kChainMaxTargets)
        throw std::invalid_argument("rlz index: seed chains take at most 2^24 targets per batch, this one has " + std::to_string(k) +
                                    " (the group sort key keeps the target in 24 bits): send fewer targets");
    for (size_t j = 0; target_lens && j < k; ++j)  // (the lengths alone decide; a null array is the batch's refusal)
        if (target_lens[j] >= kAlignMaxTarget)
            throw std::invalid_argument("rlz index: alignments take targets below 2^28 bases, target " + std::to_string(j) + " has " +
                                        std::to_string(target_lens[j]) + " (an op keeps its length in 28 bits)");
}

// The path of query_seed_chains up to the chains, which stay on the device, then the align stages.
std::string nolzss::api::align_batch(Context &ctx, const nolzss_rlz_index &h, const Batch &b, size_t k,
                                     const nolzss_rlz_align_params &p, size_t extra_per_slot, AlignRun &out) {
    const size_t n = b.tcat.size();
    nolzss_rlz_chain_params cp;
    cp.min_length = p.min_length;
    cp.max_hits = p.max_hits;
    cp.max_gap = p.max_gap;
    cp.bandwidth = p.bandwidth;
    cp.min_score = p.min_score;
    const ChainRules rules = chain_rules(cp, h.m, h.view.B);
    SeedFront front(p.min_length, p.max_hits);
    reserve_arena_for(ctx, 0, seed_batch_bytes(n, k, 0));
    front.run(ctx, h, b, true);
    front.refuse_too_many();
    const uint64_t total = front.hit_total(ctx);
    const std::string refusal = hits_refusal(total, p.max_hits, p.min_length);
    if (!refusal.empty() || total == 0) return refusal;
    const size_t T = (size_t)total;
    // the chains and the jobs of the batch, planned and sized: three totals come down
    ChainsOut run;
    AlignJobs jobs;
    auto run_chains = [&] {
        const LocateSorted sorted = front.hits(ctx, h, n, T);
        const ChainAnchors anchors =
            rlz_seed_chain_anchors(ctx, h.view, (uint32_t)h.m, front.m.batch, front.d_seeds, front.m.d_len, front.S, sorted, (uint32_t)T);
        run = rlz_seed_chain_run(ctx, anchors, rules);
        jobs = rlz_align_plan(ctx, h.view, front.m.batch, run, (uint32_t)p.band, p.max_flank);
        rlz_align_sizes(ctx, jobs);
    };
    // the arena (regrow_arena) twice: once the hits are counted for what is per hit, once the jobs are sized for what is
    // per DP row and per column slot -- the batch is then searched and also chained and planned again
    const size_t per_hit = seed_batch_bytes(n, k, 0) + (kLocateBytesPerHit + kChainBytesPerHit + kAlignBytesPerHit) * T;
    if (regrow_arena(ctx, per_hit)) front.rerun(ctx, h, b, true);
    run_chains();
    if (run.num_chains == 0) return refusal;
    const uint64_t rows = jobs.total_rows, slots = jobs.total_slots, weight = jobs.total_weight;
    if (rows > 0xffffffffull || slots > 0xffffffffull || weight > 0xffffffffull)
        return "rlz index: the alignments of this batch take " + std::to_string(rows) + " DP rows, " + std::to_string(slots) +
               " column slots and up to " + std::to_string(weight) + " columns, and each is counted in 32 bits: send fewer targets";
    if (regrow_arena(ctx, per_hit + kAlignBytesPerRow * (size_t)rows + (kAlignBytesPerSlot + extra_per_slot) * (size_t)slots)) {
        front.rerun(ctx, h, b, true);
        run_chains();
        if (jobs.total_rows != rows || jobs.total_slots != slots || jobs.total_weight != weight)
            throw HipError("rlz index: the alignment jobs of a batch changed between two runs");
    }
    rlz_align_layout(ctx, jobs);
    rlz_align_dp(ctx, jobs, front.m.batch, h.view.text);
    rlz_align_traceback(ctx, jobs);
    out.out = rlz_align_ops(ctx, jobs, run, rules);
    out.batch = front.m.batch;
    out.num_jobs = jobs.J;
    out.num_rows = (size_t)rows;
    return refusal;
}

// ---- what the seed-chain query shares with its debug hook (rlz_handles.hpp) -----------------------------------------
// the chains of a run into the host blocks of a result (anchor_offsets: allocated here)
void nolzss::api::deliver_chains(Context &ctx, const ChainsOut &run, nolzss_rlz_seed_chains_result &res) {
    const size_t C = run.num_chains, A = run.num_anchors;
    res.anchor_offsets = calloc_array<uint64_t>(C + 1);
    if (C == 0) return;
    res.chains = static_cast<nolzss_rlz_chain *>(alloc_factor_block(sizeof(nolzss_rlz_chain) * C));
    if (!res.chains) throw std::bad_alloc();
    res.anchors = static_cast<nolzss_rlz_chain_anchor *>(alloc_factor_block(sizeof(nolzss_rlz_chain_anchor) * A));
    if (!res.anchors) throw std::bad_alloc();
    download_records(ctx, "chains_d2h", res.chains, run.chains, C, sizeof(nolzss_rlz_chain));
    download_records(ctx, "chain_offsets_d2h", res.anchor_offsets, run.offsets, C + 1, sizeof(uint64_t));
    download_records(ctx, "chain_anchors_d2h", res.anchors, run.anchors, A, sizeof(nolzss_rlz_chain_anchor));
    res.num_chains = C;
    res.num_anchors = A;
}

ChainRules nolzss::api::chain_rules(const nolzss_rlz_chain_params &p, uint64_t records, uint64_t B) {
    ChainRules r;
    r.max_gap = p.max_gap >= 0xffffffffull ? 0xffffffffu : (uint32_t)p.max_gap;
    r.bandwidth = p.bandwidth >= 0xffffffffull ? 0xffffffffu : (uint32_t)p.bandwidth;
    r.min_score = p.min_score;
    r.records = (uint32_t)records;
    r.B = (uint32_t)B;
    return r;
}

extern "C" {

int nolzss_rlz_index_seeds(const nolzss_rlz_index *h, const char *const *targets, const size_t *target_lens, size_t k,
                           uint64_t min_length, uint64_t max_hits, nolzss_rlz_seeds_result *out) {
    return guarded([&] { index_seeds(h, targets, target_lens, k, min_length, max_hits, out); });
}

void nolzss_free_rlz_seeds_result(nolzss_rlz_seeds_result *r) {
    if (!r) return;
    free_block(r->seeds);
    free_block(r->hit_offsets);
    free_block(r->hits);
    std::memset(r, 0, sizeof *r);
}

int nolzss_rlz_index_seed_chains(const nolzss_rlz_index *h, const char *const *targets, const size_t *target_lens, size_t k,
                                 const nolzss_rlz_chain_params *params, nolzss_rlz_seed_chains_result *out) {
    return guarded([&] { index_seed_chains(h, targets, target_lens, k, params, out); });
}

void nolzss_free_rlz_seed_chains_result(nolzss_rlz_seed_chains_result *r) {
    if (!r) return;
    free_block(r->chains);
    free_block(r->anchor_offsets);
    free_block(r->anchors);
    std::memset(r, 0, sizeof *r);
}

int nolzss_rlz_index_align(const nolzss_rlz_index *h, const char *const *targets, const size_t *target_lens, size_t k,
                           const nolzss_rlz_align_params *params, nolzss_rlz_align_result *out) {
    return guarded([&] { index_align(h, targets, target_lens, k, params, out); });
}

void nolzss_free_rlz_align_result(nolzss_rlz_align_result *r) {
    if (!r) return;
    free_block(r->alignments);
    free_block(r->op_offsets);
    free_block(r->ops);
    std::memset(r, 0, sizeof *r);
}

}  // extern "C"
