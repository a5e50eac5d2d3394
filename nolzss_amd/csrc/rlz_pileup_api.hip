// rlz_pileup_api.hip -- the pileup handle of the relative-LZ index and its entry points (part of the C ABI layer of
// libnolzss_hip.so, include/nolzss_hip.h, nolzss_rlz_pileup_*; the kernels: rlz_pileup.hip; DESIGN.md 5, "Relative-LZ
// index: pileup").  A pileup holds eight counters per position of the block in device memory of its own; an add runs a
// batch through the align path of the index (align_batch, rlz_index_seeds_api.hip) and reduces the alignments there, so
// neither records nor ops come down; counts and variants bring down the table.
#include "rlz_handles.hpp"

using namespace nolzss;
using namespace nolzss::api;

namespace {

static_assert(sizeof(nolzss_rlz_variant) == sizeof(PileupVariantRec) && sizeof(PileupVariantRec) == 40,
              "the kernels write nolzss_rlz_variant");
static_assert(sizeof(nolzss_rlz_insertion) == sizeof(PileupInsertionRec) && sizeof(PileupInsertionRec) == 56,
              "the kernels write nolzss_rlz_insertion");
static_assert(sizeof(PileupEvent) == 24 && sizeof(PileupAllele) == 32, "an event of the log keeps 24 bytes");
static_assert(NOLZSS_RLZ_PILEUP_NORMALIZE == kPileupNormalize && NOLZSS_RLZ_PILEUP_MAX_SHIFT == kPileupMaxShift &&
                  NOLZSS_RLZ_PILEUP_INS_BASES == kPileupInsBases,
              "the flag, the cap of a shift and the bases of an event are constants of the ABI");
static_assert(NOLZSS_RLZ_PILEUP_CHANNELS == kPileupChannels, "the channels of a position are a constant of the ABI");

constexpr uint64_t kPileupMaxTargets = 0x7fffffffull;  // two alignments per target and position at most: counters below 2^32
// arena bytes per column slot of an add, behind rlz_align_ops: the two sizes and the two prefixes of an op (16; an op
// is at most one per slot) and the tile sums of their scans
constexpr size_t kPileupBytesPerSlot = 17;

constexpr uint64_t kPileupMaxEvents = 0xffffffffull;  // the log and the allele table are indexed in 32 bits
constexpr uint64_t kPileupFirstLogEvents = 4096;

void pileup_open(const nolzss_rlz_index *ix, const nolzss_rlz_align_params *params, uint32_t flags, nolzss_rlz_pileup **out) {
    if (!out) throw std::invalid_argument("output pointer is null");
    *out = nullptr;
    if (flags & ~NOLZSS_RLZ_PILEUP_NORMALIZE)
        throw std::invalid_argument("rlz pileup: unknown flag bits " + std::to_string(flags & ~NOLZSS_RLZ_PILEUP_NORMALIZE));
    if (!ix) throw std::invalid_argument("handle is null");
    check_align_params(params);
    std::unique_ptr<nolzss_rlz_pileup> p(new nolzss_rlz_pileup);
    p->device = ix->device;
    p->index = ix;
    p->params = *params;
    p->flags = flags;
    const uint32_t B = ix->view.B;
    with_index_session(ix->device, "rlz_pileup_open", [&](Context &ctx) {
        p->base.alloc(ctx, rlz_pileup_footprint(B));  // (a throw frees the handle: the index is untouched)
        p->view = rlz_pileup_view(p->base.get(), B);
        HIP_CHECK(hipMemsetAsync(p->base.get(), 0, p->base.bytes(), ctx.stream));
    });
    *out = p.release();
}

// Room for `more` events behind those logged (DeviceBuf::grow_keeping).
void grow_log(Context &ctx, nolzss_rlz_pileup &p, uint64_t more) {
    const uint64_t need = p.events + more, held = p.log_capacity();
    if (need <= held) return;
    uint64_t cap = held ? 2 * held : kPileupFirstLogEvents;
    if (!held)
        if (const char *e = getenv("NOLZSS_RLZ_PILEUP_LOG_EVENTS")) {
            const unsigned long long v = strtoull(e, nullptr, 10);
            if (v >= 1 && v <= kPileupMaxEvents) cap = v;
        }
    cap = cap < need ? need : cap;
    cap = cap < kPileupMaxEvents ? cap : kPileupMaxEvents;
    ProfScope ps(ctx.profiler(), "rlz_pileup_log_grow", ctx.stream, 2.0 * sizeof(PileupEvent) * (double)p.events);
    p.log.grow_keeping(ctx, sizeof(PileupEvent) * (size_t)cap, sizeof(PileupEvent) * (size_t)p.events);
}

void pileup_add(nolzss_rlz_pileup *p, const char *const *targets, const size_t *target_lens, size_t k, int primary_only,
                nolzss_rlz_pileup_add_info *info) {
    if (!info) throw std::invalid_argument("output pointer is null");
    std::memset(info, 0, sizeof *info);
    if (!p) throw std::invalid_argument("handle is null");
    check_align_batch_shape(target_lens, k);  // (decided before the handle is read)
    std::lock_guard<std::mutex> lock(p->mu);
    const nolzss_rlz_index &h = *p->index;
    Batch b;
    prepare_batch(h, targets, target_lens, k, b);
    if (p->targets + k > kPileupMaxTargets)
        throw std::invalid_argument("rlz pileup: a pileup takes at most 2^31 - 1 targets, this one holds " + std::to_string(p->targets) +
                                    " and the batch has " + std::to_string(k) + " (a counter keeps 32 bits): open another pileup");
    info->targets = p->targets;
    if (b.tcat.size() == k) {  // no target, or none with a base: the device is not touched
        p->targets += k;
        info->targets = p->targets;
        return;
    }
    unsigned long long stats[kPileupStats] = {0, 0, 0, 0};
    std::string refusal;
    with_index_session(h.device, "rlz_pileup_add", [&](Context &ctx) {
        AlignRun run;
        refusal = align_batch(ctx, h, b, k, p->params, kPileupBytesPerSlot, run);
        if (!refusal.empty() || run.out.num_alignments == 0) return;
        unsigned long long *d_stats = ctx.arena.alloc<unsigned long long>(kPileupStats + 1);
        // the events of the batch, counted before anything is written: the log's room is secured, or the add refused
        unsigned long long more = 0;
        rlz_pileup_count_insertions(ctx, run.out, run.batch, p->view.B, primary_only != 0, d_stats + kPileupStats);
        download_bytes(ctx, &more, d_stats + kPileupStats, sizeof more);
        if (p->events + more > kPileupMaxEvents) {
            refusal = "rlz pileup: the insertion log holds " + std::to_string(p->events) + " events and the batch has " +
                      std::to_string(more) + ", beyond 2^32 - 1: open another pileup";
            return;
        }
        grow_log(ctx, *p, more);
        PileupLog log;
        log.events = p->log.as<PileupEvent>();
        log.base = p->events;
        log.capacity = p->log_capacity();
        log.flags = p->flags;
        // from here on the counters change: nothing below refuses, and every arena array is taken before the first write
        rlz_pileup_accumulate(ctx, p->view, run.out, run.batch, h.view.text, primary_only != 0, log, d_stats);
        p->dirty = true;
        p->alleles_valid = false;
        download_bytes(ctx, stats, d_stats, sizeof stats);
        p->events += stats[3] < more ? stats[3] : more;
    });
    if (!refusal.empty()) throw std::invalid_argument(refusal);
    p->targets += k;
    p->alignments += stats[0];
    p->ops += stats[1];
    p->columns += stats[2];
    p->adds += 1;
    info->alignments = stats[0];
    info->ops = stats[1];
    info->columns = stats[2];
    info->targets = p->targets;
}

// the difference entries scanned into depths if an add has changed them since the last read
void resolve(Context &ctx, nolzss_rlz_pileup &p) {
    if (!p.dirty) return;
    rlz_pileup_resolve(ctx, p.view);
    p.dirty = false;
}

void pileup_counts(nolzss_rlz_pileup *p, uint64_t start, uint64_t end, uint32_t *out) {
    if (!p) throw std::invalid_argument("handle is null");
    if (start > end || end > p->view.B)  // (the block's length never changes: read without the lock)
        throw std::invalid_argument("rlz pileup: counts take 0 <= start <= end <= block length (" + std::to_string(p->view.B) +
                                    "), not [" + std::to_string(start) + ", " + std::to_string(end) + ")");
    const size_t count = (size_t)(end - start);
    if (count == 0) return;
    if (!out) throw std::invalid_argument("output pointer is null");
    std::lock_guard<std::mutex> lock(p->mu);
    const size_t chunk_max = chunk_knob("NOLZSS_RLZ_LOCATE_CHUNK");
    const size_t chunk = count < chunk_max ? count : chunk_max, row = sizeof(uint32_t) * kPileupChannels;
    with_index_session(p->device, "rlz_pileup_counts_call", [&](Context &ctx) {
        reserve_arena_for(ctx, 0, row * chunk + (size_t(4) << 20));
        resolve(ctx, *p);
        uint32_t *d_stage = ctx.arena.alloc<uint32_t>(kPileupChannels * chunk);
        download_produced(ctx, "pileup_counts_d2h", out, d_stage, count, row, chunk, [&](size_t c0, size_t c) {
            rlz_pileup_compose(ctx, p->view, p->index->view.text, (uint32_t)(start + c0), (uint32_t)c, d_stage);
        });
    });
}

void pileup_variants(nolzss_rlz_pileup *p, uint32_t min_count, uint64_t num, uint64_t den, nolzss_rlz_variants_result *out) {
    if (!out) throw std::invalid_argument("output pointer is null");
    std::memset(out, 0, sizeof *out);
    if (!p) throw std::invalid_argument("handle is null");
    const PileupRule rule = check_pileup_rule(min_count, num, den, "variants");
    const uint32_t B = p->view.B;
    if (B == 0) return;
    std::lock_guard<std::mutex> lock(p->mu);
    const size_t chunk_max = chunk_knob("NOLZSS_RLZ_LOCATE_CHUNK");
    HostBlock<nolzss_rlz_variant> recs;
    uint64_t total = 0;  // up to five records per position: summed in 64 bits, one word comes down
    with_index_session(p->device, "rlz_pileup_variants_call", [&](Context &ctx) {
        const size_t most = 5 * (size_t)B < chunk_max ? 5 * (size_t)B : chunk_max;
        reserve_arena_for(ctx, 0, 9 * (size_t)B + sizeof(PileupVariantRec) * most + (size_t(4) << 20));
        resolve(ctx, *p);
        const PackedText &block = p->index->view.text;
        uint32_t *d_n = ctx.arena.alloc<uint32_t>(B), *d_off = ctx.arena.alloc<uint32_t>(B);
        uint64_t *d_total = ctx.arena.alloc<uint64_t>(1);
        {
            ProfScope ps(ctx.profiler(), "rlz_pileup_variants", ctx.stream, 48.0 * (double)B);
            rlz_pileup_variant_flags(ctx, p->view, block, rule, d_n);
            rlz_index_rep_total(ctx, d_n, B, d_total);
            scan_exclusive_add_u32(d_n, d_off, B, nullptr, ctx.arena, ctx.stream);
            download_bytes(ctx, &total, d_total, sizeof total);
        }
        if (total > 0xffffffffull)
            throw std::invalid_argument("rlz pileup: variants would report " + std::to_string(total) +
                                        " records, and they are counted in 32 bits: raise min_count or the fraction");
        if (total == 0) return;
        recs = host_block<nolzss_rlz_variant>((size_t)total);
        const size_t chunk = total < chunk_max ? total : chunk_max;
        PileupVariantRec *d_stage = ctx.arena.alloc<PileupVariantRec>(chunk);
        download_produced(ctx, "pileup_variants_d2h", recs.get(), d_stage, total, sizeof(PileupVariantRec), chunk,
                          [&](size_t c0, size_t c) {
                              rlz_pileup_variant_records(ctx, p->view, block, rule, d_off, c0, (uint32_t)c, d_stage);
                          });
    });
    out->num_variants = total;  // (the result stays zeroed up to here: a throw above frees the block)
    out->variants = recs.release();
}

// The allele table of the log as it stands: built in the arena on the first read after an add, then kept in an
// allocation of the handle's own until the next add.
const PileupAllele *cached_alleles(Context &ctx, nolzss_rlz_pileup &p, uint32_t &G) {
    if (!p.alleles_valid) {
        uint32_t count = 0;
        const PileupAllele *d_built = rlz_pileup_alleles(ctx, p.log.as<PileupEvent>(), (uint32_t)p.events, &count);
        const size_t bytes = sizeof(PileupAllele) * (size_t)count;
        if (bytes > p.allele_table.bytes()) p.allele_table.grow_keeping(ctx, bytes, 0);
        if (count) HIP_CHECK(hipMemcpyAsync(p.allele_table.get(), d_built, bytes, hipMemcpyDeviceToDevice, ctx.stream));
        p.alleles = count;
        p.alleles_valid = true;
    }
    G = (uint32_t)p.alleles;
    return p.allele_table.as<PileupAllele>();
}

void pileup_insertions(nolzss_rlz_pileup *p, uint32_t min_count, uint64_t num, uint64_t den, nolzss_rlz_insertions_result *out) {
    if (!out) throw std::invalid_argument("output pointer is null");
    std::memset(out, 0, sizeof *out);
    if (!p) throw std::invalid_argument("handle is null");
    const PileupRule rule = check_pileup_rule(min_count, num, den, "insertions");
    std::lock_guard<std::mutex> lock(p->mu);
    if (p->view.B == 0 || p->events == 0) return;
    try {
        with_index_session(p->device, "rlz_pileup_insertions_call", [&](Context &ctx) {
            const size_t E = (size_t)p->events, chunk_max = chunk_knob("NOLZSS_RLZ_LOCATE_CHUNK");
            reserve_arena_for(ctx, 0, (kAllelesArenaPerEvent + kInsertionsArenaPerAllele) * E +
                                          sizeof(PileupInsertionRec) * (E < chunk_max ? E : chunk_max) + (size_t(4) << 20));
            resolve(ctx, *p);
            uint32_t G = 0;
            const PileupAllele *d_alleles = cached_alleles(ctx, *p, G);
            deliver_insertions(ctx, p->view, p->index->view.text, d_alleles, G, rule, *out);
        });
    } catch (...) {
        nolzss_free_rlz_insertions_result(out);
        throw;
    }
}

void pileup_consensus(nolzss_rlz_pileup *p, const nolzss_rlz_consensus_params *params, int want_map, nolzss_rlz_consensus_result *out) {
    if (!out) throw std::invalid_argument("output pointer is null");
    std::memset(out, 0, sizeof *out);
    if (!p) throw std::invalid_argument("handle is null");
    const ConsensusRule rule = check_consensus_params(params);
    std::lock_guard<std::mutex> lock(p->mu);
    const uint32_t B = p->view.B;
    if (B == 0) return;
    try {
        with_index_session(p->device, "rlz_pileup_consensus_call", [&](Context &ctx) {
            const size_t E = (size_t)p->events, chunk_max = chunk_knob("NOLZSS_RLZ_LOCATE_CHUNK");
            const size_t longest = (1 + (size_t)NOLZSS_RLZ_PILEUP_INS_BASES) * ((size_t)B + 1);  // bytes of text at most
            const size_t most = longest < chunk_max ? longest : chunk_max;
            reserve_arena_for(ctx, 0, kAllelesArenaPerEvent * E + kConsensusArenaPerBase * ((size_t)B + 1) + 8 * ((size_t)p->index->m + 1) +
                                          8 * most + (size_t(4) << 20));
            resolve(ctx, *p);
            uint32_t G = 0;
            const PileupAllele *d_alleles = cached_alleles(ctx, *p, G);
            deliver_consensus(ctx, p->view, p->index->view.text, (uint32_t)p->index->m, d_alleles, G, rule, want_map != 0, *out);
        });
    } catch (...) {
        nolzss_free_rlz_consensus_result(out);
        throw;
    }
}

}  // namespace

PileupRule nolzss::api::check_pileup_rule(uint32_t min_count, uint64_t num, uint64_t den, const char *what) {
    if (den == 0 || num > den || min_count == 0)
        throw std::invalid_argument(std::string("rlz pileup: ") + what + " take min_count >= 1 and a fraction 0 <= num / den <= 1 with "
                                    "den >= 1, not min_count " + std::to_string(min_count) + " and " + std::to_string(num) + " / " +
                                    std::to_string(den));
    if (den > 0xffffffffull)  // (num <= den: both factors of either product then fit 32 bits)
        throw std::invalid_argument("rlz pileup: the fraction's denominator must fit 32 bits (the products are taken in 64)");
    PileupRule rule;
    rule.min_count = min_count;
    rule.num = num;
    rule.den = den;
    return rule;
}

ConsensusRule nolzss::api::check_consensus_params(const nolzss_rlz_consensus_params *params) {
    if (!params) throw std::invalid_argument("params is null");
    if (params->min_depth == 0 || params->low > 1 || params->den == 0 || params->num > params->den)
        throw std::invalid_argument("rlz pileup: a consensus takes min_depth >= 1, low 0 or 1 and a fraction 0 <= num / den <= 1 with "
                                    "den >= 1, not min_depth " + std::to_string(params->min_depth) + ", low " +
                                    std::to_string(params->low) + " and " + std::to_string(params->num) + " / " +
                                    std::to_string(params->den));
    if (params->den > 0xffffffffull)
        throw std::invalid_argument("rlz pileup: the fraction's denominator must fit 32 bits (the products are taken in 64)");
    ConsensusRule rule;
    rule.min_depth = params->min_depth;
    rule.low = params->low;
    rule.num = params->num;
    rule.den = params->den;
    return rule;
}

void nolzss::api::deliver_insertions(Context &ctx, const PileupView &v, const PackedText &block, const PileupAllele *d_alleles,
                                     uint32_t G, const PileupRule &rule, nolzss_rlz_insertions_result &out) {
    if (G == 0) return;
    const size_t chunk_max = chunk_knob("NOLZSS_RLZ_LOCATE_CHUNK");
    uint32_t *d_n = ctx.arena.alloc<uint32_t>(G), *d_off = ctx.arena.alloc<uint32_t>(G), *d_total = ctx.arena.alloc<uint32_t>(1);
    uint32_t total = 0;  // at most G records: 32 bits hold them
    {
        ProfScope ps(ctx.profiler(), "rlz_pileup_insertions", ctx.stream, 88.0 * (double)G);
        rlz_pileup_insertion_flags(ctx, v, block, d_alleles, G, rule, d_n);
        scan_exclusive_add_u32(d_n, d_off, G, d_total, ctx.arena, ctx.stream);
        download_bytes(ctx, &total, d_total, sizeof total);
    }
    if (total == 0) return;
    out.insertions = static_cast<nolzss_rlz_insertion *>(alloc_factor_block(sizeof(nolzss_rlz_insertion) * (size_t)total));
    if (!out.insertions) throw std::bad_alloc();
    const size_t chunk = total < chunk_max ? total : chunk_max;
    PileupInsertionRec *d_stage = ctx.arena.alloc<PileupInsertionRec>(chunk);
    download_produced(ctx, "pileup_insertions_d2h", out.insertions, d_stage, total, sizeof(PileupInsertionRec), chunk,
                      [&](size_t c0, size_t c) {
                          rlz_pileup_insertion_records(ctx, v, block, d_alleles, G, d_n, d_off, c0, (uint32_t)c, d_stage);
                      });
    out.num_insertions = total;
}

void nolzss::api::deliver_consensus(Context &ctx, const PileupView &v, const PackedText &block, uint32_t records,
                                    const PileupAllele *d_alleles, uint32_t G, const ConsensusRule &rule, bool want_map,
                                    nolzss_rlz_consensus_result &out) {
    const uint32_t B = v.B;
    const size_t chunk_max = chunk_knob("NOLZSS_RLZ_LOCATE_CHUNK");
    uint32_t *d_len = ctx.arena.alloc<uint32_t>((size_t)B + 1), *d_off = ctx.arena.alloc<uint32_t>((size_t)B + 1);
    unsigned long long *d_stats = ctx.arena.alloc<unsigned long long>(kConsensusStats);
    uint64_t *d_total = ctx.arena.alloc<uint64_t>(1), *d_rec = ctx.arena.alloc<uint64_t>((size_t)records + 1);
    unsigned long long stats[kConsensusStats];
    uint64_t total = 0;  // up to 1 + NOLZSS_RLZ_PILEUP_INS_BASES bytes per position: summed in 64 bits
    {
        ProfScope ps(ctx.profiler(), "rlz_consensus", ctx.stream, 56.0 * (double)B);
        rlz_consensus_lengths(ctx, v, block, d_alleles, G, rule, d_len, d_stats);
        rlz_index_rep_total(ctx, d_len, B, d_total);
        scan_exclusive_add_u32(d_len, d_off, (size_t)B + 1, nullptr, ctx.arena, ctx.stream);
        download_bytes(ctx, &total, d_total, sizeof total);
    }
    if (total > 0xffffffffull)
        throw std::invalid_argument("rlz pileup: the consensus would hold " + std::to_string(total) +
                                    " bytes, and its offsets are counted in 32 bits");
    rlz_consensus_record_offsets(ctx, block, d_off, B, records, total, d_rec);
    out.record_offsets = calloc_array<uint64_t>((size_t)records + 1);
    download_records(ctx, "consensus_records_d2h", out.record_offsets, d_rec, (size_t)records + 1, sizeof(uint64_t));
    download_bytes(ctx, stats, d_stats, sizeof stats);
    out.text = static_cast<char *>(alloc_factor_block(total ? (size_t)total : 1));
    if (!out.text) throw std::bad_alloc();
    const size_t most = ((size_t)B + 1 > total ? (size_t)B + 1 : (size_t)total);
    const size_t chunk = most < chunk_max ? most : chunk_max;
    uint64_t *d_stage = ctx.arena.alloc<uint64_t>(chunk);  // the text's bytes, then the map's words
    if (total)
        download_produced(ctx, "consensus_text_d2h", out.text, d_stage, (size_t)total, 1, chunk, [&](size_t c0, size_t c) {
            rlz_consensus_text(ctx, v, block, d_alleles, G, rule, d_off, c0, (uint32_t)c, reinterpret_cast<uint8_t *>(d_stage));
        });
    if (want_map) {
        out.starts = static_cast<uint64_t *>(alloc_factor_block(sizeof(uint64_t) * ((size_t)B + 1)));
        if (!out.starts) throw std::bad_alloc();
        download_produced(ctx, "consensus_map_d2h", out.starts, d_stage, (size_t)B + 1, sizeof(uint64_t), chunk,
                          [&](size_t c0, size_t c) { rlz_consensus_starts(ctx, d_off, c0, (uint32_t)c, d_stage); });
    }
    out.length = (size_t)total;
    out.num_records = records;
    out.called = stats[0];
    out.low_positions = stats[1];
    out.substitutions = stats[2];
    out.deleted = stats[3];
    out.insertions = stats[4];
    out.inserted_bases = stats[5];
    out.truncated_skipped = stats[6];
}

extern "C" {

int nolzss_rlz_pileup_open(const nolzss_rlz_index *index, const nolzss_rlz_align_params *params, nolzss_rlz_pileup **out) {
    return guarded([&] { pileup_open(index, params, 0, out); });
}

int nolzss_rlz_pileup_open_flags(const nolzss_rlz_index *index, const nolzss_rlz_align_params *params, uint32_t flags,
                                 nolzss_rlz_pileup **out) {
    return guarded([&] { pileup_open(index, params, flags, out); });
}

int nolzss_rlz_pileup_log_info(nolzss_rlz_pileup *p, uint32_t *flags, uint64_t *events, uint64_t *log_bytes) {
    return guarded([&] {
        if (!p || !flags || !events || !log_bytes) throw std::invalid_argument("handle or output pointer is null");
        std::lock_guard<std::mutex> lock(p->mu);
        *flags = p->flags;
        *events = p->events;
        *log_bytes = p->log.bytes();
    });
}

int nolzss_rlz_pileup_insertions(nolzss_rlz_pileup *p, uint32_t min_count, uint64_t num, uint64_t den,
                                 nolzss_rlz_insertions_result *out) {
    return guarded([&] { pileup_insertions(p, min_count, num, den, out); });
}

void nolzss_free_rlz_insertions_result(nolzss_rlz_insertions_result *r) {
    if (!r) return;
    free_block(r->insertions);
    std::memset(r, 0, sizeof *r);
}

int nolzss_rlz_pileup_consensus(nolzss_rlz_pileup *p, const nolzss_rlz_consensus_params *params, int want_map,
                                nolzss_rlz_consensus_result *out) {
    return guarded([&] { pileup_consensus(p, params, want_map, out); });
}

void nolzss_free_rlz_consensus_result(nolzss_rlz_consensus_result *r) {
    if (!r) return;
    free_block(r->text);
    free_block(r->record_offsets);
    free_block(r->starts);
    std::memset(r, 0, sizeof *r);
}

int nolzss_rlz_pileup_add(nolzss_rlz_pileup *p, const char *const *targets, const size_t *target_lens, size_t k,
                          int primary_only, nolzss_rlz_pileup_add_info *info) {
    return guarded([&] { pileup_add(p, targets, target_lens, k, primary_only, info); });
}

int nolzss_rlz_pileup_counts(nolzss_rlz_pileup *p, uint64_t start, uint64_t end, uint32_t *out) {
    return guarded([&] { pileup_counts(p, start, end, out); });
}

int nolzss_rlz_pileup_variants(nolzss_rlz_pileup *p, uint32_t min_count, uint64_t num, uint64_t den,
                               nolzss_rlz_variants_result *out) {
    return guarded([&] { pileup_variants(p, min_count, num, den, out); });
}

void nolzss_free_rlz_variants_result(nolzss_rlz_variants_result *r) {
    if (!r) return;
    free_block(r->variants);
    std::memset(r, 0, sizeof *r);
}

int nolzss_rlz_pileup_info(nolzss_rlz_pileup *p, nolzss_rlz_pileup_summary *info) {
    return guarded([&] {
        if (!p || !info) throw std::invalid_argument("handle or output pointer is null");
        std::memset(info, 0, sizeof *info);
        std::lock_guard<std::mutex> lock(p->mu);
        info->block_length = p->view.B;
        info->device_bytes = p->base.bytes();
        info->targets = p->targets;
        info->alignments = p->alignments;
        info->ops = p->ops;
        info->columns = p->columns;
        info->adds = p->adds;
        info->device = p->device;
        info->dirty = p->dirty ? 1 : 0;
        info->params = p->params;
    });
}

int nolzss_rlz_pileup_close(nolzss_rlz_pileup *p) {
    return guarded([&] { delete p; });
}

}  // extern "C"
