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
static_assert(NOLZSS_RLZ_PILEUP_CHANNELS == kPileupChannels, "the channels of a position are a constant of the ABI");

constexpr uint64_t kPileupMaxTargets = 0x7fffffffull;  // two alignments per target and position at most: counters below 2^32
// arena bytes per column slot of an add, behind rlz_align_ops: the two sizes and the two prefixes of an op (16; an op
// is at most one per slot) and the tile sums of their scans
constexpr size_t kPileupBytesPerSlot = 17;

void pileup_open(const nolzss_rlz_index *ix, const nolzss_rlz_align_params *params, nolzss_rlz_pileup **out) {
    if (!out) throw std::invalid_argument("output pointer is null");
    *out = nullptr;
    if (!ix) throw std::invalid_argument("handle is null");
    check_align_params(params);
    std::unique_ptr<nolzss_rlz_pileup> p(new nolzss_rlz_pileup);
    p->device = ix->device;
    p->index = ix;
    p->params = *params;
    const uint32_t B = ix->view.B;
    DeviceRestore restore;
    Session ses(ix->device, nullptr);
    Context &ctx = ses.ctx();
    {
        ProfScope whole(ctx.profiler(), "rlz_pileup_open", ctx.stream);
        p->device_bytes = rlz_pileup_footprint(B);
        p->d_base = device_alloc(ctx, p->device_bytes);  // (a throw frees the handle: the index is untouched)
        p->view = rlz_pileup_view(p->d_base, B);
        HIP_CHECK(hipMemsetAsync(p->d_base, 0, p->device_bytes, ctx.stream));
    }
    HIP_CHECK(hipStreamSynchronize(ctx.stream));
    ctx.prof.collect();
    *out = p.release();
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
    unsigned long long stats[3] = {0, 0, 0};
    std::string refusal;
    with_index_session(h.device, "rlz_pileup_add", [&](Context &ctx) {
        AlignRun run;
        refusal = align_batch(ctx, h, b, k, p->params, kPileupBytesPerSlot, run);
        if (!refusal.empty() || run.out.num_alignments == 0) return;
        unsigned long long *d_stats = ctx.arena.alloc<unsigned long long>(3);
        // from here on the counters change: nothing below refuses, and every arena array is taken before the first write
        rlz_pileup_accumulate(ctx, p->view, run.out, run.batch, primary_only != 0, d_stats);
        p->dirty = true;
        download_bytes(ctx, stats, d_stats, sizeof stats);
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
    if (den == 0 || num > den || min_count == 0)
        throw std::invalid_argument("rlz pileup: variants take min_count >= 1 and a fraction 0 <= num / den <= 1 with den >= 1, not "
                                    "min_count " + std::to_string(min_count) + " and " + std::to_string(num) + " / " +
                                    std::to_string(den));
    if (den > 0xffffffffull)  // (num <= den: both factors of either product then fit 32 bits)
        throw std::invalid_argument("rlz pileup: the fraction's denominator must fit 32 bits (the products are taken in 64)");
    const uint32_t B = p->view.B;
    if (B == 0) return;
    std::lock_guard<std::mutex> lock(p->mu);
    PileupRule rule;
    rule.min_count = min_count;
    rule.num = num;
    rule.den = den;
    const size_t chunk_max = chunk_knob("NOLZSS_RLZ_LOCATE_CHUNK");
    nolzss_rlz_variant *recs = nullptr;
    try {
        with_index_session(p->device, "rlz_pileup_variants_call", [&](Context &ctx) {
            const size_t most = 5 * (size_t)B < chunk_max ? 5 * (size_t)B : chunk_max;
            reserve_arena_for(ctx, 0, 9 * (size_t)B + sizeof(PileupVariantRec) * most + (size_t(4) << 20));
            resolve(ctx, *p);
            const PackedText &block = p->index->view.text;
            uint32_t *d_n = ctx.arena.alloc<uint32_t>(B), *d_off = ctx.arena.alloc<uint32_t>(B);
            uint64_t *d_total = ctx.arena.alloc<uint64_t>(1);
            uint64_t total = 0;  // up to five records per position: summed in 64 bits, one word comes down
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
            recs = static_cast<nolzss_rlz_variant *>(alloc_factor_block(sizeof(nolzss_rlz_variant) * (size_t)total));
            if (!recs) throw std::bad_alloc();
            const size_t chunk = total < chunk_max ? total : chunk_max;
            PileupVariantRec *d_stage = ctx.arena.alloc<PileupVariantRec>(chunk);
            download_produced(ctx, "pileup_variants_d2h", recs, d_stage, total, sizeof(PileupVariantRec), chunk,
                              [&](size_t c0, size_t c) {
                                  rlz_pileup_variant_records(ctx, p->view, block, rule, d_off, c0, (uint32_t)c, d_stage);
                              });
            out->num_variants = total;
        });
    } catch (...) {
        free_block(recs);
        std::memset(out, 0, sizeof *out);
        throw;
    }
    out->variants = recs;
}

}  // namespace

extern "C" {

int nolzss_rlz_pileup_open(const nolzss_rlz_index *index, const nolzss_rlz_align_params *params, nolzss_rlz_pileup **out) {
    return guarded([&] { pileup_open(index, params, out); });
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
        info->device_bytes = p->device_bytes;
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
