// rlz_cohort_api.hip -- the cohort handle of the relative-LZ index and its entry points (part of the C ABI layer of
// libnolzss_hip.so, include/nolzss_hip.h, nolzss_rlz_cohort_*; the kernels: rlz_cohort.hip; DESIGN.md 5, "Relative-LZ
// index: cohort").  A cohort holds three bit planes per sample in device memory of its own; an add packs the calls of a
// resolved pileup, or of a byte string, into the next sample's planes and brings down four counts; distances, sites,
// columns and calls read the planes and bring down their results through arena memory.
#include "rlz_handles.hpp"

using namespace nolzss;
using namespace nolzss::api;

namespace {

static_assert(sizeof(nolzss_rlz_cohort_site) == sizeof(CohortSiteRec) && sizeof(CohortSiteRec) == 48,
              "the kernels write nolzss_rlz_cohort_site");
// both matrices of a full cohort, 2 x N^2 cells of 4 bytes, stay below 2^32 bytes
static_assert((uint64_t)NOLZSS_RLZ_COHORT_MAX_SAMPLES * NOLZSS_RLZ_COHORT_MAX_SAMPLES * 2 * sizeof(uint32_t) <= (1ull << 32),
              "the matrices of a full cohort stay addressable in 32 bits");

constexpr uint64_t kCohortDefaultBytes = uint64_t(256) << 20, kCohortDefaultSamples = 64;

size_t sample_bytes(const nolzss_rlz_cohort &c) { return 3 * sizeof(uint64_t) * c.W; }

void cohort_open(const nolzss_rlz_index *ix, nolzss_rlz_cohort **out) {
    if (!out) throw std::invalid_argument("output pointer is null");
    *out = nullptr;
    if (!ix) throw std::invalid_argument("handle is null");
    std::unique_ptr<nolzss_rlz_cohort> c(new nolzss_rlz_cohort);
    c->device = ix->device;
    c->index = ix;
    c->index_serial = ix->serial;
    c->B = ix->view.B;
    c->W = cohort_words(c->B);
    const uint64_t per = sample_bytes(*c) ? sample_bytes(*c) : 1;
    uint64_t first = kCohortDefaultBytes / per;
    first = first < 1 ? 1 : (first < kCohortDefaultSamples ? first : kCohortDefaultSamples);
    if (const char *e = getenv("NOLZSS_RLZ_COHORT_SAMPLES")) {
        const unsigned long long v = strtoull(e, nullptr, 10);
        if (v >= 1 && v <= NOLZSS_RLZ_COHORT_MAX_SAMPLES) first = v;
    }
    c->first_capacity = first;
    *out = c.release();  // (no device memory until the first add)
}

// Room for one more sample (DeviceBuf::grow_keeping; a cohort of block length 0 never comes here, so a sample has bytes).
void secure_room(Context &ctx, nolzss_rlz_cohort &c) {
    const uint64_t n = c.samples.size();
    if (n < c.capacity) return;
    uint64_t cap = c.capacity ? 2 * c.capacity : c.first_capacity;
    cap = cap < n + 1 ? n + 1 : cap;
    cap = cap < NOLZSS_RLZ_COHORT_MAX_SAMPLES ? cap : NOLZSS_RLZ_COHORT_MAX_SAMPLES;
    const size_t per = sample_bytes(c);
    ProfScope ps(ctx.profiler(), "rlz_cohort_grow", ctx.stream, 2.0 * (double)per * (double)n);
    c.planes.grow_keeping(ctx, per * (size_t)cap, per * (size_t)n);
    c.capacity = cap;
}

void refuse_full(const nolzss_rlz_cohort &c) {
    if (c.samples.size() >= NOLZSS_RLZ_COHORT_MAX_SAMPLES)
        throw std::invalid_argument("rlz cohort: a cohort takes at most " + std::to_string(NOLZSS_RLZ_COHORT_MAX_SAMPLES) +
                                    " samples (its two matrices stay below 2^32 bytes): open another cohort");
}

// the statistics of a packed sample into its info, and the sample into the cohort
void commit(nolzss_rlz_cohort &c, const unsigned long long stats[kCohortStats], nolzss_rlz_cohort_sample_info *info) {
    info->sample = c.samples.size();
    info->called = stats[0];
    info->low = stats[1];
    info->deleted = stats[2];
    info->differs = stats[3];
    c.samples.push_back(*info);
}

void cohort_add_pileup(nolzss_rlz_cohort *c, nolzss_rlz_pileup *p, const nolzss_rlz_consensus_params *params,
                       nolzss_rlz_cohort_sample_info *info) {
    if (!info) throw std::invalid_argument("output pointer is null");
    std::memset(info, 0, sizeof *info);
    if (!c || !p) throw std::invalid_argument("handle is null");
    const ConsensusRule rule = check_consensus_params(params);
    std::lock_guard<std::mutex> lock(c->mu);
    std::lock_guard<std::mutex> plock(p->mu);  // (the cohort's first, then the pileup's: rlz_handles.hpp)
    if (p->index != c->index || !p->index || p->index->serial != c->index_serial || p->device != c->device)
        throw std::invalid_argument("rlz cohort: the pileup is not open over the index of this cohort (index " +
                                    std::to_string(c->index_serial) + " on device " + std::to_string(c->device) + ")");
    refuse_full(*c);
    unsigned long long stats[kCohortStats] = {0, 0, 0, 0};
    if (c->B == 0) {  // no position: the device is not touched
        commit(*c, stats, info);
        return;
    }
    with_index_session(c->device, "rlz_cohort_add_pileup", [&](Context &ctx) {
        secure_room(ctx, *c);
        regrow_arena(ctx, size_t(4) << 20);  // (the tile sums of the two scans of a resolve, and the statistics)
        if (p->dirty) {  // as any read of the pileup does
            rlz_pileup_resolve(ctx, p->view);
            p->dirty = false;
        }
        unsigned long long *d_stats = ctx.arena.alloc<unsigned long long>(kCohortStats);
        rlz_cohort_pack_counts(ctx, p->view, c->index->view.text, rule, c->planes.as<uint64_t>() + 3 * c->W * c->samples.size(), d_stats);
        download_bytes(ctx, stats, d_stats, sizeof stats);
    });
    commit(*c, stats, info);
}

void cohort_add_calls(nolzss_rlz_cohort *c, const char *calls, size_t n, nolzss_rlz_cohort_sample_info *info) {
    if (!info) throw std::invalid_argument("output pointer is null");
    std::memset(info, 0, sizeof *info);
    if (!c) throw std::invalid_argument("handle is null");
    if (n != c->B)  // (the block's length never changes: read without the lock)
        throw std::invalid_argument("rlz cohort: add_calls takes one byte per block position (" + std::to_string(c->B) + "), not " +
                                    std::to_string(n));
    if (n && !calls) throw std::invalid_argument("calls pointer is null");
    std::lock_guard<std::mutex> lock(c->mu);
    refuse_full(*c);
    unsigned long long stats[kCohortStats] = {0, 0, 0, 0};
    if (c->B == 0) {
        commit(*c, stats, info);
        return;
    }
    with_index_session(c->device, "rlz_cohort_add_calls", [&](Context &ctx) {
        secure_room(ctx, *c);
        regrow_arena(ctx, n + (size_t(4) << 20));
        uint8_t *d_bytes = ctx.arena.alloc<uint8_t>(n);
        unsigned long long *d_stats = ctx.arena.alloc<unsigned long long>(kCohortStats);
        {
            ProfScope ps(ctx.profiler(), "cohort_calls_h2d", ctx.stream, (double)n);
            upload_bytes(ctx, d_bytes, calls, n);
        }
        rlz_cohort_pack_bytes(ctx, d_bytes, c->B, c->index->view.text, c->planes.as<uint64_t>() + 3 * c->W * c->samples.size(), d_stats);
        download_bytes(ctx, stats, d_stats, sizeof stats);  // (waits: the caller's bytes have gone up)
    });
    commit(*c, stats, info);
}

// NOLZSS_RLZ_COHORT_SLICE (tests; read on every call): the words of a slice of the pair kernel; 0: none named
uint32_t slice_knob() {
    if (const char *e = std::getenv("NOLZSS_RLZ_COHORT_SLICE")) {
        char *end = nullptr;
        const unsigned long long v = std::strtoull(e, &end, 10);
        if (*e && !*end && v >= 1) return (uint32_t)(v < kCohortMaxSlice ? v : kCohortMaxSlice);
    }
    return 0;
}

void cohort_distances(nolzss_rlz_cohort *c, nolzss_rlz_cohort_distances_result *out) {
    if (!out) throw std::invalid_argument("output pointer is null");
    std::memset(out, 0, sizeof *out);
    if (!c) throw std::invalid_argument("handle is null");
    std::lock_guard<std::mutex> lock(c->mu);
    const size_t N = c->samples.size(), cells = N * N;
    if (N == 0) return;
    HostBlock<uint32_t> differences = host_block<uint32_t>(cells), compared = host_block<uint32_t>(cells);
    if (c->B == 0) {
        std::memset(differences.get(), 0, sizeof(uint32_t) * cells);
        std::memset(compared.get(), 0, sizeof(uint32_t) * cells);
    } else {
        with_index_session(c->device, "rlz_cohort_distances_call", [&](Context &ctx) {
            regrow_arena(ctx, 2 * sizeof(uint32_t) * cells + (size_t(4) << 20));
            uint32_t *d_diff = ctx.arena.alloc<uint32_t>(cells), *d_cmp = ctx.arena.alloc<uint32_t>(cells);
            rlz_cohort_pairs(ctx, c->planes.as<uint64_t>(), (uint32_t)N, c->B, slice_knob(), d_diff, d_cmp);
            download_records(ctx, "cohort_distances_d2h", differences.get(), d_diff, cells, sizeof(uint32_t));
            download_records(ctx, "cohort_distances_d2h", compared.get(), d_cmp, cells, sizeof(uint32_t));
        });
    }
    out->differences = differences.release();
    out->compared = compared.release();
    out->num_samples = N;
}

void cohort_sites(nolzss_rlz_cohort *c, uint64_t min_present, int with_reference, nolzss_rlz_cohort_sites_result *out) {
    if (!out) throw std::invalid_argument("output pointer is null");
    std::memset(out, 0, sizeof *out);
    if (!c) throw std::invalid_argument("handle is null");
    std::lock_guard<std::mutex> lock(c->mu);
    const size_t N = c->samples.size();
    const uint32_t B = c->B;
    if (N == 0 || B == 0 || min_present > N) return;
    const size_t chunk_max = chunk_knob("NOLZSS_RLZ_LOCATE_CHUNK");
    HostBlock<nolzss_rlz_cohort_site> recs;
    uint64_t total = 0;  // at most B records: 32 bits hold every offset
    with_index_session(c->device, "rlz_cohort_sites_call", [&](Context &ctx) {
        const size_t most = (size_t)B < chunk_max ? (size_t)B : chunk_max;
        regrow_arena(ctx, 9 * (size_t)B + sizeof(CohortSiteRec) * most + (size_t(4) << 20));
        const PackedText &block = c->index->view.text;
        const uint64_t *d_planes = c->planes.as<uint64_t>();
        uint32_t *d_n = ctx.arena.alloc<uint32_t>(B), *d_off = ctx.arena.alloc<uint32_t>(B);
        uint64_t *d_total = ctx.arena.alloc<uint64_t>(1);
        {
            ProfScope ps(ctx.profiler(), "rlz_cohort_sites", ctx.stream, 0.375 * (double)B * (double)N + 12.0 * (double)B);
            rlz_cohort_site_flags(ctx, d_planes, (uint32_t)N, B, block, (uint32_t)min_present, with_reference != 0, d_n);
            rlz_index_rep_total(ctx, d_n, B, d_total);
            scan_exclusive_add_u32(d_n, d_off, B, nullptr, ctx.arena, ctx.stream);
            download_bytes(ctx, &total, d_total, sizeof total);
        }
        total = total < B ? total : B;
        if (total == 0) return;
        recs = host_block<nolzss_rlz_cohort_site>((size_t)total);
        const size_t chunk = total < chunk_max ? (size_t)total : chunk_max;
        CohortSiteRec *d_stage = ctx.arena.alloc<CohortSiteRec>(chunk);
        download_produced(ctx, "cohort_sites_d2h", recs.get(), d_stage, (size_t)total, sizeof(CohortSiteRec), chunk,
                          [&](size_t c0, size_t cnt) {
                              rlz_cohort_site_records(ctx, d_planes, (uint32_t)N, B, block, d_n, d_off, c0, (uint32_t)cnt, d_stage);
                          });
    });
    out->num_sites = (size_t)total;  // (the result stays zeroed up to here: a throw above frees the block)
    out->sites = recs.release();
}

void cohort_columns(nolzss_rlz_cohort *c, const uint64_t *positions, size_t S, char *out) {
    if (!c) throw std::invalid_argument("handle is null");
    if (S && !positions) throw std::invalid_argument("positions pointer is null");
    if (S > 0xffffffffull) throw std::invalid_argument("rlz cohort: columns take fewer than 2^32 positions");
    std::vector<uint32_t> pos(S);
    for (size_t k = 0; k < S; ++k) {
        if (positions[k] >= c->B)  // (the block's length never changes: read without the lock)
            throw std::invalid_argument("rlz cohort: position " + std::to_string(positions[k]) + " (entry " + std::to_string(k) +
                                        ") lies at or beyond the block's length " + std::to_string(c->B));
        pos[k] = (uint32_t)positions[k];
    }
    std::lock_guard<std::mutex> lock(c->mu);
    const size_t N = c->samples.size(), total = N * S;
    if (total == 0) return;
    if (!out) throw std::invalid_argument("output pointer is null");
    const size_t chunk_max = chunk_knob("NOLZSS_RLZ_LOCATE_CHUNK");
    const size_t chunk = total < chunk_max ? total : chunk_max;
    with_index_session(c->device, "rlz_cohort_columns_call", [&](Context &ctx) {
        regrow_arena(ctx, sizeof(uint32_t) * S + chunk + (size_t(4) << 20));
        uint32_t *d_pos = ctx.arena.alloc<uint32_t>(S);
        uint8_t *d_stage = ctx.arena.alloc<uint8_t>(chunk);
        upload_bytes(ctx, d_pos, pos.data(), sizeof(uint32_t) * S);
        download_produced(ctx, "cohort_columns_d2h", out, d_stage, total, 1, chunk, [&](size_t c0, size_t cnt) {
            rlz_cohort_columns(ctx, c->planes.as<uint64_t>(), (uint32_t)N, c->B, d_pos, S, c0, (uint32_t)cnt, d_stage);
        });
    });
}

void cohort_calls(nolzss_rlz_cohort *c, uint64_t sample, uint64_t start, uint64_t end, char *out) {
    if (!c) throw std::invalid_argument("handle is null");
    if (start > end || end > c->B)
        throw std::invalid_argument("rlz cohort: calls take 0 <= start <= end <= block length (" + std::to_string(c->B) + "), not [" +
                                    std::to_string(start) + ", " + std::to_string(end) + ")");
    std::lock_guard<std::mutex> lock(c->mu);
    if (sample >= c->samples.size())
        throw std::invalid_argument("rlz cohort: sample " + std::to_string(sample) + " of " + std::to_string(c->samples.size()));
    const size_t count = (size_t)(end - start);
    if (count == 0) return;
    if (!out) throw std::invalid_argument("output pointer is null");
    const size_t chunk_max = chunk_knob("NOLZSS_RLZ_LOCATE_CHUNK");
    const size_t chunk = count < chunk_max ? count : chunk_max;
    with_index_session(c->device, "rlz_cohort_calls_call", [&](Context &ctx) {
        regrow_arena(ctx, chunk + (size_t(4) << 20));
        uint8_t *d_stage = ctx.arena.alloc<uint8_t>(chunk);
        const uint64_t *d_sample = c->planes.as<uint64_t>() + 3 * c->W * (size_t)sample;
        download_produced(ctx, "cohort_calls_d2h", out, d_stage, count, 1, chunk, [&](size_t c0, size_t cnt) {
            rlz_cohort_calls(ctx, d_sample, c->B, (uint32_t)(start + c0), (uint32_t)cnt, d_stage);
        });
    });
}

}  // namespace

extern "C" {

int nolzss_rlz_cohort_open(const nolzss_rlz_index *index, nolzss_rlz_cohort **out) {
    return guarded([&] { cohort_open(index, out); });
}

int nolzss_rlz_cohort_add_pileup(nolzss_rlz_cohort *c, nolzss_rlz_pileup *p, const nolzss_rlz_consensus_params *params,
                                 nolzss_rlz_cohort_sample_info *info) {
    return guarded([&] { cohort_add_pileup(c, p, params, info); });
}

int nolzss_rlz_cohort_add_calls(nolzss_rlz_cohort *c, const char *calls, size_t n, nolzss_rlz_cohort_sample_info *info) {
    return guarded([&] { cohort_add_calls(c, calls, n, info); });
}

int nolzss_rlz_cohort_info(nolzss_rlz_cohort *c, nolzss_rlz_cohort_summary *info) {
    return guarded([&] {
        if (!c || !info) throw std::invalid_argument("handle or output pointer is null");
        std::memset(info, 0, sizeof *info);
        std::lock_guard<std::mutex> lock(c->mu);
        info->samples = c->samples.size();
        info->capacity = c->capacity;
        info->block_length = c->B;
        info->device_bytes = c->planes.bytes();
        info->device = c->device;
    });
}

int nolzss_rlz_cohort_samples(nolzss_rlz_cohort *c, nolzss_rlz_cohort_sample_info *out, size_t capacity, size_t *count) {
    return guarded([&] {
        if (!c || !count || (capacity && !out)) throw std::invalid_argument("handle or output pointer is null");
        std::lock_guard<std::mutex> lock(c->mu);
        *count = c->samples.size();
        const size_t take = *count < capacity ? *count : capacity;
        if (take) std::memcpy(out, c->samples.data(), sizeof(nolzss_rlz_cohort_sample_info) * take);
    });
}

int nolzss_rlz_cohort_distances(nolzss_rlz_cohort *c, nolzss_rlz_cohort_distances_result *out) {
    return guarded([&] { cohort_distances(c, out); });
}

void nolzss_free_rlz_cohort_distances_result(nolzss_rlz_cohort_distances_result *r) {
    if (!r) return;
    free_block(r->differences);
    free_block(r->compared);
    std::memset(r, 0, sizeof *r);
}

int nolzss_rlz_cohort_sites(nolzss_rlz_cohort *c, uint64_t min_present, int with_reference, nolzss_rlz_cohort_sites_result *out) {
    return guarded([&] { cohort_sites(c, min_present, with_reference, out); });
}

void nolzss_free_rlz_cohort_sites_result(nolzss_rlz_cohort_sites_result *r) {
    if (!r) return;
    free_block(r->sites);
    std::memset(r, 0, sizeof *r);
}

int nolzss_rlz_cohort_columns(nolzss_rlz_cohort *c, const uint64_t *positions, size_t S, char *out) {
    return guarded([&] { cohort_columns(c, positions, S, out); });
}

int nolzss_rlz_cohort_calls(nolzss_rlz_cohort *c, uint64_t sample, uint64_t start, uint64_t end, char *out) {
    return guarded([&] { cohort_calls(c, sample, start, end, out); });
}

int nolzss_rlz_cohort_close(nolzss_rlz_cohort *c) {
    return guarded([&] { delete c; });
}

}  // extern "C"
