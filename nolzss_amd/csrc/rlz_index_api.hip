// rlz_index_api.hip -- the relative-LZ index handle and its entry points: the references in, their suffix structures
// kept in one device allocation of the handle's own, target batches matched against them (part of the C ABI layer of
// libnolzss_hip.so, include/nolzss_hip.h, nolzss_rlz_index_*; the kernels: rlz_index.hip; DESIGN.md 5, "Relative-LZ
// index: targets matched against a resident reference").  Also what every query on the handle is built from: the batch
// searched, the arena grown for a total learnt on the device, chunked downloads and the session of a call
// (rlz_handles.hpp).  The pattern queries: rlz_index_query_api.hip; the seed queries: rlz_index_seeds_api.hip; the
// archive over an index: rlz_archive_api.hip.
#include "rlz_handles.hpp"

using namespace nolzss;
using namespace nolzss::api;

uint32_t nolzss::api::choose_prefix(size_t index_length) {  // clamp(floor(log4 |X|) - 1, 4, 12)
    int l = 0;
    while ((index_length >> (2 * (l + 1))) != 0) ++l;
    const int P = l - 1;
    return (uint32_t)(P < 4 ? 4 : (P > (int)kIndexMaxPrefix ? (int)kIndexMaxPrefix : P));
}

void nolzss::api::prepare_batch(const nolzss_rlz_index &h, const char *const *targets, const size_t *target_lens, size_t k,
                                Batch &b) {
    if (k && (!targets || !target_lens)) throw std::invalid_argument("sequence array is null");
    size_t bases = 0;
    bool overflow = false;
    for (size_t j = 0; j < k; ++j) {
        if (target_lens[j] && !targets[j]) throw std::invalid_argument("sequence pointer is null");
        overflow |= bases + target_lens[j] < bases;
        bases += target_lens[j];
    }
    const size_t B = h.view.B;
    if (overflow || bases > kMaxText || k > kMaxText || B + 1 + bases + k > kMaxText)
        throw std::invalid_argument("text too long: the device pipeline uses 32-bit indices");
    for (size_t j = 0; j < k; ++j) {
        const size_t bad = first_invalid_nucleotide(targets[j], target_lens[j]);
        if (bad < target_lens[j])
            throw std::runtime_error("Invalid nucleotide '" + std::string(1, targets[j][bad]) + "' found in sequence " +
                                     std::to_string(h.m + j));
    }
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
}

uint8_t *nolzss::api::upload_and_pack(Context &ctx, const Batch &b, PackedText &packed) {
    const size_t n = b.tcat.size();
    uint8_t *d_T = ctx.arena.alloc<uint8_t>(n);
    {
        ProfScope ps(ctx.profiler(), "text_h2d", ctx.stream, (double)n);
        upload_bytes(ctx, d_T, b.tcat.data(), n);
    }
    if (!pack_independent_text(ctx, d_T, n, b.separators, packed))
        throw std::runtime_error("rlz index: the batch holds bytes that are neither bases nor its separators");
    return d_T;
}

Searched nolzss::api::search_batch(Context &ctx, const nolzss_rlz_index &h, const Batch &b) {
    const size_t n = b.tcat.size();
    Searched m;
    m.d_T = upload_and_pack(ctx, b, m.batch);
    m.d_len = ctx.arena.alloc<uint32_t>(n);
    m.d_rank = ctx.arena.alloc<uint32_t>(n);
    rlz_index_search(ctx, h.view, m.batch, m.d_len, m.d_rank);
    return m;
}

// The two-reservation rule of every query that learns a total on the device: it reserves for its batch, runs its front
// end, and reserves again for what the total takes.  A reservation that is not a no-op may replace the slab (and the new
// one may be as large as the old), so the arena is then emptied and the caller runs its front end again in it.
bool nolzss::api::regrow_arena(Context &ctx, size_t extra) {
    if (arena_bytes_for(0) + extra <= ctx.arena.capacity()) return false;
    HIP_CHECK(hipStreamSynchronize(ctx.stream));  // (nothing still reads the slab that goes)
    reserve_arena_for(ctx, 0, extra);
    ctx.arena.rewind(0);
    return true;
}

void nolzss::api::download_records(Context &ctx, const char *scope, void *h_dst, const void *d_src, size_t count, size_t size) {
    const size_t chunk_max = chunk_knob("NOLZSS_RLZ_LOCATE_CHUNK");
    for (size_t c0 = 0; c0 < count; c0 += chunk_max) {
        const size_t c = count - c0 < chunk_max ? count - c0 : chunk_max;
        ProfScope ps(ctx.profiler(), scope, ctx.stream, (double)(size * c));
        download_bytes(ctx, static_cast<char *>(h_dst) + c0 * size, static_cast<const char *>(d_src) + c0 * size, c * size);
    }
}

void nolzss::api::download_produced(Context &ctx, const char *scope, void *h_dst, const void *d_stage, size_t count, size_t size,
                                    size_t chunk, const std::function<void(size_t, size_t)> &produce) {
    for (size_t c0 = 0; c0 < count; c0 += chunk) {
        const size_t c = count - c0 < chunk ? count - c0 : chunk;
        produce(c0, c);
        ProfScope ps(ctx.profiler(), scope, ctx.stream, (double)(size * c));
        download_bytes(ctx, static_cast<char *>(h_dst) + c0 * size, d_stage, c * size);  // (waits: d_stage is free again)
    }
}

void nolzss::api::with_index_session(int device, const char *scope, const std::function<void(Context &)> &f) {
    DeviceRestore restore;
    Session ses(device, nullptr);
    Context &ctx = ses.ctx();
    {
        ProfScope whole(ctx.profiler(), scope, ctx.stream);
        f(ctx);
    }
    HIP_CHECK(hipStreamSynchronize(ctx.stream));
    HIP_CHECK(hipGetLastError());
    ctx.prof.collect();
}

namespace {

void open_index(const char *const *refs, const size_t *ref_lens, size_t m, bool with_rc, uint32_t prefix_syms, int device,
                nolzss_rlz_index **out) {
    if (!out) throw std::invalid_argument("output pointer is null");
    *out = nullptr;
    if (prefix_syms > kIndexMaxPrefix) throw std::invalid_argument("prefix_syms must be 0 (choose) or 1 .. 12");
    RlzPrepared p;  // X and every refusal of the reference side, before any device is touched
    rlz_prepare(refs, ref_lens, m, nullptr, nullptr, 0, with_rc, p);
    const size_t total = p.S.size();
    const uint32_t P = prefix_syms ? prefix_syms : choose_prefix(total);

    static std::atomic<uint64_t> serials{0};
    std::unique_ptr<nolzss_rlz_index> h(new nolzss_rlz_index);
    h->device = device;
    h->m = m;
    h->serial = ++serials;  // (never 0: an archive with serial 0 was not opened over an index)
    DeviceRestore restore;
    Session ses(device, nullptr);
    Context &ctx = ses.ctx();
    {
        ProfScope whole(ctx.profiler(), "rlz_index_open", ctx.stream);
        reserve_arena_for(ctx, total, total + 4 * ((size_t(1) << (2 * P)) + 1));
        uint8_t *d_X = ctx.arena.alloc<uint8_t>(total);
        {
            ProfScope ps(ctx.profiler(), "text_h2d", ctx.stream);
            upload_bytes(ctx, d_X, p.S.data(), total);
        }
        const RlzIndexView built = rlz_index_build(ctx, d_X, (uint32_t)total, p.lay.block_length, with_rc, P);
        h->base.alloc(ctx, rlz_index_footprint(built));
        h->view = rlz_index_copy_into(ctx, built, h->base.get());
    }
    HIP_CHECK(hipStreamSynchronize(ctx.stream));
    ctx.prof.collect();
    // the sort's arena goes back to the driver: what stays resident is the handle, and a match reserves its own
    ctx.arena.release();
    *out = h.release();
}

struct MatchOut {
    std::vector<size_t> counts, first;  // per target: records, and the index of its first record in block
    FactorBlock block;
};

// One batch against the handle (k >= 1).  h_codes: the codes of every position and nothing else.  Otherwise the chain;
// want_factors: every record comes down (the separator literals with them) and is split by searching the ascending
// starts, else the starts are counted per target on the device and only the k counts cross PCIe.
void match_batch(const nolzss_rlz_index &h, const Batch &b, const size_t *target_lens, size_t k, bool want_factors,
                 uint32_t *h_codes, MatchOut &out) {
    const size_t n = b.tcat.size();
    const uint64_t base = (uint64_t)h.view.B + 1;
    DeviceRestore restore;
    Session ses(h.device, nullptr);
    Context &ctx = ses.ctx();
    hipStream_t s = ctx.stream;
    reserve_arena_for(ctx, 0, kBatchBytesPerPosition * n + 12 * k + sizeof(IndexRec) * kRecordChunk + (size_t(4) << 20));
    const Searched m = search_batch(ctx, h, b);
    uint32_t *d_len = m.d_len, *d_rank = m.d_rank;
    if (h_codes) {
        rlz_index_strands(ctx, h.view, (uint32_t)n, d_len, d_rank);
        download_bytes(ctx, h_codes, d_len, n * sizeof(uint32_t));
        ctx.prof.collect();
        return;
    }
    // the chain and its factor starts: they read the codes and nothing else (chain.hip)
    const Chain chain = mark_chain(ctx, (uint32_t)n, 0u, LstarCodes::of(d_len));
    const uint32_t z = chain.z;
    const uint32_t *d_fpos = chain_starts(ctx, chain);
    if (want_factors) {
        out.block.reset(static_cast<nolzss_factor *>(alloc_factor_block(sizeof(nolzss_factor) * (z ? z : 1))));
        if (!out.block) throw std::bad_alloc();
        const size_t chunk = z < kRecordChunk ? z : kRecordChunk;
        IndexRec *d_recs = ctx.arena.alloc<IndexRec>(chunk ? chunk : 1);
        download_produced(ctx, "factors_d2h", out.block.get(), d_recs, z, sizeof(IndexRec), chunk, [&](size_t c0, size_t cnt) {
            rlz_index_records(ctx, h.view, d_fpos + c0, (uint32_t)cnt, d_len, d_rank, d_recs);
        });
        HIP_CHECK(hipStreamSynchronize(s));
        const nolzss_factor *f = out.block.get();
        auto first_at = [&](uint64_t pos) {
            return (size_t)(std::lower_bound(f, f + z, pos, [](const nolzss_factor &a, uint64_t x) { return a.start < x; }) - f);
        };
        for (size_t j = 0; j < k; ++j) {
            out.first[j] = first_at(base + b.offsets[j]);
            out.counts[j] = first_at(base + b.offsets[j] + target_lens[j]) - out.first[j];
        }
    } else if (z) {
        std::vector<uint32_t> bounds(2 * k), counts(k);
        for (size_t j = 0; j < k; ++j) {
            bounds[2 * j] = (uint32_t)b.offsets[j];
            bounds[2 * j + 1] = (uint32_t)(b.offsets[j] + target_lens[j]);
        }
        uint32_t *d_bounds = ctx.arena.alloc<uint32_t>(2 * k), *d_counts = ctx.arena.alloc<uint32_t>(k);
        HIP_CHECK(hipMemcpyAsync(d_bounds, bounds.data(), bounds.size() * sizeof(uint32_t), hipMemcpyHostToDevice, s));
        rlz_count_per_target(ctx, d_fpos, z, d_bounds, (uint32_t)k, d_counts);
        HIP_CHECK(hipMemcpyAsync(counts.data(), d_counts, k * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipStreamSynchronize(s));  // (bounds and counts are local vectors)
        for (size_t j = 0; j < k; ++j) out.counts[j] = counts[j];
    }
    HIP_CHECK(hipStreamSynchronize(s));
    ctx.prof.collect();
}

void index_factorize(const nolzss_rlz_index &h, const char *const *targets, const size_t *target_lens, size_t k,
                     bool want_factors, nolzss_rlz_result *out) {
    Batch b;
    prepare_batch(h, targets, target_lens, k, b);
    MatchOut run;
    run.counts.assign(k, 0);
    run.first.assign(k, 0);
    if (k) match_batch(h, b, target_lens, k, want_factors, nullptr, run);
    nolzss_rlz_result res;
    std::memset(&res, 0, sizeof res);
    try {
        res.num_targets = k;
        res.block_length = h.view.B;
        res.target_offsets = calloc_array<uint64_t>(k);
        res.target_lengths = calloc_array<uint64_t>(k);
        res.counts = calloc_array<size_t>(k);
        if (want_factors) res.factors = calloc_array<nolzss_factor *>(k);
        for (size_t j = 0; j < k; ++j) {
            res.target_offsets[j] = (uint64_t)h.view.B + 1 + b.offsets[j];
            res.target_lengths[j] = target_lens[j];
            res.counts[j] = run.counts[j];
            if (want_factors) res.factors[j] = run.block ? run.block.get() + run.first[j] : nullptr;
        }
    } catch (...) {
        nolzss_free_rlz_result(&res);
        throw;
    }
    res.block = run.block.release();  // ownership moves to the caller
    *out = res;
}

}  // namespace

extern "C" {

int nolzss_rlz_index_open(const char *const *refs, const size_t *ref_lens, size_t m, int with_rc, uint32_t prefix_syms,
                          int device, nolzss_rlz_index **h) {
    return guarded([&] { open_index(refs, ref_lens, m, with_rc != 0, prefix_syms, device, h); });
}

int nolzss_rlz_index_open_fasta(const char *reference_fasta_path, int with_rc, int sanitize_mode, uint32_t prefix_syms,
                                int device, nolzss_rlz_index **h) {
    return guarded([&] {
        if (!h) throw std::invalid_argument("output pointer is null");
        *h = nullptr;
        if (sanitize_mode != 0 && sanitize_mode != 1) throw std::invalid_argument("sanitize_mode must be 0 or 1");
        const FastaParse ref = parse_fasta(reference_fasta_path, sanitize_mode == 1);
        std::vector<const char *> ptrs;
        std::vector<size_t> lens;
        for (const auto &q : ref.sequences) {
            ptrs.push_back(q.data());
            lens.push_back(q.size());
        }
        open_index(ptrs.data(), lens.data(), ptrs.size(), with_rc != 0, prefix_syms, device, h);
    });
}

int nolzss_rlz_index_info(const nolzss_rlz_index *h, nolzss_rlz_index_summary *info) {
    return guarded([&] {
        if (!h || !info) throw std::invalid_argument("handle or output pointer is null");
        std::memset(info, 0, sizeof *info);
        info->num_references = h->m;
        info->block_length = h->view.B;
        info->index_length = h->view.text.n;
        info->with_rc = h->view.with_rc ? 1 : 0;
        info->device = h->device;
        info->prefix_syms = h->view.P;
        info->device_bytes = h->base.bytes();
    });
}

int nolzss_rlz_index_factorize(const nolzss_rlz_index *h, const char *const *targets, const size_t *target_lens, size_t k,
                               int want_factors, nolzss_rlz_result *out) {
    return guarded([&] {
        if (!out) throw std::invalid_argument("output pointer is null");
        std::memset(out, 0, sizeof *out);
        if (!h) throw std::invalid_argument("handle is null");
        index_factorize(*h, targets, target_lens, k, want_factors != 0, out);
    });
}

int nolzss_rlz_index_codes(const nolzss_rlz_index *h, const char *const *targets, const size_t *target_lens, size_t k,
                           uint32_t *code) {
    return guarded([&] {
        if (!h) throw std::invalid_argument("handle is null");
        Batch b;
        prepare_batch(*h, targets, target_lens, k, b);
        if (k == 0) return;
        if (!code) throw std::invalid_argument("output pointer is null");
        MatchOut run;
        match_batch(*h, b, target_lens, k, false, code, run);
    });
}

int nolzss_rlz_index_close(nolzss_rlz_index *h) {
    return guarded([&] { delete h; });
}

}  // extern "C"
