// rlz_index_api.hip -- the relative-LZ index handle and its entry points: the references in, their suffix structures
// kept in one device allocation of the handle's own, target batches matched against them (part of the C ABI layer of
// libnolzss_hip.so, include/nolzss_hip.h, nolzss_rlz_index_*; the kernels: rlz_index.hip; DESIGN.md 5, "Relative-LZ
// index: targets matched against a resident reference").  Also nolzss_rlz_archive_open_index / _append_index: the
// archive opened over an index and the batches appended to it on the device, which run the same match (DESIGN.md 5,
// "Relative-LZ archive: batches appended from the index"), and nolzss_rlz_index_count / _locate: pattern batches
// queried against the handle (the kernels: rlz_locate.hip; DESIGN.md 5, "Relative-LZ index: pattern count and locate"),
// and nolzss_rlz_index_seeds: the maximal exact matches of a target batch and their occurrences (the kernels:
// rlz_seeds.hip; DESIGN.md 5, "Relative-LZ index: maximal match seeds"), and nolzss_rlz_index_seed_chains: the seeds of
// every target chained into placements on the device (the kernels: rlz_seed_chain.hip; DESIGN.md 5, "Relative-LZ index:
// colinear seed chains"), and nolzss_rlz_index_align: every such chain aligned base by base on the device (the kernels:
// rlz_align.hip; DESIGN.md 5, "Relative-LZ index: base-level alignments").
#include "rlz_handles.hpp"

using namespace nolzss;
using namespace nolzss::api;

namespace {

// device memory per batch position: packed text 1/4, code 4, rank 4, the chain's exits, bitmaps and node lists (12 on
// ordinary batches, 24 when every position is a node), the factor starts 4 -- not the 52 of a suffix sort
constexpr size_t kBatchBytesPerPosition = 36;

}  // namespace
uint32_t nolzss::api::choose_prefix(size_t index_length) {  // clamp(floor(log4 |X|) - 1, 4, 12)
    int l = 0;
    while ((index_length >> (2 * (l + 1))) != 0) ++l;
    const int P = l - 1;
    return (uint32_t)(P < 4 ? 4 : (P > (int)kIndexMaxPrefix ? (int)kIndexMaxPrefix : P));
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
        h->device_bytes = rlz_index_footprint(built);
        h->d_base = device_alloc(ctx, h->device_bytes);
        h->view = rlz_index_copy_into(ctx, built, h->d_base);
    }
    HIP_CHECK(hipStreamSynchronize(ctx.stream));
    ctx.prof.collect();
    // the sort's arena goes back to the driver: what stays resident is the handle, and a match reserves its own
    ctx.arena.release();
    *out = h.release();
}

// every check of a match, in the order the header states them, and the batch laid out
void prepare_batch(const nolzss_rlz_index &h, const char *const *targets, const size_t *target_lens, size_t k, Batch &b) {
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

}  // namespace

// (prepare_patterns, chunk_knob and pattern_batch_bytes are shared with the finder's queries, rlz_find_api.hip:
// rlz_handles.hpp declares them)
// The checks of a pattern batch -- the length rule first, decided by the lengths alone, then the bases, as the header
// states -- and the batch laid out as a target batch is.  A batch holds millions of short patterns: they are validated
// and upper-cased in one pass over the batch, split between the host threads by position (every pattern is followed by
// its separator, so the offsets ascend strictly), not one helper call per pattern.
void nolzss::api::prepare_patterns(const char *const *patterns, const size_t *pattern_lens, size_t q, Batch &b) {
    if (q && (!patterns || !pattern_lens)) throw std::invalid_argument("pattern array is null");
    size_t bases = 0;
    bool overflow = false;
    for (size_t j = 0; j < q; ++j) {
        if (pattern_lens[j] && !patterns[j]) throw std::invalid_argument("pattern pointer is null");
        overflow |= bases + pattern_lens[j] < bases;
        bases += pattern_lens[j];
    }
    if (overflow || bases > kMaxText || q > kMaxText || bases + q > kMaxText)
        throw std::invalid_argument("pattern batch too long: sum(len) + q is beyond the " + std::to_string(kMaxText) +
                                    " positions the 32-bit device pipeline takes");
    b.tcat.resize(bases + q);
    b.separators.resize(q);
    b.offsets.resize(q);
    size_t at = 0;
    for (size_t j = 0; j < q; ++j) {
        b.offsets[j] = at;
        at += pattern_lens[j];
        b.separators[j] = (uint32_t)at++;
    }
    std::atomic<size_t> first_bad{q};
    host_parallel(bases + q, [&](size_t lo, size_t hi) {  // the patterns that start in [lo, hi)
        size_t j = (size_t)(std::lower_bound(b.offsets.begin(), b.offsets.end(), (uint64_t)lo) - b.offsets.begin());
        for (; j < q && b.offsets[j] < hi; ++j) {
            uint8_t *dst = b.tcat.data() + b.offsets[j];
            const char *src = patterns[j];
            const size_t len = pattern_lens[j];
            bool bad = false;
            for (size_t i = 0; i < len; ++i) {  // [ACGTacgt] and nothing else folds onto ACGT
                const uint8_t c = (uint8_t)src[i] & 0xdfu;
                bad |= c != 'A' && c != 'C' && c != 'G' && c != 'T';
                dst[i] = c;
            }
            dst[len] = kSeparator;
            if (bad) {
                size_t cur = first_bad.load();
                while (j < cur && !first_bad.compare_exchange_weak(cur, j)) {
                }
            }
        }
    });
    const size_t j = first_bad.load();
    if (j < q) {
        const size_t bad = first_invalid_nucleotide(patterns[j], pattern_lens[j]);
        throw std::runtime_error("Invalid nucleotide '" + std::string(1, patterns[j][bad]) + "' found in pattern " +
                                 std::to_string(j));
    }
}

namespace {

struct MatchOut {
    std::vector<size_t> counts, first;  // per target: records, and the index of its first record in block
    FactorBlock block;
};

// What every use of a match starts with: the batch up, packed with the target ends as terminators, and searched.
struct Searched {
    uint8_t *d_T;              // the batch bytes (upper case, separators)
    uint32_t *d_len, *d_rank;  // per position: the longest match and a rank that attains it
    PackedText batch;          // the packed batch: its terminator table holds the target ends
};

Searched search_batch(Context &ctx, const nolzss_rlz_index &h, const Batch &b) {
    const size_t n = b.tcat.size();
    Searched m;
    m.d_T = ctx.arena.alloc<uint8_t>(n);
    {
        ProfScope ps(ctx.profiler(), "text_h2d", ctx.stream, (double)n);
        upload_bytes(ctx, m.d_T, b.tcat.data(), n);
    }
    if (!pack_independent_text(ctx, m.d_T, n, b.separators, m.batch))
        throw std::runtime_error("rlz index: the batch holds bytes that are neither bases nor its separators");
    m.d_len = ctx.arena.alloc<uint32_t>(n);
    m.d_rank = ctx.arena.alloc<uint32_t>(n);
    rlz_index_search(ctx, h.view, m.batch, m.d_len, m.d_rank);
    return m;
}

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
        for (size_t c0 = 0; c0 < z; c0 += chunk) {
            const size_t cnt = z - c0 < chunk ? z - c0 : chunk;
            rlz_index_records(ctx, h.view, d_fpos + c0, (uint32_t)cnt, d_len, d_rank, d_recs);
            ProfScope ps(ctx.profiler(), "factors_d2h", s, (double)(sizeof(IndexRec) * cnt));
            download_bytes(ctx, out.block.get() + c0, d_recs, sizeof(IndexRec) * cnt);  // (waits: d_recs is free again)
        }
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

// ---- the archive over an index: open, and batches appended on the device -------------------------------------------
void archive_open_index(const nolzss_rlz_index &ix, nolzss_rlz_archive **out) {
    if (!out) throw std::invalid_argument("output pointer is null");
    *out = nullptr;
    std::unique_ptr<nolzss_rlz_archive> h(new nolzss_rlz_archive);
    h->device = ix.device;
    h->block_len = ix.view.B;
    h->index_serial = ix.serial;
    h->bases.assign(1, 0);
    DeviceRestore restore;
    Session ses(ix.device, nullptr);
    Context &ctx = ses.ctx();
    {
        ProfScope whole(ctx.profiler(), "rlz_archive_open_index", ctx.stream);
        const size_t block_bytes = ix.view.B ? ix.view.B : 1;
        h->d_block = static_cast<uint8_t *>(device_alloc(ctx, block_bytes));
        h->device_bytes = block_bytes;
        archive_unpack_block(ctx, ix.view.text, ix.view.B, h->d_block);
    }
    HIP_CHECK(hipStreamSynchronize(ctx.stream));
    ctx.prof.collect();
    *out = h.release();
}

}  // namespace

// NOLZSS_RLZ_APPEND_CHUNK: records per look-up chunk of an append; NOLZSS_RLZ_LOCATE_CHUNK: hit records per download
// chunk of a locate (test knobs, read on every call)
size_t nolzss::api::chunk_knob(const char *name) {
    const char *e = std::getenv(name);
    if (!e || !*e) return kRecordChunk;
    char *end = nullptr;
    const unsigned long long v = std::strtoull(e, &end, 10);
    if (*end || v == 0) return kRecordChunk;
    return v < kRecordChunk ? (size_t)v : kRecordChunk;
}

namespace {

// a device array that replaces one of the handle's: freed on the way out unless it was swapped in (then the old one is)
struct Fresh {
    void *p = nullptr;
    ~Fresh() {
        if (p) (void)hipFree(p);
    }
};

void fill_append_info(const nolzss_rlz_archive &a, nolzss_rlz_archive_append_info *info, uint64_t targets, uint64_t records,
                      uint64_t literals, uint64_t bases, bool reallocated) {
    if (!info) return;
    std::memset(info, 0, sizeof *info);
    info->targets_added = targets;
    info->records_added = records;
    info->literals_added = literals;
    info->bases_added = bases;
    info->num_targets = a.lengths.size();
    info->z = a.z;
    info->total_length = a.decoded;
    info->capacity_records = a.cap_recs;
    info->device_bytes = a.device_bytes;
    info->reallocated = reallocated ? 1 : 0;
}

void archive_append(nolzss_rlz_archive &a, const nolzss_rlz_index &ix, const char *const *targets, const size_t *target_lens,
                    size_t k, nolzss_rlz_archive_append_info *info) {
    if (!a.index_serial)
        throw std::invalid_argument("rlz archive: append takes an archive opened by nolzss_rlz_archive_open_index");
    if (a.index_serial != ix.serial || a.device != ix.device)
        throw std::invalid_argument("rlz archive: the archive is bound to another index (it was opened over index " +
                                    std::to_string(a.index_serial) + " on device " + std::to_string(a.device) +
                                    ", this is index " + std::to_string(ix.serial) + " on device " + std::to_string(ix.device) + ")");
    if (k && targets && target_lens) {  // the lengths alone decide: no target byte is read before this
        uint64_t sum = 0;
        bool overflow = false;
        for (size_t j = 0; j < k; ++j) {
            overflow |= sum + target_lens[j] < sum;
            sum += target_lens[j];
        }
        if (!overflow && sum <= kMaxText && a.decoded + sum > kMaxText)
            throw std::invalid_argument("rlz archive: decoded length: the archive holds " + std::to_string(a.decoded) +
                                        " bytes and the batch " + std::to_string(sum) + ", together beyond the " +
                                        std::to_string(kMaxText) + " positions the 32-bit device pipeline takes");
    }
    Batch b;
    prepare_batch(ix, targets, target_lens, k, b);
    if (k == 0) {
        fill_append_info(a, info, 0, 0, 0, 0, false);
        return;
    }
    const size_t n = b.tcat.size();
    const uint64_t bases = n - k, base = (uint64_t)ix.view.B + 1;
    a.lengths.reserve(a.lengths.size() + k);  // (the commit below cannot fail)
    a.bases.reserve(a.bases.size() + k);
    const size_t chunk_max = chunk_knob("NOLZSS_RLZ_APPEND_CHUNK");

    DeviceRestore restore;
    Fresh fresh_recs, fresh_sample;  // (freed while the handle's device is still current)
    ArchiveRec *recs = a.d_recs;
    uint32_t *sample = a.d_sample;
    size_t cap_recs = a.cap_recs, cap_samples = a.cap_samples;
    uint64_t z_new = 0, added = 0, lit_added = 0;
    const uint64_t decoded_new = a.decoded + bases;
    const size_t samples_old = archive_samples((size_t)a.decoded), samples_new = archive_samples((size_t)decoded_new);

    Session ses(ix.device, nullptr);
    Context &ctx = ses.ctx();
    hipStream_t s = ctx.stream;
    std::vector<uint32_t> lit_counts;
    try {
        ProfScope whole(ctx.profiler(), "rlz_archive_append", s);
        reserve_arena_for(ctx, 0, (kBatchBytesPerPosition + 2) * n + 16 * k + sizeof(IndexRec) * (chunk_max < n ? chunk_max : n) +
                                      (size_t(4) << 20));
        const Searched m = search_batch(ctx, ix, b);
        const uint8_t *d_T = m.d_T;
        uint32_t *d_len = m.d_len, *d_rank = m.d_rank;
        const Chain chain = mark_chain(ctx, (uint32_t)n, 0u, LstarCodes::of(d_len));
        const uint32_t zb = chain.z;
        const uint32_t *d_fpos = chain_starts(ctx, chain);
        if (zb < k) throw HipError("rlz archive: the chain of a batch holds fewer factor starts than separators");
        added = zb - k;  // every separator is a factor start of its own
        z_new = a.z + added;
        if (z_new > 0xffffffffull)
            throw std::invalid_argument("rlz archive: z: the archive holds " + std::to_string(a.z) + " records and the batch " +
                                        std::to_string(added) + ", the position sample indexes records in 32 bits, 2^32 or "
                                        "more are refused");
        // growth: max(needed, 2 x current), the old contents copied on the stream; the old array is freed at the commit
        if (z_new > cap_recs) {
            cap_recs = std::max<size_t>((size_t)z_new, 2 * cap_recs);
            fresh_recs.p = device_alloc(ctx, sizeof(ArchiveRec) * cap_recs);
            recs = static_cast<ArchiveRec *>(fresh_recs.p);
            if (a.z) HIP_CHECK(hipMemcpyAsync(recs, a.d_recs, sizeof(ArchiveRec) * a.z, hipMemcpyDeviceToDevice, s));
        }
        if (samples_new > cap_samples) {
            cap_samples = std::max<size_t>(samples_new, 2 * cap_samples);
            fresh_sample.p = device_alloc(ctx, sizeof(uint32_t) * cap_samples);
            sample = static_cast<uint32_t *>(fresh_sample.p);
            if (samples_old)
                HIP_CHECK(hipMemcpyAsync(sample, a.d_sample, sizeof(uint32_t) * samples_old, hipMemcpyDeviceToDevice, s));
        }
        uint32_t *d_seps = ctx.arena.alloc<uint32_t>(k);
        upload_bytes(ctx, d_seps, b.separators.data(), sizeof(uint32_t) * k);
        const AppendBatch ab{d_T, d_seps, (uint32_t)n, (uint32_t)k, (uint32_t)a.z, (uint32_t)a.decoded, (uint32_t)z_new};
        const size_t chunk = zb < chunk_max ? zb : chunk_max;
        IndexRec *d_chunk = ctx.arena.alloc<IndexRec>(chunk ? chunk : 1);
        // one word per wavefront of the conversion launches: the literals it wrote (at most n / 64 + 4 per chunk words)
        lit_counts.resize(chunk ? (zb / chunk) * archive_append_counts(chunk) + archive_append_counts(zb % chunk) : 0);
        uint32_t *d_counts = ctx.arena.alloc<uint32_t>(lit_counts.size() ? lit_counts.size() : 1);
        size_t counts_at = 0;
        for (size_t c0 = 0; c0 < zb; c0 += chunk) {  // (one stream: a chunk's conversion has read d_chunk before the next look-up)
            const size_t cnt = zb - c0 < chunk ? zb - c0 : chunk;
            rlz_index_records(ctx, ix.view, d_fpos + c0, (uint32_t)cnt, d_len, d_rank, d_chunk);
            archive_append_records(ctx, d_chunk, d_fpos + c0, (uint32_t)c0, (uint32_t)cnt, base, ab, recs, d_counts + counts_at);
            counts_at += archive_append_counts(cnt);
        }
        archive_extend_sample(ctx, recs, (uint32_t)a.z, (uint32_t)z_new, (uint32_t)samples_old, (uint32_t)samples_new, sample);
        if (counts_at != lit_counts.size()) throw HipError("rlz archive: the literal counts of an append are laid out wrongly");
        if (counts_at)
            HIP_CHECK(hipMemcpyAsync(lit_counts.data(), d_counts, sizeof(uint32_t) * counts_at, hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipStreamSynchronize(s));
        HIP_CHECK(hipGetLastError());
        for (uint32_t c : lit_counts) lit_added += c;
    } catch (...) {
        (void)hipStreamSynchronize(s);  // nothing still reads the batch or writes the fresh arrays when they go
        throw;
    }
    // (the whole scope recorded its stop event as the block above closed, behind that wait: collect() drops a scope whose
    // events have not completed)
    HIP_CHECK(hipStreamSynchronize(s));
    ctx.prof.collect();
    // the commit: host state only, after the device work has finished without error; the stream has drained
    const bool moved = fresh_recs.p || fresh_sample.p;
    if (fresh_recs.p) std::swap(fresh_recs.p, reinterpret_cast<void *&>(a.d_recs));
    if (fresh_sample.p) std::swap(fresh_sample.p, reinterpret_cast<void *&>(a.d_sample));
    a.cap_recs = cap_recs;
    a.cap_samples = cap_samples;
    a.z = z_new;
    a.n_literals += lit_added;
    for (size_t j = 0; j < k; ++j) {
        a.lengths.push_back(target_lens[j]);
        a.decoded += target_lens[j];
        a.bases.push_back(a.decoded);
    }
    a.device_bytes = (a.block_len ? a.block_len : 1) + sizeof(ArchiveRec) * cap_recs + sizeof(uint32_t) * cap_samples;
    fill_append_info(a, info, k, added, lit_added, bases, moved);
}

template <typename T> T *calloc_array(size_t count) {
    T *p = static_cast<T *>(std::calloc(count ? count : 1, sizeof(T)));
    if (!p) throw std::bad_alloc();
    return p;
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

// ---- pattern count and locate --------------------------------------------------------------------------------------
// device memory of a pattern batch of n positions and q patterns: the bytes, the packed words, the terminator table, and
// lo, cnt, rep, off; per hit: two key and two value arrays of the sort (24), its histograms (1/4), and the records of a
// chunk (16)
}  // namespace
size_t nolzss::api::pattern_batch_bytes(size_t n, size_t q) { return 2 * n + 24 * q + (size_t(4) << 20); }
namespace {

using HitBlock = std::unique_ptr<nolzss_rlz_hit, FreeBlock>;
static_assert(sizeof(nolzss_rlz_hit) == sizeof(LocateHit) && sizeof(LocateHit) == 16, "the kernels write nolzss_rlz_hit");

// One batch of q >= 1 patterns against the handle, inside a session.  counts: q entries.  With hit_offsets (q + 1
// entries) the hits of every pattern with at most max_hits occurrences (0: no cap) come down too.
void query_patterns(Context &ctx, const nolzss_rlz_index &h, const Batch &b, size_t q, uint64_t max_hits, uint64_t *counts,
                    uint64_t *hit_offsets, HitBlock &hits, size_t &num_hits) {
    const size_t n = b.tcat.size();
    const bool locate = hit_offsets != nullptr;
    const uint32_t cap = (max_hits == 0 || max_hits >= 0xffffffffull) ? 0xffffffffu : (uint32_t)max_hits;
    const size_t chunk_max = chunk_knob("NOLZSS_RLZ_LOCATE_CHUNK");
    hipStream_t s = ctx.stream;
    std::vector<uint32_t> cnt(q);
    PackedText batch;
    uint32_t *d_lo = nullptr, *d_rep = nullptr;
    // the batch up, packed with the pattern ends as terminators, and searched: the counts come down once
    auto run_patterns = [&] {
        uint8_t *d_T = ctx.arena.alloc<uint8_t>(n);
        {
            ProfScope ps(ctx.profiler(), "text_h2d", s, (double)n);
            upload_bytes(ctx, d_T, b.tcat.data(), n);
        }
        if (!pack_independent_text(ctx, d_T, n, b.separators, batch))
            throw std::runtime_error("rlz index: the batch holds bytes that are neither bases nor its separators");
        d_lo = ctx.arena.alloc<uint32_t>(q);
        d_rep = ctx.arena.alloc<uint32_t>(q);
        uint32_t *d_cnt = ctx.arena.alloc<uint32_t>(q);
        rlz_index_patterns(ctx, h.view, batch, (uint32_t)q, cap, d_lo, d_cnt, d_rep);
        ProfScope ps(ctx.profiler(), "counts_d2h", s, 4.0 * (double)q);
        download_bytes(ctx, cnt.data(), d_cnt, sizeof(uint32_t) * q);
    };
    reserve_arena_for(ctx, 0, pattern_batch_bytes(n, q));
    run_patterns();
    uint64_t total = 0;  // the hits to report, summed in 64 bits
    for (size_t j = 0; j < q; ++j) {
        counts[j] = cnt[j];
        if (locate) {
            hit_offsets[j] = total;
            if (cnt[j] <= cap) total += cnt[j];
        }
    }
    if (!locate) return;
    hit_offsets[q] = total;
    if (total == 0) return;
    if (total > kMaxText)
        throw std::invalid_argument("rlz index: locate would report " + std::to_string(total) + " hits, more than the " +
                                    std::to_string(kMaxText) + " the 32-bit device pipeline takes: lower max_hits (it is " +
                                    std::to_string(max_hits) + "; 0 means no cap) or send fewer patterns");
    const size_t T = (size_t)total, chunk = T < chunk_max ? T : chunk_max;
    // the arena for the hits: a reservation that is not a no-op may replace the slab (and the new one may be as large as
    // the old), so the arena is then emptied and the patterns are searched again in it
    const size_t extra = pattern_batch_bytes(n, q) + kLocateBytesPerHit * T + sizeof(LocateHit) * chunk;
    if (arena_bytes_for(0) + extra > ctx.arena.capacity()) {
        HIP_CHECK(hipStreamSynchronize(s));  // (nothing still reads the slab that goes)
        reserve_arena_for(ctx, 0, extra);
        ctx.arena.rewind(0);
        run_patterns();
    }
    uint32_t *d_off = ctx.arena.alloc<uint32_t>(q);
    rlz_index_hit_offsets(ctx, d_rep, (uint32_t)q, d_off);
    const LocateSorted sorted = rlz_index_hits(ctx, h.view, (uint32_t)h.m, batch, (uint32_t)q, d_off, d_lo, (uint32_t)T);
    hits.reset(static_cast<nolzss_rlz_hit *>(alloc_factor_block(sizeof(nolzss_rlz_hit) * T)));
    if (!hits) throw std::bad_alloc();
    LocateHit *d_recs = ctx.arena.alloc<LocateHit>(chunk);
    for (size_t c0 = 0; c0 < T; c0 += chunk) {
        const size_t c = T - c0 < chunk ? T - c0 : chunk;
        rlz_index_hit_records(ctx, sorted, c0, (uint32_t)c, d_recs);
        ProfScope ps(ctx.profiler(), "hits_d2h", s, (double)(sizeof(LocateHit) * c));
        download_bytes(ctx, hits.get() + c0, d_recs, sizeof(LocateHit) * c);  // (waits: d_recs is free again)
    }
    num_hits = T;
}

void index_query(const nolzss_rlz_index *h, const char *const *patterns, const size_t *pattern_lens, size_t q,
                 uint64_t max_hits, uint64_t *counts, uint64_t *hit_offsets, nolzss_rlz_hit **hits, size_t *num_hits) {
    const bool locate = hits != nullptr;
    if (locate) {
        *hits = nullptr;
        if (num_hits) *num_hits = 0;
    }
    if (!h) throw std::invalid_argument("handle is null");
    if (locate && (!hit_offsets || !num_hits)) throw std::invalid_argument("output pointer is null");
    if (q && !counts) throw std::invalid_argument("output pointer is null");
    // the sort key of a hit holds its pattern in the 31 bits above (position, strand)
    if (locate && q > 0x7fffffffull) throw std::invalid_argument("rlz index: a locate takes at most 2^31 - 1 patterns per batch");
    Batch b;
    prepare_patterns(patterns, pattern_lens, q, b);
    if (locate) hit_offsets[0] = 0;
    if (q == 0) return;
    HitBlock block;
    size_t T = 0;
    DeviceRestore restore;
    Session ses(h->device, nullptr);
    Context &ctx = ses.ctx();
    {
        ProfScope whole(ctx.profiler(), locate ? "rlz_index_locate" : "rlz_index_count", ctx.stream);
        query_patterns(ctx, *h, b, q, max_hits, counts, locate ? hit_offsets : nullptr, block, T);
    }
    HIP_CHECK(hipStreamSynchronize(ctx.stream));
    HIP_CHECK(hipGetLastError());
    ctx.prof.collect();
    if (locate) {
        *hits = block.release();  // ownership moves to the caller
        *num_hits = T;
    }
}

// ---- maximal match seeds -------------------------------------------------------------------------------------------
// device memory of a seed query over a batch of n positions and k targets: per position the byte, the packed word
// (1/4), len, rank, flag and slot (4 each), and -- every position can be a seed (a run of one base against a record of
// one base), so the seeds' arrays are reserved with the batch and their number never moves the arena -- the list,
// first, rep and off (4 each): 34; the terminator table; the seed records of a download chunk.  Per hit: as a locate.
size_t seed_batch_bytes(size_t n, size_t k, size_t chunk) {
    return 34 * n + 16 * k + sizeof(SeedRec) * chunk + (size_t(4) << 20);
}

static_assert(sizeof(nolzss_rlz_seed) == sizeof(SeedRec) && sizeof(SeedRec) == 32, "the kernels write nolzss_rlz_seed");

// One batch of k >= 1 targets with at least one base against the handle, inside a session.  res is filled as the
// results arrive: the seed records and hit_offsets once the counts are known, the hits last.  Returns false when the
// hit total is beyond the pipeline: res then holds the seeds, their counts and the offsets, *total the number.
bool query_seeds(Context &ctx, const nolzss_rlz_index &h, const Batch &b, size_t k, uint64_t min_length, uint64_t max_hits,
                 nolzss_rlz_seeds_result &res, uint64_t *total_out) {
    const size_t n = b.tcat.size();
    const uint32_t cap = (max_hits == 0 || max_hits >= 0xffffffffull) ? 0xffffffffu : (uint32_t)max_hits;
    const uint32_t min_len = min_length >= 0xffffffffull ? 0xffffffffu : (uint32_t)(min_length ? min_length : 1);
    const size_t chunk_max = chunk_knob("NOLZSS_RLZ_LOCATE_CHUNK");
    const size_t seed_chunk = n < chunk_max ? n : chunk_max;
    hipStream_t s = ctx.stream;
    Searched m;
    uint32_t *d_seeds = nullptr, *d_first = nullptr, *d_rep = nullptr;
    uint32_t S = 0;
    // the batch up, packed and searched as a match does, the seeds flagged and listed: their number comes down as one word
    auto run_search = [&] {
        m = search_batch(ctx, h, b);
        uint32_t *d_flag = ctx.arena.alloc<uint32_t>(n), *d_slot = ctx.arena.alloc<uint32_t>(n);
        d_seeds = ctx.arena.alloc<uint32_t>(n);
        uint32_t *d_total = ctx.arena.alloc<uint32_t>(1);
        rlz_index_seed_list(ctx, m.d_len, (uint32_t)n, min_len, d_flag, d_slot, d_seeds, d_total);
        download_bytes(ctx, &S, d_total, sizeof(uint32_t));
        if (S > n) throw HipError("rlz index: more seeds than batch positions");
        d_first = ctx.arena.alloc<uint32_t>(S ? S : 1);
        d_rep = ctx.arena.alloc<uint32_t>(S ? S : 1);
    };
    reserve_arena_for(ctx, 0, seed_batch_bytes(n, k, seed_chunk));
    run_search();
    res.hit_offsets = calloc_array<uint64_t>((size_t)S + 1);
    if (S == 0) return true;
    // the sort key of a hit holds its seed in the 31 bits above (position, strand)
    if (S > 0x7fffffffu) throw std::invalid_argument("rlz index: a batch may report at most 2^31 - 1 seeds, this one has " +
                                                     std::to_string(S) + ": raise min_length or send fewer targets");
    res.seeds = static_cast<nolzss_rlz_seed *>(alloc_factor_block(sizeof(nolzss_rlz_seed) * S));
    if (!res.seeds) throw std::bad_alloc();
    {
        const size_t chunk = S < chunk_max ? S : chunk_max;
        SeedRec *d_recs = ctx.arena.alloc<SeedRec>(chunk);
        for (size_t c0 = 0; c0 < S; c0 += chunk) {
            const size_t c = S - c0 < chunk ? S - c0 : chunk;
            rlz_index_seed_intervals(ctx, h.view, m.batch, d_seeds, (uint32_t)c0, (uint32_t)c, cap, m.d_len, m.d_rank, d_first,
                                     d_rep, d_recs);
            ProfScope ps(ctx.profiler(), "seeds_d2h", s, (double)(sizeof(SeedRec) * c));
            download_bytes(ctx, res.seeds + c0, d_recs, sizeof(SeedRec) * c);  // (waits: d_recs is free again)
        }
    }
    res.num_seeds = S;
    uint64_t total = 0;  // the hits to report, summed in 64 bits
    for (size_t j = 0; j < S; ++j) {
        res.hit_offsets[j] = total;
        if (res.seeds[j].count <= cap) total += res.seeds[j].count;
    }
    res.hit_offsets[S] = total;
    *total_out = total;
    if (total == 0) return true;
    if (total > kMaxText) return false;
    const size_t T = (size_t)total, chunk = T < chunk_max ? T : chunk_max;
    // the arena for the hits, by the rule of a locate: a reservation that is not a no-op may replace the slab (and the
    // new one may be as large as the old), so the arena is then emptied and the batch is searched again in it, its seeds
    // listed and their intervals looked up -- the records have come down and are not written a second time
    const size_t extra = seed_batch_bytes(n, k, seed_chunk) + kLocateBytesPerHit * T + sizeof(LocateHit) * chunk;
    if (arena_bytes_for(0) + extra > ctx.arena.capacity()) {
        HIP_CHECK(hipStreamSynchronize(s));  // (nothing still reads the slab that goes)
        reserve_arena_for(ctx, 0, extra);
        ctx.arena.rewind(0);
        const uint32_t before = S;
        run_search();
        if (S != before) throw HipError("rlz index: the seeds of a batch changed between two searches");
        rlz_index_seed_intervals(ctx, h.view, m.batch, d_seeds, 0u, S, cap, m.d_len, m.d_rank, d_first, d_rep, nullptr);
    }
    const LocateSorted sorted =
        rlz_index_seed_hits(ctx, h.view, (uint32_t)h.m, (uint32_t)n, d_seeds, m.d_len, S, d_rep, d_first, (uint32_t)T);
    res.hits = static_cast<nolzss_rlz_hit *>(alloc_factor_block(sizeof(nolzss_rlz_hit) * T));
    if (!res.hits) throw std::bad_alloc();
    LocateHit *d_recs = ctx.arena.alloc<LocateHit>(chunk);
    for (size_t c0 = 0; c0 < T; c0 += chunk) {
        const size_t c = T - c0 < chunk ? T - c0 : chunk;
        rlz_index_hit_records(ctx, sorted, c0, (uint32_t)c, d_recs);
        ProfScope ps(ctx.profiler(), "hits_d2h", s, (double)(sizeof(LocateHit) * c));
        download_bytes(ctx, res.hits + c0, d_recs, sizeof(LocateHit) * c);  // (waits: d_recs is free again)
    }
    res.num_hits = T;
    return true;
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
    bool fits = true;
    uint64_t total = 0;
    try {
        if (b.tcat.size() == k) {  // no target, or none with a base: the device is not touched
            res.hit_offsets = calloc_array<uint64_t>(1);
        } else {
            DeviceRestore restore;
            Session ses(h->device, nullptr);
            Context &ctx = ses.ctx();
            {
                ProfScope whole(ctx.profiler(), "rlz_index_seeds", ctx.stream);
                fits = query_seeds(ctx, *h, b, k, min_length, max_hits, res, &total);
            }
            HIP_CHECK(hipStreamSynchronize(ctx.stream));
            HIP_CHECK(hipGetLastError());
            ctx.prof.collect();
        }
    } catch (...) {
        nolzss_free_rlz_seeds_result(&res);
        throw;
    }
    *out = res;  // ownership moves to the caller
    if (!fits)
        throw std::invalid_argument("rlz index: seeds would report " + std::to_string(total) + " hits, more than the " +
                                    std::to_string(kMaxText) + " the 32-bit device pipeline takes: lower max_hits (it is " +
                                    std::to_string(max_hits) + "; 0 means no cap), raise min_length (it is " +
                                    std::to_string(min_length) + ") or send fewer targets");
}

// ---- colinear seed chains ------------------------------------------------------------------------------------------
// device memory per hit of a seed-chain query, on top of the 25 of the expanded and sorted hits: the anchors in group
// order (two key and two value arrays of the second sort, q and L by slot and by anchor: 40, the histograms 1) and what
// rlz_seed_chain_run states (152); every group and every chain anchor is at most one per hit
constexpr size_t kChainBytesPerHit = 40 + 1 + 152;

static_assert(sizeof(nolzss_rlz_chain) == sizeof(ChainRec) && sizeof(ChainRec) == 64, "the kernels write nolzss_rlz_chain");
static_assert(sizeof(nolzss_rlz_chain_anchor) == sizeof(ChainAnchorRec) && sizeof(ChainAnchorRec) == 24,
              "the kernels write nolzss_rlz_chain_anchor");
static_assert(NOLZSS_RLZ_CHAIN_LOOKBACK == kChainLookback, "the look-back is a constant of the ABI");

// `count` records of `size` bytes from device memory into a host array, NOLZSS_RLZ_LOCATE_CHUNK records per copy
void download_records(Context &ctx, const char *scope, void *h_dst, const void *d_src, size_t count, size_t size) {
    const size_t chunk_max = chunk_knob("NOLZSS_RLZ_LOCATE_CHUNK");
    for (size_t c0 = 0; c0 < count; c0 += chunk_max) {
        const size_t c = count - c0 < chunk_max ? count - c0 : chunk_max;
        ProfScope ps(ctx.profiler(), scope, ctx.stream, (double)(size * c));
        download_bytes(ctx, static_cast<char *>(h_dst) + c0 * size, static_cast<const char *>(d_src) + c0 * size, c * size);
    }
}

}  // namespace
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

namespace {

// One batch of k >= 1 targets with at least one base against the handle, inside a session: the path of query_seeds up to
// the sorted hits, which stay on the device, then the chain stages.  Returns false when the hit total is beyond the
// pipeline: res is then empty, *total the number.
bool query_seed_chains(Context &ctx, const nolzss_rlz_index &h, const Batch &b, size_t k, const nolzss_rlz_chain_params &p,
                       nolzss_rlz_seed_chains_result &res, uint64_t *total_out) {
    const size_t n = b.tcat.size();
    const uint32_t cap = (p.max_hits == 0 || p.max_hits >= 0xffffffffull) ? 0xffffffffu : (uint32_t)p.max_hits;
    const uint32_t min_len = p.min_length >= 0xffffffffull ? 0xffffffffu : (uint32_t)(p.min_length ? p.min_length : 1);
    hipStream_t s = ctx.stream;
    Searched m;
    uint32_t *d_seeds = nullptr, *d_first = nullptr, *d_rep = nullptr;
    uint32_t S = 0;
    // as query_seeds: the batch searched, the seeds listed, their intervals looked up -- no record is written
    auto run_search = [&] {
        m = search_batch(ctx, h, b);
        uint32_t *d_flag = ctx.arena.alloc<uint32_t>(n), *d_slot = ctx.arena.alloc<uint32_t>(n);
        d_seeds = ctx.arena.alloc<uint32_t>(n);
        uint32_t *d_total = ctx.arena.alloc<uint32_t>(1);
        rlz_index_seed_list(ctx, m.d_len, (uint32_t)n, min_len, d_flag, d_slot, d_seeds, d_total);
        download_bytes(ctx, &S, d_total, sizeof(uint32_t));
        if (S > n) throw HipError("rlz index: more seeds than batch positions");
        d_first = ctx.arena.alloc<uint32_t>(S ? S : 1);
        d_rep = ctx.arena.alloc<uint32_t>(S ? S : 1);
        if (S > 0x7fffffffu) return;
        rlz_index_seed_intervals(ctx, h.view, m.batch, d_seeds, 0u, S, cap, m.d_len, m.d_rank, d_first, d_rep, nullptr);
    };
    reserve_arena_for(ctx, 0, seed_batch_bytes(n, k, 0));
    run_search();
    if (S > 0x7fffffffu) throw std::invalid_argument("rlz index: a batch may report at most 2^31 - 1 seeds, this one has " +
                                                     std::to_string(S) + ": raise min_length or send fewer targets");
    res.num_seeds = S;
    uint64_t total = 0;  // the hits to expand, summed in 64 bits on the device: one word comes down
    if (S) {
        uint64_t *d_sum = ctx.arena.alloc<uint64_t>(1);
        rlz_index_rep_total(ctx, d_rep, S, d_sum);
        download_bytes(ctx, &total, d_sum, sizeof(uint64_t));
    }
    *total_out = total;
    if (total > kMaxText) return false;
    if (total == 0) {
        res.anchor_offsets = calloc_array<uint64_t>(1);
        return true;
    }
    const size_t T = (size_t)total;
    // the arena for the hits, by the two-reservation rule of a locate and of the seeds, extended by the per-hit and
    // per-group arrays of the chain stages: a reservation that is not a no-op may replace the slab, so the arena is then
    // emptied and the batch is searched again in it
    const size_t extra = seed_batch_bytes(n, k, 0) + (kLocateBytesPerHit + kChainBytesPerHit) * T;
    if (arena_bytes_for(0) + extra > ctx.arena.capacity()) {
        HIP_CHECK(hipStreamSynchronize(s));  // (nothing still reads the slab that goes)
        reserve_arena_for(ctx, 0, extra);
        ctx.arena.rewind(0);
        const uint32_t before = S;
        run_search();
        if (S != before) throw HipError("rlz index: the seeds of a batch changed between two searches");
    }
    const LocateSorted sorted =
        rlz_index_seed_hits(ctx, h.view, (uint32_t)h.m, (uint32_t)n, d_seeds, m.d_len, S, d_rep, d_first, (uint32_t)T);
    res.num_seed_hits = T;
    const ChainAnchors anchors = rlz_seed_chain_anchors(ctx, h.view, (uint32_t)h.m, m.batch, d_seeds, m.d_len, S, sorted, (uint32_t)T);
    const ChainsOut run = rlz_seed_chain_run(ctx, anchors, chain_rules(p, h.m, h.view.B));
    deliver_chains(ctx, run, res);
    return true;
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
    bool fits = true;
    uint64_t total = 0;
    try {
        if (b.tcat.size() == k) {  // no target, or none with a base: the device is not touched
            res.anchor_offsets = calloc_array<uint64_t>(1);
        } else {
            DeviceRestore restore;
            Session ses(h->device, nullptr);
            Context &ctx = ses.ctx();
            {
                ProfScope whole(ctx.profiler(), "rlz_index_seed_chains", ctx.stream);
                fits = query_seed_chains(ctx, *h, b, k, *params, res, &total);
            }
            HIP_CHECK(hipStreamSynchronize(ctx.stream));
            HIP_CHECK(hipGetLastError());
            ctx.prof.collect();
        }
    } catch (...) {
        nolzss_free_rlz_seed_chains_result(&res);
        throw;
    }
    if (!fits) {  // an empty result and the status
        nolzss_free_rlz_seed_chains_result(&res);
        throw std::invalid_argument("rlz index: seeds would report " + std::to_string(total) + " hits, more than the " +
                                    std::to_string(kMaxText) + " the 32-bit device pipeline takes: lower max_hits (it is " +
                                    std::to_string(params->max_hits) + "; 0 means no cap), raise min_length (it is " +
                                    std::to_string(params->min_length) + ") or send fewer targets");
    }
    *out = res;  // ownership moves to the caller
}

// ---- base-level alignments -----------------------------------------------------------------------------------------
// device memory of the align stages, on top of a seed-chain query.  Per hit -- a chain has at least one anchor and an
// anchor is a hit, so the jobs, one per anchor and one more per chain, are at most two per hit --: the jobs with their
// sizes, offsets and results (48 + 12 + 20 each), L' per anchor (4) and the record and op offset of a chain (88): at most 264.
// Per DP row the two direction words: 16.  Per column slot the code byte, flag, weight and their scans (17) and, an op
// being at most one per slot, its start, code and word (12), rounded up for the scans' tile sums: 32.
constexpr size_t kAlignBytesPerHit = 264, kAlignBytesPerRow = 16, kAlignBytesPerSlot = 32;

static_assert(sizeof(nolzss_rlz_alignment) == sizeof(AlignRec) && sizeof(AlignRec) == 80, "the kernels write nolzss_rlz_alignment");
static_assert(NOLZSS_RLZ_ALIGN_LANES == kAlignLanes, "the diagonals of a job are a constant of the ABI");
static_assert(sizeof(AlignJob) == 48, "the arena accounting counts 48 bytes per job");

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

// One batch of k >= 1 targets with at least one base against the handle, inside a session: the path of
// query_seed_chains up to the chains, which stay on the device, then the align stages.  Returns false with *why when a
// total is beyond the pipeline: res is then empty.
bool query_align(Context &ctx, const nolzss_rlz_index &h, const Batch &b, size_t k, const nolzss_rlz_align_params &p,
                 nolzss_rlz_align_result &res, std::string *why) {
    const size_t n = b.tcat.size();
    const uint32_t cap = (p.max_hits == 0 || p.max_hits >= 0xffffffffull) ? 0xffffffffu : (uint32_t)p.max_hits;
    const uint32_t min_len = p.min_length >= 0xffffffffull ? 0xffffffffu : (uint32_t)(p.min_length ? p.min_length : 1);
    nolzss_rlz_chain_params cp;
    cp.min_length = p.min_length;
    cp.max_hits = p.max_hits;
    cp.max_gap = p.max_gap;
    cp.bandwidth = p.bandwidth;
    cp.min_score = p.min_score;
    const ChainRules rules = chain_rules(cp, h.m, h.view.B);
    hipStream_t s = ctx.stream;
    Searched m;
    uint32_t *d_seeds = nullptr, *d_first = nullptr, *d_rep = nullptr;
    uint32_t S = 0;
    // as query_seed_chains: the batch searched, the seeds listed, their intervals looked up
    auto run_search = [&] {
        m = search_batch(ctx, h, b);
        uint32_t *d_flag = ctx.arena.alloc<uint32_t>(n), *d_slot = ctx.arena.alloc<uint32_t>(n);
        d_seeds = ctx.arena.alloc<uint32_t>(n);
        uint32_t *d_total = ctx.arena.alloc<uint32_t>(1);
        rlz_index_seed_list(ctx, m.d_len, (uint32_t)n, min_len, d_flag, d_slot, d_seeds, d_total);
        download_bytes(ctx, &S, d_total, sizeof(uint32_t));
        if (S > n) throw HipError("rlz index: more seeds than batch positions");
        d_first = ctx.arena.alloc<uint32_t>(S ? S : 1);
        d_rep = ctx.arena.alloc<uint32_t>(S ? S : 1);
        if (S > 0x7fffffffu) return;
        rlz_index_seed_intervals(ctx, h.view, m.batch, d_seeds, 0u, S, cap, m.d_len, m.d_rank, d_first, d_rep, nullptr);
    };
    reserve_arena_for(ctx, 0, seed_batch_bytes(n, k, 0));
    run_search();
    if (S > 0x7fffffffu) throw std::invalid_argument("rlz index: a batch may report at most 2^31 - 1 seeds, this one has " +
                                                     std::to_string(S) + ": raise min_length or send fewer targets");
    uint64_t total = 0;  // the hits to expand, summed in 64 bits on the device: one word comes down
    if (S) {
        uint64_t *d_sum = ctx.arena.alloc<uint64_t>(1);
        rlz_index_rep_total(ctx, d_rep, S, d_sum);
        download_bytes(ctx, &total, d_sum, sizeof(uint64_t));
    }
    if (total > kMaxText) {
        *why = "rlz index: seeds would report " + std::to_string(total) + " hits, more than the " + std::to_string(kMaxText) +
               " the 32-bit device pipeline takes: lower max_hits (it is " + std::to_string(p.max_hits) +
               "; 0 means no cap), raise min_length (it is " + std::to_string(p.min_length) + ") or send fewer targets";
        return false;
    }
    if (total == 0) {
        res.op_offsets = calloc_array<uint64_t>(1);
        return true;
    }
    const size_t T = (size_t)total;
    // the chains and the jobs of the batch, planned and sized: three totals come down
    ChainsOut run;
    AlignJobs jobs;
    auto run_chains = [&] {
        const LocateSorted sorted =
            rlz_index_seed_hits(ctx, h.view, (uint32_t)h.m, (uint32_t)n, d_seeds, m.d_len, S, d_rep, d_first, (uint32_t)T);
        const ChainAnchors anchors = rlz_seed_chain_anchors(ctx, h.view, (uint32_t)h.m, m.batch, d_seeds, m.d_len, S, sorted, (uint32_t)T);
        run = rlz_seed_chain_run(ctx, anchors, rules);
        jobs = rlz_align_plan(ctx, h.view, m.batch, run, (uint32_t)p.band, p.max_flank);
        rlz_align_sizes(ctx, jobs);
    };
    // the arena by the two-reservation rule of the seeds and the seed chains, twice: once the hits are counted for what
    // is per hit, once the jobs are sized for what is per DP row and per column slot.  A reservation that is not a no-op
    // may replace the slab, so the arena is then emptied and the batch is searched -- and the second time chained and
    // planned -- again in it
    auto regrow = [&](size_t extra) {
        if (arena_bytes_for(0) + extra <= ctx.arena.capacity()) return false;
        HIP_CHECK(hipStreamSynchronize(s));  // (nothing still reads the slab that goes)
        reserve_arena_for(ctx, 0, extra);
        ctx.arena.rewind(0);
        const uint32_t before = S;
        run_search();
        if (S != before) throw HipError("rlz index: the seeds of a batch changed between two searches");
        return true;
    };
    const size_t per_hit = seed_batch_bytes(n, k, 0) + (kLocateBytesPerHit + kChainBytesPerHit + kAlignBytesPerHit) * T;
    regrow(per_hit);
    run_chains();
    if (run.num_chains == 0) {
        res.op_offsets = calloc_array<uint64_t>(1);
        return true;
    }
    const uint64_t rows = jobs.total_rows, slots = jobs.total_slots, weight = jobs.total_weight;
    if (rows > 0xffffffffull || slots > 0xffffffffull || weight > 0xffffffffull) {
        *why = "rlz index: the alignments of this batch take " + std::to_string(rows) + " DP rows, " + std::to_string(slots) +
               " column slots and up to " + std::to_string(weight) + " columns, and each is counted in 32 bits: send fewer targets";
        return false;
    }
    if (regrow(per_hit + kAlignBytesPerRow * (size_t)rows + kAlignBytesPerSlot * (size_t)slots)) {
        run_chains();
        if (jobs.total_rows != rows || jobs.total_slots != slots || jobs.total_weight != weight)
            throw HipError("rlz index: the alignment jobs of a batch changed between two runs");
    }
    rlz_align_layout(ctx, jobs);
    rlz_align_dp(ctx, jobs, m.batch, h.view.text);
    rlz_align_traceback(ctx, jobs);
    const AlignOut aligned = rlz_align_ops(ctx, jobs, run, rules);
    res.num_jobs = jobs.J;
    res.num_rows = (size_t)rows;
    deliver_alignments(ctx, aligned, res);
    return true;
}

void index_align(const nolzss_rlz_index *h, const char *const *targets, const size_t *target_lens, size_t k,
                 const nolzss_rlz_align_params *params, nolzss_rlz_align_result *out) {
    if (!out) throw std::invalid_argument("output pointer is null");
    std::memset(out, 0, sizeof *out);
    if (!h) throw std::invalid_argument("handle is null");
    if (!params) throw std::invalid_argument("rlz index: alignments need their parameters: params is null");
    if (k > kChainMaxTargets)
        throw std::invalid_argument("rlz index: seed chains take at most 2^24 targets per batch, this one has " + std::to_string(k) +
                                    " (the group sort key keeps the target in 24 bits): send fewer targets");
    if (params->bandwidth >= kAlignLanes || params->band >= kAlignLanes || params->bandwidth + 2 * params->band + 1 > kAlignLanes)
        throw std::invalid_argument("rlz index: an alignment job has at most 64 diagonals, one per lane of a wavefront: bandwidth + 2 "
                                    "band + 1 is " + std::to_string(params->bandwidth) + " + 2 * " + std::to_string(params->band) +
                                    " + 1: lower bandwidth or band");
    for (size_t j = 0; target_lens && j < k; ++j)  // (the lengths alone decide; a null array is the batch's refusal below)
        if (target_lens[j] >= kAlignMaxTarget)
            throw std::invalid_argument("rlz index: alignments take targets below 2^28 bases, target " + std::to_string(j) + " has " +
                                        std::to_string(target_lens[j]) + " (an op keeps its length in 28 bits)");
    Batch b;
    prepare_batch(*h, targets, target_lens, k, b);
    nolzss_rlz_align_result res;
    std::memset(&res, 0, sizeof res);
    bool fits = true;
    std::string why;
    try {
        if (b.tcat.size() == k) {  // no target, or none with a base: the device is not touched
            res.op_offsets = calloc_array<uint64_t>(1);
        } else {
            DeviceRestore restore;
            Session ses(h->device, nullptr);
            Context &ctx = ses.ctx();
            {
                ProfScope whole(ctx.profiler(), "rlz_index_align", ctx.stream);
                fits = query_align(ctx, *h, b, k, *params, res, &why);
            }
            HIP_CHECK(hipStreamSynchronize(ctx.stream));
            HIP_CHECK(hipGetLastError());
            ctx.prof.collect();
        }
    } catch (...) {
        nolzss_free_rlz_align_result(&res);
        throw;
    }
    if (!fits) {  // an empty result and the status
        nolzss_free_rlz_align_result(&res);
        throw std::invalid_argument(why);
    }
    *out = res;  // ownership moves to the caller
}

}  // namespace

extern "C" {

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
        info->device_bytes = h->device_bytes;
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

int nolzss_rlz_index_count(const nolzss_rlz_index *h, const char *const *patterns, const size_t *pattern_lens, size_t q,
                           uint64_t *counts) {
    return guarded([&] { index_query(h, patterns, pattern_lens, q, 0, counts, nullptr, nullptr, nullptr); });
}

int nolzss_rlz_index_locate(const nolzss_rlz_index *h, const char *const *patterns, const size_t *pattern_lens, size_t q,
                            uint64_t max_hits, uint64_t *counts, uint64_t *hit_offsets, nolzss_rlz_hit **hits,
                            size_t *num_hits) {
    return guarded([&] {
        if (!hits) throw std::invalid_argument("output pointer is null");
        index_query(h, patterns, pattern_lens, q, max_hits, counts, hit_offsets, hits, num_hits);
    });
}

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

int nolzss_debug_rlz_locate_shifts(uint64_t block_length, uint64_t q, int *shifts, int *npasses) {
    return guarded([&] {
        if (!shifts || !npasses) throw std::invalid_argument("output pointer is null");
        *npasses = rlz_locate_sort_shifts(block_length, q, shifts);
    });
}

int nolzss_rlz_archive_open_index(const nolzss_rlz_index *ix, nolzss_rlz_archive **h) {
    return guarded([&] {
        if (h) *h = nullptr;
        if (!ix) throw std::invalid_argument("index handle is null");
        archive_open_index(*ix, h);
    });
}

int nolzss_rlz_archive_append_index(nolzss_rlz_archive *h, const nolzss_rlz_index *ix, const char *const *targets,
                                    const size_t *target_lens, size_t k, nolzss_rlz_archive_append_info *info) {
    return guarded([&] {
        if (info) std::memset(info, 0, sizeof *info);
        if (!h || !ix) throw std::invalid_argument("archive or index handle is null");
        archive_append(*h, *ix, targets, target_lens, k, info);
    });
}

int nolzss_rlz_index_close(nolzss_rlz_index *h) {
    return guarded([&] { delete h; });
}

}  // extern "C"
