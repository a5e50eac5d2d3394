// rlz_find_api.hip -- the finder handle and its entry points: a snapshot of a relative-LZ archive opened over an index,
// queried for the occurrences of pattern batches inside the targets (part of the C ABI layer of libnolzss_hip.so,
// include/nolzss_hip.h, nolzss_rlz_finder_*; the kernels: rlz_find.hip, and rlz_locate.hip for the pattern bisection,
// the hit expansion and the sort; DESIGN.md 5, "Relative-LZ archive: locate through the parse").
#include "rlz_handles.hpp"

using namespace nolzss;
using namespace nolzss::api;

namespace {

constexpr uint64_t kMaxPattern = 4096;

size_t padded(size_t bytes) { return (bytes + 255) & ~size_t(255); }

// arrays copied one behind the other into one allocation, each 256-byte aligned and padded
struct Layout {
    char *base;
    size_t at = 0;
    Context &ctx;
    Layout(Context &c, void *b) : base(static_cast<char *>(b)), ctx(c) {}
    const uint32_t *put(const uint32_t *d_src, size_t count) {
        char *dst = base + at;
        HIP_CHECK(hipMemcpyAsync(dst, d_src, count * sizeof(uint32_t), hipMemcpyDeviceToDevice, ctx.stream));
        at += padded(count * sizeof(uint32_t));
        return reinterpret_cast<const uint32_t *>(dst);
    }
};

void finder_open(const nolzss_rlz_archive *ap, const nolzss_rlz_index *ip, uint64_t M, uint32_t prefix_syms,
                 nolzss_rlz_finder **out) {
    if (!out) throw std::invalid_argument("output pointer is null");
    *out = nullptr;
    if (!ap || !ip) throw std::invalid_argument("archive or index handle is null");
    const nolzss_rlz_archive &a = *ap;
    const nolzss_rlz_index &ix = *ip;
    if (!a.index_serial)
        throw std::invalid_argument("rlz finder: open takes an archive opened by nolzss_rlz_archive_open_index");
    if (a.index_serial != ix.serial || a.device != ix.device)
        throw std::invalid_argument("rlz finder: the archive is bound to another index (it was opened over index " +
                                    std::to_string(a.index_serial) + " on device " + std::to_string(a.device) +
                                    ", this is index " + std::to_string(ix.serial) + " on device " + std::to_string(ix.device) + ")");
    if (M < 1 || M > kMaxPattern)
        throw std::invalid_argument("rlz finder: max_pattern_length must be 1 .. " + std::to_string(kMaxPattern) + ", it is " +
                                    std::to_string(M));
    if (prefix_syms > kIndexMaxPrefix) throw std::invalid_argument("prefix_syms must be 0 (choose) or 1 .. 12");
    const bool with_rc = ix.view.with_rc;
    const uint64_t W = M > 1 ? M - 1 : 1;
    const uint64_t bound = std::min<uint64_t>(a.decoded, 2 * W * a.z);  // every record start brings at most 2 W bytes
    const uint64_t text_bound = with_rc ? 2 * bound + 2 : bound + 1;
    if (text_bound > kMaxText)
        throw std::invalid_argument("rlz finder: the kernel text of z = " + std::to_string(a.z) + " records with max_pattern_length " +
                                    std::to_string(M) + " may hold " + std::to_string(bound) + " bytes, an index text of " +
                                    std::to_string(text_bound) + " positions, beyond the " + std::to_string(kMaxText) +
                                    " the 32-bit device pipeline takes");

    std::unique_ptr<nolzss_rlz_finder> h(new nolzss_rlz_finder);
    h->device = a.device;
    h->archive = ap;
    h->index = ip;
    h->z = a.z;
    h->targets = a.lengths.size();
    h->decoded = a.decoded;
    h->M = M;
    h->with_rc = with_rc;
    if (a.z == 0) {  // nothing to find: no device
        *out = h.release();
        return;
    }
    const uint32_t z = (uint32_t)a.z, k = (uint32_t)a.lengths.size();
    std::vector<uint32_t> bases(a.bases.begin(), a.bases.end());  // (decoded <= kMaxText)
    const ArchiveView av = a.view();

    DeviceRestore restore;
    Session ses(a.device, nullptr);
    Context &ctx = ses.ctx();
    hipStream_t s = ctx.stream;
    try {
        ProfScope whole(ctx.profiler(), "rlz_finder_open", s);
        // the intervals: found in the arena, kept in an allocation of the handle's own
        reserve_arena_for(ctx, 0, 4 * ((size_t)k + 1) + 28 * ((size_t)z + 1) + (size_t(4) << 20));
        uint32_t *d_bases = ctx.arena.alloc<uint32_t>((size_t)k + 1);
        uint32_t *d_kstart = ctx.arena.alloc<uint32_t>((size_t)z + 1), *d_dstart = ctx.arena.alloc<uint32_t>((size_t)z + 1);
        upload_bytes(ctx, d_bases, bases.data(), sizeof(uint32_t) * bases.size());
        uint32_t K_len = 0;
        const uint32_t nI = find_intervals(ctx, av, d_bases, k, (uint32_t)W, d_kstart, d_dstart, &K_len);
        if (K_len == 0 || K_len > bound) throw HipError("rlz finder: the kernel text is laid out wrongly");
        const size_t table_bytes = 2 * padded(sizeof(uint32_t) * ((size_t)nI + 1)) + padded(sizeof(uint32_t) * ((size_t)k + 1));
        h->tables.alloc(ctx, table_bytes);
        HIP_CHECK(hipMemsetAsync(h->tables.get(), 0, table_bytes, s));
        Layout tables(ctx, h->tables.get());
        FinderView &f = h->view;
        f.kstart = tables.put(d_kstart, (size_t)nI + 1);
        f.dstart = tables.put(d_dstart, (size_t)nI + 1);
        f.bases = tables.put(d_bases, (size_t)k + 1);
        f.z = z;
        f.nI = nI;
        f.k = k;
        h->K_len = K_len;
        h->intervals = nI;
        HIP_CHECK(hipStreamSynchronize(s));  // (nothing still reads the slab that may go)

        // K and its index, built as an index over one reference record is
        const size_t nX = with_rc ? 2 * (size_t)K_len + 2 : (size_t)K_len + 1;
        const uint32_t P = prefix_syms ? prefix_syms : choose_prefix(nX);
        reserve_arena_for(ctx, nX, nX + 4 * ((size_t(1) << (2 * P)) + 1) + 64 * (size_t)z + (size_t(4) << 20));
        ctx.arena.rewind(0);
        uint8_t *d_X = ctx.arena.alloc<uint8_t>(nX);
        find_kernel_text(ctx, av, f.kstart, f.dstart, nI, K_len, with_rc, rc_sentinel(0), rc_sentinel(1), d_X);
        const RlzIndexView built = rlz_index_build(ctx, d_X, (uint32_t)nX, K_len, with_rc, P);
        h->kindex.alloc(ctx, rlz_index_footprint(built));
        h->kview = rlz_index_copy_into(ctx, built, h->kindex.get());
        HIP_CHECK(hipStreamSynchronize(s));
        ctx.arena.rewind(0);

        // the source table
        const SourceTable st = find_source_table(ctx, av, (uint32_t)a.block_len);
        size_t source_bytes = 3 * padded(sizeof(uint32_t) * (size_t)z);
        for (int l = 1; l < st.Phi.nlev; ++l) source_bytes += padded(sizeof(uint32_t) * (size_t)st.Phi.len[l]);
        h->sources.alloc(ctx, source_bytes);
        HIP_CHECK(hipMemsetAsync(h->sources.get(), 0, source_bytes, s));  // (the padding is read, never used)
        Layout sources(ctx, h->sources.get());
        f.lo = sources.put(st.lo, z);
        f.hi = sources.put(st.hi, z);
        f.rec = sources.put(st.rec, z);
        f.Phi = st.Phi;
        f.Phi.lvl[0] = f.hi;
        for (int l = 1; l < st.Phi.nlev; ++l) f.Phi.lvl[l] = sources.put(st.Phi.lvl[l], st.Phi.len[l]);
    } catch (...) {
        (void)hipStreamSynchronize(s);  // nothing still writes the handle's arrays when they go
        throw;
    }
    HIP_CHECK(hipStreamSynchronize(s));
    HIP_CHECK(hipGetLastError());
    ctx.prof.collect();
    ctx.arena.release();  // the sort's arena goes back to the driver, as after nolzss_rlz_index_open
    *out = h.release();
}

using TargetHitBlock = HostBlock<nolzss_rlz_target_hit>;
static_assert(sizeof(nolzss_rlz_target_hit) == sizeof(TargetHit) && sizeof(TargetHit) == 24,
              "the kernels write nolzss_rlz_target_hit");

// per expanded hit: what a locate keeps (the sorted pairs and the sort, kLocateBytesPerHit), its count and its scan entry
constexpr size_t kFindBytesPerHit = kLocateBytesPerHit + 4 + 8;

// One batch of q >= 1 patterns against a finder with records, inside a session.  counts: q entries.  With hit_offsets (q
// + 1 entries) the hits of every pattern with at most max_hits occurrences (0: no cap) come down too.
void query_finder(Context &ctx, const nolzss_rlz_finder &h, const Batch &b, size_t q, uint64_t max_hits, uint64_t *counts,
                  uint64_t *hit_offsets, TargetHitBlock &hits, size_t &num_hits) {
    const size_t n = b.tcat.size();
    const bool locate = hit_offsets != nullptr;
    const size_t chunk_max = chunk_knob("NOLZSS_RLZ_LOCATE_CHUNK");
    const FinderView &f = h.view;
    const ArchiveView av = h.archive->view();
    const RlzIndexView *views[2] = {&h.index->view, &h.kview};
    const uint32_t records[2] = {(uint32_t)h.index->m, 1u};
    hipStream_t s = ctx.stream;
    std::vector<uint32_t> cnt(q), out_off;
    // The arena: the batch first, then, once their numbers are known, the expanded hits, then the hits to report.  A
    // reservation that is not a no-op may replace the slab, so the query then starts again in the new one: at most
    // three times, as every start asks for more than the one before.
    const size_t need_batch = 2 * pattern_batch_bytes(n, q) + 16 * q;
    size_t need = need_batch, granted = 0;
    for (int attempt = 0; attempt < 4; ++attempt) {
        if (need > granted && arena_bytes_for(0) + need > ctx.arena.capacity()) {
            HIP_CHECK(hipStreamSynchronize(s));  // (nothing still reads the slab that goes)
            reserve_arena_for(ctx, 0, need);
        }
        granted = need;
        ctx.arena.rewind(0);
        // the batch up, packed with the pattern ends as terminators, and searched in the block and in K
        uint8_t *d_T = ctx.arena.alloc<uint8_t>(n);
        {
            ProfScope ps(ctx.profiler(), "text_h2d", s, (double)n);
            upload_bytes(ctx, d_T, b.tcat.data(), n);
        }
        PackedText batch;
        if (!pack_independent_text(ctx, d_T, n, b.separators, batch))
            throw std::runtime_error("rlz finder: the batch holds bytes that are neither bases nor its separators");
        uint32_t *d_lo[2], *d_rep[2], *d_off[2];
        uint64_t T[2] = {0, 0};
        for (int c = 0; c < 2; ++c) {
            d_lo[c] = ctx.arena.alloc<uint32_t>(q);
            d_rep[c] = ctx.arena.alloc<uint32_t>(q + 1);  // (one entry more: the scan then ends in the total)
            d_off[c] = ctx.arena.alloc<uint32_t>(q + 1);
            uint32_t *d_cnt = ctx.arena.alloc<uint32_t>(q);
            HIP_CHECK(hipMemsetAsync(d_rep[c] + q, 0, sizeof(uint32_t), s));
            rlz_index_patterns(ctx, *views[c], batch, (uint32_t)q, 0xffffffffu, d_lo[c], d_cnt, d_rep[c]);
            ProfScope ps(ctx.profiler(), "counts_d2h", s, 4.0 * (double)q);
            download_bytes(ctx, cnt.data(), d_cnt, sizeof(uint32_t) * q);
            for (size_t j = 0; j < q; ++j) T[c] += cnt[j];
        }
        if (T[0] > kMaxText || T[1] > kMaxText)
            throw std::invalid_argument("rlz finder: the batch has " + std::to_string(T[0]) + " occurrences in the block and " +
                                        std::to_string(T[1]) + " in the kernel text, more than the " + std::to_string(kMaxText) +
                                        " the 32-bit device pipeline takes: send fewer patterns");
        const size_t need_hits = need_batch + kFindBytesPerHit * (size_t)(T[0] + T[1]) + 8 * q + (size_t(1) << 20);
        if (need_hits > granted && arena_bytes_for(0) + need_hits > ctx.arena.capacity()) {
            need = need_hits;
            continue;
        }

        // every occurrence expanded and sorted by (pattern, position, strand); counted; the counts scanned in 64 bits
        const uint64_t *d_hits[2];
        uint64_t *d_scan[2];
        for (int c = 0; c < 2; ++c) {
            scan_exclusive_add_u32(d_rep[c], d_off[c], q + 1, nullptr, ctx.arena, s);
            const LocateSorted sorted =
                rlz_index_hits(ctx, *views[c], records[c], batch, (uint32_t)q, d_off[c], d_lo[c], (uint32_t)T[c]);
            d_hits[c] = sorted.keys;
            uint32_t *d_cnt = ctx.arena.alloc<uint32_t>(T[c] ? T[c] : 1);
            d_scan[c] = ctx.arena.alloc<uint64_t>(T[c] + 1);
            if (c == 0) find_secondary_count(ctx, f, d_hits[c], (uint32_t)T[c], batch.terms.pos, d_cnt);
            else find_primary_count(ctx, f, av, d_hits[c], (uint32_t)T[c], batch.terms.pos, d_cnt);
            find_scan_u64(ctx, d_cnt, (uint32_t)T[c], d_scan[c]);
        }
        uint64_t *d_counts = ctx.arena.alloc<uint64_t>(q);
        find_pattern_counts(ctx, d_scan[0], d_off[0], d_scan[1], d_off[1], (uint32_t)q, d_counts);
        {
            ProfScope ps(ctx.profiler(), "counts_d2h", s, 8.0 * (double)q);
            download_bytes(ctx, counts, d_counts, sizeof(uint64_t) * q);
        }
        if (!locate) return;
        const uint64_t cap = max_hits == 0 ? ~0ull : max_hits;
        uint64_t total = 0;  // the hits to report
        bool wraps = false;
        for (size_t j = 0; j < q; ++j) {
            hit_offsets[j] = total;
            if (counts[j] <= cap) {
                wraps |= total + counts[j] < total;
                total += counts[j];
            }
        }
        hit_offsets[q] = total;
        if (total == 0) return;
        if (wraps || total > kMaxText)
            throw std::invalid_argument("rlz finder: locate would report " + (wraps ? std::string("2^64 or more") : std::to_string(total)) +
                                        " hits, more than the " + std::to_string(kMaxText) +
                                        " the 32-bit device pipeline takes: lower max_hits (it is " + std::to_string(max_hits) +
                                        "; 0 means no cap) or send fewer patterns");
        const size_t Tout = (size_t)total, chunk = Tout < chunk_max ? Tout : chunk_max;
        const size_t need_out = need_hits + kLocateBytesPerHit * Tout + sizeof(TargetHit) * chunk + 4 * (q + 1) + (size_t(1) << 20);
        if (need_out > granted && arena_bytes_for(0) + need_out > ctx.arena.capacity()) {
            need = need_out;
            continue;
        }

        // the reported patterns' occurrences written at their offsets, sorted with the locate's digit plan, unpacked
        out_off.resize(q + 1);
        for (size_t j = 0; j <= q; ++j) out_off[j] = (uint32_t)hit_offsets[j];
        uint32_t *d_out_off = ctx.arena.alloc<uint32_t>(q + 1);
        upload_bytes(ctx, d_out_off, out_off.data(), sizeof(uint32_t) * (q + 1));
        uint64_t *keys[2] = {ctx.arena.alloc<uint64_t>(Tout), ctx.arena.alloc<uint64_t>(Tout)};
        uint32_t *vals[2] = {ctx.arena.alloc<uint32_t>(Tout), ctx.arena.alloc<uint32_t>(Tout)};
        const FindEmit e{d_scan[0], d_scan[1], d_off[0], d_off[1], d_out_off, keys[0], vals[0], (uint32_t)Tout};
        find_secondary_emit(ctx, f, av, d_hits[0], (uint32_t)T[0], batch.terms.pos, e);
        find_primary_emit(ctx, f, av, d_hits[1], (uint32_t)T[1], batch.terms.pos, e);
        int shifts[kLocateMaxPasses];
        const int npasses = rlz_locate_sort_shifts(h.decoded, q, shifts);
        int at;
        {
            ProfScope ps(ctx.profiler(), "rlz_find_sort", s, 24.0 * (double)Tout * npasses);
            at = radix_sort_pairs(keys, vals, Tout, shifts, npasses, ctx.arena, s, ctx.profiler());
        }
        hits.reset(static_cast<nolzss_rlz_target_hit *>(alloc_factor_block(sizeof(nolzss_rlz_target_hit) * Tout)));
        if (!hits) throw std::bad_alloc();
        TargetHit *d_recs = ctx.arena.alloc<TargetHit>(chunk);
        download_produced(ctx, "hits_d2h", hits.get(), d_recs, Tout, sizeof(TargetHit), chunk, [&](size_t c0, size_t c) {
            find_hit_records(ctx, f, keys[at] + c0, vals[at] + c0, (uint32_t)c, d_recs);
        });
        num_hits = Tout;
        return;
    }
    throw HipError("rlz finder: the arena of a query did not settle");
}

void finder_query(const nolzss_rlz_finder *h, const char *const *patterns, const size_t *pattern_lens, size_t q,
                  uint64_t max_hits, uint64_t *counts, uint64_t *hit_offsets, nolzss_rlz_target_hit **hits, size_t *num_hits) {
    const bool locate = hits != nullptr;
    if (locate) {
        *hits = nullptr;
        if (num_hits) *num_hits = 0;
    }
    if (!h) throw std::invalid_argument("handle is null");
    if (locate && (!hit_offsets || !num_hits)) throw std::invalid_argument("output pointer is null");
    if (q && !counts) throw std::invalid_argument("output pointer is null");
    // the sort key of a hit holds its pattern in the 31 bits above (position, strand)
    if (locate && q > 0x7fffffffull) throw std::invalid_argument("rlz finder: a locate takes at most 2^31 - 1 patterns per batch");
    Batch b;
    prepare_patterns(patterns, pattern_lens, q, b);
    for (size_t j = 0; j < q; ++j)
        if (pattern_lens[j] > h->M)
            throw std::invalid_argument("rlz finder: pattern " + std::to_string(j) + " has " + std::to_string(pattern_lens[j]) +
                                        " bases, the finder was opened with max_pattern_length " + std::to_string(h->M));
    if (h->archive->z != h->z || h->archive->lengths.size() != h->targets)
        throw std::invalid_argument("rlz finder: the archive has grown since the finder was opened (it held " +
                                    std::to_string(h->targets) + " targets in " + std::to_string(h->z) + " records, now " +
                                    std::to_string(h->archive->lengths.size()) + " in " + std::to_string(h->archive->z) +
                                    "): open a new finder");
    if (locate) hit_offsets[0] = 0;
    if (q == 0) return;
    if (h->z == 0) {  // no record, no occurrence: the device is not touched
        for (size_t j = 0; j < q; ++j) counts[j] = 0;
        if (locate)
            for (size_t j = 0; j <= q; ++j) hit_offsets[j] = 0;
        return;
    }
    TargetHitBlock block;
    size_t T = 0;
    DeviceRestore restore;
    Session ses(h->device, nullptr);
    Context &ctx = ses.ctx();
    try {
        ProfScope whole(ctx.profiler(), locate ? "rlz_finder_locate" : "rlz_finder_count", ctx.stream);
        query_finder(ctx, *h, b, q, max_hits, counts, locate ? hit_offsets : nullptr, block, T);
    } catch (...) {
        (void)hipStreamSynchronize(ctx.stream);  // nothing still reads the batch when it goes
        throw;
    }
    HIP_CHECK(hipStreamSynchronize(ctx.stream));
    HIP_CHECK(hipGetLastError());
    ctx.prof.collect();
    if (locate) {
        *hits = block.release();  // ownership moves to the caller
        *num_hits = T;
    }
}

void finder_kernel(const nolzss_rlz_finder &h, uint8_t **kernel, size_t *kernel_len, uint64_t **kstart, uint64_t **dstart,
                   size_t *intervals) {
    const size_t nI = (size_t)h.intervals, K = (size_t)h.K_len;
    HostBlock<uint8_t> h_K = host_block<uint8_t>(K);
    HostBlock<uint64_t> h_ks = host_block<uint64_t>(nI + 1), h_ds = host_block<uint64_t>(nI + 1);
    h_ks.get()[0] = 0;
    h_ds.get()[0] = h.decoded;
    if (h.z) {
        if (h.archive->z != h.z || h.archive->lengths.size() != h.targets)
            throw std::invalid_argument("rlz finder: the archive has grown since the finder was opened: open a new finder");
        std::vector<uint32_t> ks(nI + 1), ds(nI + 1);
        DeviceRestore restore;
        Session ses(h.device, nullptr);
        Context &ctx = ses.ctx();
        reserve_arena_for(ctx, 0, K + (size_t(4) << 20));
        uint8_t *d_X = ctx.arena.alloc<uint8_t>(K + 1);
        // (the bytes come from the archive again, as at the open: the finder keeps K packed)
        find_kernel_text(ctx, h.archive->view(), h.view.kstart, h.view.dstart, (uint32_t)nI, (uint32_t)K, false, kSeparator,
                         kSeparator, d_X);
        download_bytes(ctx, h_K.get(), d_X, K);
        download_bytes(ctx, ks.data(), h.view.kstart, sizeof(uint32_t) * (nI + 1));
        download_bytes(ctx, ds.data(), h.view.dstart, sizeof(uint32_t) * (nI + 1));
        ctx.prof.collect();
        for (size_t i = 0; i <= nI; ++i) {
            h_ks.get()[i] = ks[i];
            h_ds.get()[i] = ds[i];
        }
    }
    *kernel = h_K.release();
    *kernel_len = K;
    *kstart = h_ks.release();
    *dstart = h_ds.release();
    *intervals = nI;
}

}  // namespace

extern "C" {

int nolzss_rlz_finder_open(const nolzss_rlz_archive *archive, const nolzss_rlz_index *index, uint64_t max_pattern_length,
                           uint32_t prefix_syms, nolzss_rlz_finder **h) {
    return guarded([&] { finder_open(archive, index, max_pattern_length, prefix_syms, h); });
}

int nolzss_rlz_finder_info(const nolzss_rlz_finder *h, nolzss_rlz_finder_summary *info) {
    return guarded([&] {
        if (!h || !info) throw std::invalid_argument("handle or output pointer is null");
        std::memset(info, 0, sizeof *info);
        info->num_targets = h->targets;
        info->z = h->z;
        info->total_length = h->decoded;
        info->max_pattern_length = h->M;
        info->kernel_length = h->K_len;
        info->intervals = h->intervals;
        info->with_rc = h->with_rc ? 1 : 0;
        info->device = h->device;
        info->device_bytes = h->tables.bytes() + h->kindex.bytes() + h->sources.bytes();
    });
}

int nolzss_rlz_finder_count(const nolzss_rlz_finder *h, const char *const *patterns, const size_t *pattern_lens, size_t q,
                            uint64_t *counts) {
    return guarded([&] { finder_query(h, patterns, pattern_lens, q, 0, counts, nullptr, nullptr, nullptr); });
}

int nolzss_rlz_finder_locate(const nolzss_rlz_finder *h, const char *const *patterns, const size_t *pattern_lens,
                             size_t q, uint64_t max_hits, uint64_t *counts, uint64_t *hit_offsets,
                             nolzss_rlz_target_hit **hits, size_t *num_hits) {
    return guarded([&] {
        if (!hits) throw std::invalid_argument("output pointer is null");
        finder_query(h, patterns, pattern_lens, q, max_hits, counts, hit_offsets, hits, num_hits);
    });
}

int nolzss_rlz_finder_kernel(const nolzss_rlz_finder *h, uint8_t **kernel, size_t *kernel_len, uint64_t **kstart,
                             uint64_t **dstart, size_t *intervals) {
    return guarded([&] {
        if (!kernel || !kernel_len || !kstart || !dstart || !intervals) throw std::invalid_argument("output pointer is null");
        *kernel = nullptr;
        *kstart = *dstart = nullptr;
        *kernel_len = *intervals = 0;
        if (!h) throw std::invalid_argument("handle is null");
        finder_kernel(*h, kernel, kernel_len, kstart, dstart, intervals);
    });
}

int nolzss_rlz_finder_close(nolzss_rlz_finder *h) {
    return guarded([&] { delete h; });
}

}  // extern "C"
