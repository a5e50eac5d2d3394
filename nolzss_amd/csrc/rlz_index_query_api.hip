// rlz_index_query_api.hip -- nolzss_rlz_index_count / _locate: pattern batches queried against the relative-LZ index
// handle (part of the C ABI layer of libnolzss_hip.so, include/nolzss_hip.h; the kernels: rlz_locate.hip; DESIGN.md 5,
// "Relative-LZ index: pattern count and locate"; the handle and its match: rlz_index_api.hip).
#include "rlz_handles.hpp"

using namespace nolzss;
using namespace nolzss::api;

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

// device memory of a pattern batch of n positions and q patterns: the bytes, the packed words, the terminator table, and
// lo, cnt, rep, off; per hit: two key and two value arrays of the sort (24), its histograms (1/4), and the records of a
// chunk (16)
size_t nolzss::api::pattern_batch_bytes(size_t n, size_t q) { return 2 * n + 24 * q + (size_t(4) << 20); }

namespace {

using HitBlock = HostBlock<nolzss_rlz_hit>;
static_assert(sizeof(nolzss_rlz_hit) == sizeof(LocateHit) && sizeof(LocateHit) == 16, "the kernels write nolzss_rlz_hit");

// One batch of q >= 1 patterns against the handle, inside a session.  counts: q entries.  With hit_offsets (q + 1
// entries) the hits of every pattern with at most max_hits occurrences (0: no cap) come down too.
void query_patterns(Context &ctx, const nolzss_rlz_index &h, const Batch &b, size_t q, uint64_t max_hits, uint64_t *counts,
                    uint64_t *hit_offsets, HitBlock &hits, size_t &num_hits) {
    const size_t n = b.tcat.size();
    const bool locate = hit_offsets != nullptr;
    const uint32_t cap = hit_cap(max_hits);
    const size_t chunk_max = chunk_knob("NOLZSS_RLZ_LOCATE_CHUNK");
    std::vector<uint32_t> cnt(q);
    PackedText batch;
    uint32_t *d_lo = nullptr, *d_rep = nullptr;
    // the batch up, packed with the pattern ends as terminators, and searched: the counts come down once
    auto run_patterns = [&] {
        upload_and_pack(ctx, b, batch);
        d_lo = ctx.arena.alloc<uint32_t>(q);
        d_rep = ctx.arena.alloc<uint32_t>(q);
        uint32_t *d_cnt = ctx.arena.alloc<uint32_t>(q);
        rlz_index_patterns(ctx, h.view, batch, (uint32_t)q, cap, d_lo, d_cnt, d_rep);
        ProfScope ps(ctx.profiler(), "counts_d2h", ctx.stream, 4.0 * (double)q);
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
    // the arena for the hits (regrow_arena): the patterns are searched again in a slab that was replaced
    if (regrow_arena(ctx, pattern_batch_bytes(n, q) + kLocateBytesPerHit * T + sizeof(LocateHit) * chunk)) run_patterns();
    uint32_t *d_off = ctx.arena.alloc<uint32_t>(q);
    rlz_index_hit_offsets(ctx, d_rep, (uint32_t)q, d_off);
    const LocateSorted sorted = rlz_index_hits(ctx, h.view, (uint32_t)h.m, batch, (uint32_t)q, d_off, d_lo, (uint32_t)T);
    hits.reset(static_cast<nolzss_rlz_hit *>(alloc_factor_block(sizeof(nolzss_rlz_hit) * T)));
    if (!hits) throw std::bad_alloc();
    LocateHit *d_recs = ctx.arena.alloc<LocateHit>(chunk);
    download_produced(ctx, "hits_d2h", hits.get(), d_recs, T, sizeof(LocateHit), chunk,
                      [&](size_t c0, size_t c) { rlz_index_hit_records(ctx, sorted, c0, (uint32_t)c, d_recs); });
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
    with_index_session(h->device, locate ? "rlz_index_locate" : "rlz_index_count", [&](Context &ctx) {
        query_patterns(ctx, *h, b, q, max_hits, counts, locate ? hit_offsets : nullptr, block, T);
    });
    if (locate) {
        *hits = block.release();  // ownership moves to the caller
        *num_hits = T;
    }
}

}  // namespace

extern "C" {

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

int nolzss_debug_rlz_locate_shifts(uint64_t block_length, uint64_t q, int *shifts, int *npasses) {
    return guarded([&] {
        if (!shifts || !npasses) throw std::invalid_argument("output pointer is null");
        *npasses = rlz_locate_sort_shifts(block_length, q, shifts);
    });
}

}  // extern "C"
