// rlz_index_repeats_api.hip -- nolzss_rlz_index_repeat_count / _repeats: the maximal repeats of the reference itself,
// read off the resident arrays of the relative-LZ index handle (part of the C ABI layer of libnolzss_hip.so,
// include/nolzss_hip.h; the kernels: rlz_repeats.hip; DESIGN.md 5, "Relative-LZ index: maximal repeats"; the handle:
// rlz_index_api.hip).
#include "rlz_handles.hpp"

using namespace nolzss;
using namespace nolzss::api;

namespace {

static_assert(sizeof(nolzss_rlz_repeat) == sizeof(RepeatRec) && sizeof(RepeatRec) == 32, "the kernels write nolzss_rlz_repeat");
static_assert(sizeof(nolzss_rlz_hit) == sizeof(LocateHit) && sizeof(LocateHit) == 16, "the kernels write nolzss_rlz_hit");

// device memory of the flags over n ranks: the scanned left-context flags, the interval flags and their slots (4 each,
// one entry more for the first), and the scans' tile sums
size_t repeat_rank_bytes(size_t n) { return 12 * (n + 1) + (size_t(4) << 20); }
// per repeat: two key and two value arrays of the sort (24), first, count, rep and the palindrome byte (13), the hit
// offsets (4), the histograms (1/4), rounded up
constexpr size_t kRepeatBytesPerRecord = 44;

// min_length and min_count as the kernels take them: no LCP value and no interval reaches 2^32 - 1
uint32_t clamp32(uint64_t v) { return v >= 0xffffffffull ? 0xffffffffu : (uint32_t)v; }

// What a repeats query answers once its counts are known when the records or their hits do not fit the pipeline; empty
// when they do.  The sort key of a hit keeps its repeat in the 31 bits above (position, strand).
std::string repeats_refusal(uint64_t num_repeats, uint64_t total, uint64_t max_hits, uint64_t min_length) {
    if (num_repeats > 0x7fffffffull)
        return "rlz index: a repeats query reports at most 2^31 - 1 records, this one has " + std::to_string(num_repeats) +
               ": raise min_length (it is " + std::to_string(min_length) + ") or min_count";
    if (total <= kMaxText) return std::string();
    return "rlz index: repeats would report " + std::to_string(total) + " hits, more than the " + std::to_string(kMaxText) +
           " the 32-bit device pipeline takes: lower max_hits (it is " + std::to_string(max_hits) +
           "; 0 means no cap) or raise min_length (it is " + std::to_string(min_length) + ")";
}

// Stages 1 and 2 in the arena: the number of reported repeats comes down as one word.
struct RepeatFront {
    uint32_t *d_left = nullptr, *d_flag = nullptr, *d_slot = nullptr;
    uint32_t S = 0, min_len, min_count;
    RepeatFront(uint64_t min_length, uint64_t min_cnt) : min_len(clamp32(min_length)), min_count(clamp32(min_cnt)) {}
    void run(Context &ctx, const nolzss_rlz_index &h) {
        const size_t n = h.view.text.n;
        d_left = ctx.arena.alloc<uint32_t>(n + 1);
        d_flag = ctx.arena.alloc<uint32_t>(n);
        d_slot = ctx.arena.alloc<uint32_t>(n);
        uint32_t *d_total = ctx.arena.alloc<uint32_t>(1);
        rlz_repeat_flags(ctx, h.view, min_len, min_count, d_left, d_flag, d_slot, d_total);
        ProfScope ps(ctx.profiler(), "counts_d2h", ctx.stream, 4.0);
        download_bytes(ctx, &S, d_total, sizeof(uint32_t));
        if (S > n) throw HipError("rlz index: more repeats than ranks");
    }
    // ... again, in an arena that regrow_arena has emptied
    void rerun(Context &ctx, const nolzss_rlz_index &h) {
        const uint32_t before = S;
        run(ctx, h);
        if (S != before) throw HipError("rlz index: the repeats of a handle changed between two passes");
    }
    RepeatList list(Context &ctx, const nolzss_rlz_index &h, uint32_t cap) {
        return rlz_repeat_list(ctx, h.view, min_len, min_count, cap, d_left, d_flag, d_slot, S);
    }
};

// Inside a session.  res is filled as the results arrive: the records and hit_offsets once the counts are known, the
// hits last.  Returns the refusal of the totals: res then holds what had come down before it.
std::string query_repeats(Context &ctx, const nolzss_rlz_index &h, uint64_t min_length, uint64_t min_count, uint64_t max_hits,
                          nolzss_rlz_repeats_result &res) {
    const size_t n = h.view.text.n;
    const size_t chunk_max = chunk_knob("NOLZSS_RLZ_LOCATE_CHUNK");
    const uint32_t cap = hit_cap(max_hits);
    RepeatFront front(min_length, min_count);
    reserve_arena_for(ctx, 0, repeat_rank_bytes(n));
    front.run(ctx, h);
    const size_t S = front.S;
    std::string refusal = repeats_refusal(S, 0, max_hits, min_length);
    if (!refusal.empty()) return refusal;
    res.hit_offsets = calloc_array<uint64_t>(S + 1);
    if (S == 0) return refusal;
    const size_t rchunk = S < chunk_max ? S : chunk_max;
    const size_t list_bytes = repeat_rank_bytes(n) + kRepeatBytesPerRecord * S + sizeof(RepeatRec) * rchunk;
    // the arena for the list (regrow_arena): the flags are computed again in a slab that was replaced
    if (regrow_arena(ctx, list_bytes)) front.rerun(ctx, h);
    RepeatList list = front.list(ctx, h, cap);
    res.repeats = static_cast<nolzss_rlz_repeat *>(alloc_factor_block(sizeof(nolzss_rlz_repeat) * S));
    if (!res.repeats) throw std::bad_alloc();
    {
        RepeatRec *d_recs = ctx.arena.alloc<RepeatRec>(rchunk);
        download_produced(ctx, "repeats_d2h", res.repeats, d_recs, S, sizeof(RepeatRec), rchunk,
                          [&](size_t c0, size_t c) { rlz_repeat_records(ctx, h.view, list, c0, (uint32_t)c, d_recs); });
    }
    res.num_repeats = S;
    uint64_t total = 0;  // the hits to report, summed in 64 bits
    for (size_t j = 0; j < S; ++j) {
        res.hit_offsets[j] = total;
        if (res.repeats[j].count <= cap) total += res.repeats[j].count;
    }
    res.hit_offsets[S] = total;
    refusal = repeats_refusal(S, total, max_hits, min_length);
    if (total == 0 || !refusal.empty()) return refusal;
    const size_t T = (size_t)total, chunk = T < chunk_max ? T : chunk_max;
    // ... and for the hits: the flags and the list again in a slab that was replaced -- the records have come down and
    // are not written a second time
    if (regrow_arena(ctx, list_bytes + kLocateBytesPerHit * T + sizeof(LocateHit) * chunk)) {
        front.rerun(ctx, h);
        list = front.list(ctx, h, cap);
    }
    const LocateSorted sorted = rlz_repeat_hits(ctx, h.view, (uint32_t)h.m, list, (uint32_t)T);
    res.hits = static_cast<nolzss_rlz_hit *>(alloc_factor_block(sizeof(nolzss_rlz_hit) * T));
    if (!res.hits) throw std::bad_alloc();
    LocateHit *d_recs = ctx.arena.alloc<LocateHit>(chunk);
    download_produced(ctx, "hits_d2h", res.hits, d_recs, T, sizeof(LocateHit), chunk,
                      [&](size_t c0, size_t c) { rlz_index_hit_records(ctx, sorted, c0, (uint32_t)c, d_recs); });
    res.num_hits = T;
    return refusal;
}

void check_repeat_rules(const nolzss_rlz_index *h, uint64_t min_length, uint64_t min_count) {
    if (!h) throw std::invalid_argument("handle is null");
    if (min_length == 0) throw std::invalid_argument("rlz index: repeats need min_length >= 1");
    if (min_count < 2) throw std::invalid_argument("rlz index: repeats need min_count >= 2: a repeat occurs at least twice");
}

void index_repeat_count(const nolzss_rlz_index *h, uint64_t min_length, uint64_t min_count, uint64_t *num_repeats) {
    if (!num_repeats) throw std::invalid_argument("output pointer is null");
    *num_repeats = 0;
    check_repeat_rules(h, min_length, min_count);
    with_index_session(h->device, "rlz_index_repeat_count", [&](Context &ctx) {
        RepeatFront front(min_length, min_count);
        reserve_arena_for(ctx, 0, repeat_rank_bytes(h->view.text.n));
        front.run(ctx, *h);
        *num_repeats = front.S;
    });
}

void index_repeats(const nolzss_rlz_index *h, uint64_t min_length, uint64_t min_count, uint64_t max_hits,
                   nolzss_rlz_repeats_result *out) {
    if (!out) throw std::invalid_argument("output pointer is null");
    std::memset(out, 0, sizeof *out);
    check_repeat_rules(h, min_length, min_count);
    nolzss_rlz_repeats_result res;
    std::memset(&res, 0, sizeof res);
    std::string refusal;
    try {
        with_index_session(h->device, "rlz_index_repeats",
                           [&](Context &ctx) { refusal = query_repeats(ctx, *h, min_length, min_count, max_hits, res); });
    } catch (...) {
        nolzss_free_rlz_repeats_result(&res);
        throw;
    }
    *out = res;  // ownership moves to the caller: the records and the offsets also with the refusal of the hit total
    if (!refusal.empty()) throw std::invalid_argument(refusal);
}

}  // namespace

extern "C" {

int nolzss_rlz_index_repeat_count(const nolzss_rlz_index *h, uint64_t min_length, uint64_t min_count, uint64_t *num_repeats) {
    return guarded([&] { index_repeat_count(h, min_length, min_count, num_repeats); });
}

int nolzss_rlz_index_repeats(const nolzss_rlz_index *h, uint64_t min_length, uint64_t min_count, uint64_t max_hits,
                             nolzss_rlz_repeats_result *out) {
    return guarded([&] { index_repeats(h, min_length, min_count, max_hits, out); });
}

void nolzss_free_rlz_repeats_result(nolzss_rlz_repeats_result *r) {
    if (!r) return;
    free_block(r->repeats);
    free_block(r->hit_offsets);
    free_block(r->hits);
    std::memset(r, 0, sizeof *r);
}

int nolzss_debug_rlz_repeats_refusal(uint64_t num_repeats, uint64_t total_hits, uint64_t max_hits, uint64_t min_length) {
    return guarded([&] {
        const std::string refusal = repeats_refusal(num_repeats, total_hits, max_hits, min_length);
        if (!refusal.empty()) throw std::invalid_argument(refusal);
    });
}

int nolzss_debug_rlz_repeat_shifts(uint64_t block_length, int *shifts, int *npasses) {
    return guarded([&] {
        if (!shifts || !npasses) throw std::invalid_argument("output pointer is null");
        *npasses = rlz_repeat_sort_shifts(block_length, shifts);
    });
}

}  // extern "C"
