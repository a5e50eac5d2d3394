// debug_api.hip -- debug hooks (plans, intermediate arrays, primitives) and the stage profiler
// (part of the C ABI layer of libnolzss_hip.so, include/nolzss_hip.h; shared declarations: api_internal.hpp)
#include "api_internal.hpp"
#include "queues.hpp"
#include "sa_internal.hpp"

using namespace nolzss;
using namespace nolzss::api;

extern "C" {

int nolzss_debug_lpt_plan(const size_t *lens, size_t m, size_t bins, size_t *owners) {
    return guarded([&] {
        if ((m && (!lens || !owners)) || bins == 0) throw std::invalid_argument("bad plan arguments");
        const std::vector<size_t> o = lpt_owner(std::vector<size_t>(lens, lens + m), bins);
        for (size_t j = 0; j < m; ++j) owners[j] = o[j];
    });
}

int nolzss_debug_batch_plan(const size_t *lens, size_t m, size_t n_dev, int with_rc, int32_t *chunk_of, int32_t *device_of,
                            size_t *n_chunks) {
    return guarded([&] {
        if (!lens || !chunk_of || !device_of || n_dev == 0) throw std::invalid_argument("null argument");
        BatchPlan bp = plan_batch(lens, m, with_rc != 0);
        for (size_t j = 0; j < m; ++j) chunk_of[j] = device_of[j] = -1;
        for (size_t k = 0; k < bp.chunks.size(); ++k)
            for (size_t j : bp.chunks[k]) {
                if (chunk_of[j] != -1) throw std::logic_error("batch plan: a record sits in two runs");
                chunk_of[j] = (int32_t)k;
            }
        const std::vector<std::vector<size_t>> plan = lpt_plan_singles(bp.singles, lens, n_dev);
        for (size_t d = 0; d < n_dev; ++d)
            for (size_t j : plan[d]) {
                if (chunk_of[j] != -1 || device_of[j] != -1) throw std::logic_error("batch plan: a record is dealt twice");
                device_of[j] = (int32_t)d;
            }
        if (n_chunks) *n_chunks = bp.chunks.size();
    });
}

int nolzss_debug_trim_arenas(int device, size_t *released) {
    return guarded([&] {
        HIP_CHECK(hipSetDevice(device));
        const size_t r = trim_idle_arenas(device, nullptr);
        if (released) *released = r;
    });
}

void nolzss_debug_batch_counters(uint64_t *merged_records, uint64_t *single_records) {
    if (merged_records) *merged_records = g_merged_records.load();
    if (single_records) *single_records = g_single_records.load();
}

int nolzss_profile_enable(int device, int on) {
    return guarded([&] {
        Session ses(device, nullptr);
        ses.ctx().prof.enable(on != 0);
    });
}

int nolzss_profile_reset(int device) {
    return guarded([&] {
        Session ses(device, nullptr);
        ses.ctx().prof.reset();
    });
}

int nolzss_profile_report(int device, char *buf, size_t cap) {
    return guarded([&] {
        if (!buf || cap == 0) throw std::invalid_argument("buffer is null");
        Session ses(device, nullptr);
        std::string text;
        for (const auto &kv : ses.ctx().prof.stats()) {
            char line[256];
            snprintf(line, sizeof line, "%s %llu %.6f %.0f\n", kv.first.c_str(),
                     (unsigned long long)kv.second.count, kv.second.total_ms, kv.second.bytes);
            text += line;
        }
        const size_t len = std::min(text.size(), cap - 1);
        std::memcpy(buf, text.data(), len);
        buf[len] = 0;
    });
}

int nolzss_debug_arrays(const uint8_t *text, size_t n, int device, uint32_t *sa, uint32_t *isa, uint32_t *lcp,
                        uint32_t *lstar) {
    return guarded([&] {
        check_text_args(text, n, 0);
        if (n == 0) return;
        Session ses(device, nullptr);
        DebugOut dbg;
        dbg.sa = sa;
        dbg.isa = isa;
        dbg.lcp = lcp;
        dbg.lstar = lstar;
        run_plain_host(ses.ctx(), text, n, 0, nullptr, &dbg);
        HIP_CHECK(hipStreamSynchronize(ses.ctx().stream));
        if (isa)
            for (size_t i = 0; i < n; ++i) isa[i] -= 1u;  // the device array holds rank + 1
    });
}

int nolzss_debug_position_factors(const uint8_t *text, size_t n, int device, nolzss_factor *out) {
    return guarded([&] {
        check_text_args(text, n, 0);
        if (n == 0) return;
        if (!out) throw std::invalid_argument("output pointer is null");
        Session ses(device, nullptr);
        Context &ctx = ses.ctx();
        reserve_arena_for(ctx, n, n + n * (sizeof(nolzss_factor) + sizeof(uint32_t)));  // text, records, their positions
        uint8_t *d_text = ctx.arena.alloc<uint8_t>(n);
        upload_bytes(ctx, d_text, text, n);
        DebugOut dbg;
        dbg.records = out;
        ArenaRewind rewind(ctx.arena);
        ChainRequest rq;
        run_plain(ctx, d_text, n, 0, rq, &dbg);
        deliver(ctx, rq);
    });
}

int nolzss_debug_rc_arrays(const uint8_t *S, size_t S_len, int device, int want_plain, uint32_t *sa, uint32_t *isa,
                           uint32_t *lcp, uint32_t *code, uint32_t *plain, nolzss_factor *records, uint32_t *counters) {
    return guarded([&] {
        if (S_len && !S) throw std::invalid_argument("text pointer is null");
        if (S_len > kMaxText) throw std::invalid_argument("text too long: the device pipeline uses 32-bit indices");
        if (counters) std::fill(counters, counters + 5, 0u);
        if (!rc_guards(S_len, 0)) return;
        const size_t m = S_len, N = m / 2 - 1;
        Session ses(device, nullptr);
        Context &ctx = ses.ctx();
        // the upload path of run_rc_host, with room for the plain by-product (by rank and in text order, as
        // dna_w_rc_common asks for it) and for the records of every position
        reserve_arena_for(ctx, m, m + (want_plain ? 4 * m + 4 * N + (size_t(32) << 20) : 0) +
                                      (records ? N * (sizeof(nolzss_factor) + sizeof(uint32_t)) : 0));
        uint8_t *d_S = ctx.arena.alloc<uint8_t>(m);
        upload_bytes(ctx, d_S, S, m);
        RcDebugOut dbg;
        dbg.sa = sa;
        dbg.isa = isa;
        dbg.lcp = lcp;
        dbg.code = code;
        dbg.plain = want_plain ? plain : nullptr;
        dbg.records = records;
        RcPlainOut plain_out;
        ChainRequest rq;
        run_rc_pipeline(ctx, d_S, m, 0, rq, want_plain ? &plain_out : nullptr, &dbg);
        HIP_CHECK(hipStreamSynchronize(ctx.stream));
        ctx.prof.collect();
        if (isa)
            for (size_t i = 0; i < N; ++i) isa[i] -= 1u;  // the device array holds rank + 1
        if (counters) {
            counters[0] = dbg.far_ranks;
            counters[1] = dbg.exact_from_tiles;
            counters[2] = dbg.exact_total;
            counters[3] = dbg.compact;
            counters[4] = dbg.pending_relaunch;
        }
    });
}

int nolzss_debug_sort_pairs(uint64_t *keys, uint32_t *vals, size_t n, int device) {
    return guarded([&] {
        if (n == 0) return;
        if (!keys || !vals) throw std::invalid_argument("null array");
        Session ses(device, nullptr);
        Context &ctx = ses.ctx();
        ctx.arena.reserve(n * 28 + (size_t(64) << 20));
        const size_t mark = ctx.arena.mark();
        uint64_t *k[2] = {ctx.arena.alloc<uint64_t>(n), ctx.arena.alloc<uint64_t>(n)};
        uint32_t *v[2] = {ctx.arena.alloc<uint32_t>(n), ctx.arena.alloc<uint32_t>(n)};
        HIP_CHECK(hipMemcpyAsync(k[0], keys, n * 8, hipMemcpyHostToDevice, ctx.stream));
        HIP_CHECK(hipMemcpyAsync(v[0], vals, n * 4, hipMemcpyHostToDevice, ctx.stream));
        const int shifts[8] = {0, 8, 16, 24, 32, 40, 48, 56};
        const int cur = radix_sort_pairs(k, v, n, shifts, 8, ctx.arena, ctx.stream, ctx.profiler());
        HIP_CHECK(hipMemcpyAsync(keys, k[cur], n * 8, hipMemcpyDeviceToHost, ctx.stream));
        HIP_CHECK(hipMemcpyAsync(vals, v[cur], n * 4, hipMemcpyDeviceToHost, ctx.stream));
        HIP_CHECK(hipStreamSynchronize(ctx.stream));
        ctx.prof.collect();
        ctx.arena.rewind(mark);
    });
}

int nolzss_debug_local_sort(const uint32_t *words, const uint32_t *values, size_t n, const uint32_t *starts, size_t nb,
                            int shift0, int npass, int key35, int want_regroup, int device, uint32_t *words_out,
                            uint32_t *values_out, uint32_t *lcp, uint32_t *new_slot, uint32_t *new_grp, uint32_t *survivors,
                            uint32_t *status) {
    return guarded([&] {
        if (!words || !values || !starts || !words_out || !values_out || !status) throw std::invalid_argument("null argument");
        if (want_regroup && (!lcp || !new_slot || !new_grp || !survivors)) throw std::invalid_argument("null regroup output");
        if (n == 0 || n >= (size_t(1) << 31)) throw std::invalid_argument("1 .. 2^31 - 1 pairs");
        if (nb == 0 || nb > 65535) throw std::invalid_argument("1 .. 65535 buckets");
        if (starts[0] != 0 || starts[nb] != n) throw std::invalid_argument("the bucket starts do not run from 0 to n");
        for (size_t k = 0; k < nb; ++k)
            if (starts[k] > starts[k + 1]) throw std::invalid_argument("the bucket starts do not ascend");
        if (npass < 2 || npass > 3) throw std::invalid_argument("two or three digits");
        if (key35 ? (shift0 != kP35TagBits || npass != 2) : (shift0 < 0 || shift0 + 8 * npass > 24))
            throw std::invalid_argument("the digits do not lie between the tag and bit 24 (35-bit key: shift0 5, two digits)");
        if (want_regroup && (npass != 2 || (!key35 && shift0 != kP16TagBits)))
            throw std::invalid_argument("the regroup on the way is for the two key layouts of round 0");
        if (want_regroup && (nb * 256) % 1024 != 0) throw std::invalid_argument("the regroup on the way needs a multiple of 1024 sub-buckets");

        Session ses(device, nullptr);
        Context &ctx = ses.ctx();
        const size_t subs = nb * 256, tiles = n / kSortTile + nb + 1;
        ctx.arena.reserve(7 * (n * 4 + 256) + 1024 * (2 * tiles + std::min(n, subs)) + 16 * subs + 128 * tiles + (size_t(64) << 20));
        ArenaRewind rewind(ctx.arena);
        hipStream_t s = ctx.stream;
        uint32_t *k[2] = {ctx.arena.alloc<uint32_t>(n), ctx.arena.alloc<uint32_t>(n)};
        uint32_t *v[2] = {ctx.arena.alloc<uint32_t>(n), ctx.arena.alloc<uint32_t>(n)};
        HIP_CHECK(hipMemcpyAsync(k[0], words, n * 4, hipMemcpyHostToDevice, s));
        HIP_CHECK(hipMemcpyAsync(v[0], values, n * 4, hipMemcpyHostToDevice, s));
        Round0Regroup rg;
        if (want_regroup) {
            rg.lcp = ctx.arena.alloc<uint32_t>(n);
            rg.new_slot = ctx.arena.alloc<uint32_t>(n);
            rg.new_grp = ctx.arena.alloc<uint32_t>(n);
            rg.d_total = ctx.arena.alloc<uint32_t>(4);
        }
        LocalSortReport rep;
        rep.regroup_any_size = true;
        debug_local_sort(k, v, n, starts, (uint32_t)nb, shift0, npass, key35 != 0, want_regroup ? &rg : nullptr, rep, ctx.arena, s);
        *status = (rep.fused_done ? NOLZSS_LOCAL_SORT_FUSED : 0u) | (rep.lookback_gave_up ? NOLZSS_LOCAL_SORT_LOOKBACK_GAVE_UP : 0u) |
                  (rep.lane_order_failed ? NOLZSS_LOCAL_SORT_LANE_ORDER : 0u) | (rep.listed << NOLZSS_LOCAL_SORT_LISTED_SHIFT);
        if (!rep.fused_done) HIP_CHECK(hipMemcpyAsync(words_out, k[0], n * 4, hipMemcpyDeviceToHost, s));  // (else: never written)
        HIP_CHECK(hipMemcpyAsync(values_out, v[0], n * 4, hipMemcpyDeviceToHost, s));
        if (rep.fused_done) {
            HIP_CHECK(hipMemcpyAsync(survivors, rg.d_total, 4, hipMemcpyDeviceToHost, s));
            HIP_CHECK(hipStreamSynchronize(s));
            if (*survivors > n) throw std::logic_error("debug_local_sort: more tied elements than pairs");
            HIP_CHECK(hipMemcpyAsync(lcp, rg.lcp, n * 4, hipMemcpyDeviceToHost, s));
            HIP_CHECK(hipMemcpyAsync(new_slot, rg.new_slot, (size_t)*survivors * 4, hipMemcpyDeviceToHost, s));
            HIP_CHECK(hipMemcpyAsync(new_grp, rg.new_grp, (size_t)*survivors * 4, hipMemcpyDeviceToHost, s));
        }
        HIP_CHECK(hipStreamSynchronize(s));
    });
}

int nolzss_debug_text_order(const uint32_t *idx, const uint32_t *val, const uint64_t *packed, size_t count, size_t n_out,
                            uint32_t flags, uint32_t fill, size_t list_cap, uint32_t code_max, const uint32_t *rec_ends,
                            size_t n_recs, int device, uint32_t *out, uint32_t *out2, uint16_t *narrow, uint64_t *list_items,
                            uint32_t *idx_after, uint32_t *val_after, uint32_t *report) {
    return guarded([&] {
        const bool permute = flags & NOLZSS_TEXT_ORDER_PERMUTE_PACKED, want_out2 = permute || (flags & NOLZSS_TEXT_ORDER_OUT2),
                   want_narrow = flags & NOLZSS_TEXT_ORDER_NARROW;
        if (!out || !report || (count && !idx) || (want_out2 && !out2)) throw std::invalid_argument("null argument");
        if (count && (permute ? !packed : (!val || !idx_after || !val_after))) throw std::invalid_argument("null argument");
        if (flags >> 6) throw std::invalid_argument("unknown flag");
        if (n_out == 0 || n_out >= (size_t(1) << 32) || count >= (size_t(1) << 32)) throw std::invalid_argument("n_out 1 .. 2^32 - 1, count below 2^32");
        if (permute && (want_narrow || rec_ends || count != n_out))
            throw std::invalid_argument("permute_packed takes a permutation of [0, count) and neither codes of 16 bits nor records");
        if (want_narrow && (!want_out2 || !narrow || (list_cap && !list_items) || code_max == 0 || code_max > 0xffffu || list_cap >= (size_t(1) << 32)))
            throw std::invalid_argument("the 16-bit codes need out2, their array, a list and a saturation value of 1 .. 0xffff");
        if (rec_ends) {
            if (n_recs == 0 || count != n_out || rec_ends[n_recs - 1] != n_out) throw std::invalid_argument("the record ends do not end at count = n_out");
            for (size_t k = 0; k + 1 < n_recs; ++k)
                if (rec_ends[k] >= rec_ends[k + 1]) throw std::invalid_argument("the record ends do not ascend");
        }
        // A permutation is the contract of the forms that assemble windows of the target (count == n_out beyond 2^22 pairs,
        // a plan, permute_packed): checked here, before anything is launched.  Elsewhere idx must be free of duplicates below
        // n_out (the plain scatter is a race on them), which is the caller's business: any winner stays in bounds.
        if (permute || rec_ends || (count == n_out && count > (size_t(1) << 22))) {
            std::vector<uint64_t> seen((count + 63) / 64, 0);
            for (size_t k = 0; k < count; ++k) {
                const uint32_t i = idx[k];
                if (i >= count || (seen[i >> 6] >> (i & 63) & 1)) throw std::invalid_argument("idx is not a permutation of [0, count)");
                seen[i >> 6] |= uint64_t(1) << (i & 63);
            }
        }
        std::fill(report, report + NOLZSS_TEXT_ORDER_REPORT_WORDS, 0u);
        static_assert((int)TextOrderForm::kPacked == NOLZSS_TEXT_ORDER_FORM_PACKED &&
                          (int)TextOrderForm::kPermuteWindows == NOLZSS_TEXT_ORDER_FORM_PERMUTE_WINDOWS,
                      "the header's values are the enum's");

        Session ses(device, nullptr);
        Context &ctx = ses.ctx();
        hipStream_t s = ctx.stream;
        // the caller's pairs and their scratch (20 bytes per pair; permute_packed: 12), the targets (10 bytes each with the
        // list), what the largest form takes on top (permute_packed 12 + 1/4, the window permutation that keeps both inputs
        // 8 + 1/2, the packed form 8 + 1/8 and then the histogram form 12 + 1/4 bytes per pair), the tables of a plan (1 KiB
        // of counters and 48 bytes of descriptor per tile -- every 4096 pairs and up to two more per record --, 12 + 8 bytes
        // per window and record)
        const size_t tiles = count / kSortTile + 2 * n_recs + 2;
        ctx.arena.reserve(count * 34 + n_out * 10 + list_cap * 8 + tiles * (4 * 256 + 4 * kSegDescWords + 64) + (size_t(64) << 20));
        ArenaRewind rewind(ctx.arena);
        uint32_t *d_out = ctx.arena.alloc<uint32_t>(n_out), *d_out2 = ctx.arena.alloc<uint32_t>(n_out);
        HIP_CHECK(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(d_out), (int)fill, n_out, s));
        HIP_CHECK(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(d_out2), (int)fill, n_out, s));
        LstarCodes codes;
        if (want_narrow) {
            codes.narrow = ctx.arena.alloc<uint16_t>(n_out + 8);  // (padded as alloc_lstar pads it)
            codes.list.cap = (uint32_t)list_cap;
            codes.list.items = ctx.arena.alloc<uint64_t>(std::max<size_t>(list_cap, 1));
            codes.list.count = ctx.arena.alloc<uint32_t>(1);
            codes.list.max = code_max;
            HIP_CHECK(hipMemsetD16Async(reinterpret_cast<hipDeviceptr_t>(codes.narrow), (unsigned short)fill, n_out + 8, s));
            HIP_CHECK(hipMemsetAsync(codes.list.count, 0, sizeof(uint32_t), s));
        }
        TextOrderReport rep;
        bool result = true, plan_made = false;
        const size_t room = std::max<size_t>(count, 1);
        if (permute) {
            uint32_t *d_idx = ctx.arena.alloc<uint32_t>(room);
            uint64_t *d_packed = ctx.arena.alloc<uint64_t>(room);
            HIP_CHECK(hipMemcpyAsync(d_idx, idx, count * 4, hipMemcpyHostToDevice, s));
            HIP_CHECK(hipMemcpyAsync(d_packed, packed, count * 8, hipMemcpyHostToDevice, s));
            permute_packed(d_idx, d_packed, count, d_out, d_out2, ctx.arena, s, ctx.profiler(), &rep);
        } else {
            uint32_t *d_idx[2] = {ctx.arena.alloc<uint32_t>(room), ctx.arena.alloc<uint32_t>(room)};
            uint32_t *d_val[2] = {ctx.arena.alloc<uint32_t>(room), ctx.arena.alloc<uint32_t>(2 * room)};  // (two values: 64-bit words)
            uint32_t *const idx0 = d_idx[0], *const val0 = d_val[0];  // (the function may repoint its arrays)
            HIP_CHECK(hipMemcpyAsync(idx0, idx, count * 4, hipMemcpyHostToDevice, s));
            HIP_CHECK(hipMemcpyAsync(val0, val, count * 4, hipMemcpyHostToDevice, s));
            RecordScatterPlan plan;
            if (rec_ends) plan_made = record_scatter_plan(std::vector<uint32_t>(rec_ends, rec_ends + n_recs), (uint32_t)n_out, ctx.arena, s, plan);
            result = bucketed_scatter(d_idx, d_val, count, d_out, (uint32_t)n_out, ctx.arena, s, ctx.profiler(),
                                      flags & NOLZSS_TEXT_ORDER_KEEP_INPUT, flags & NOLZSS_TEXT_ORDER_KEEP_VAL, plan_made ? &plan : nullptr,
                                      want_out2 ? d_out2 : nullptr, flags & NOLZSS_TEXT_ORDER_SHORT_CODES, want_narrow ? &codes : nullptr, &rep);
            HIP_CHECK(hipMemcpyAsync(idx_after, idx0, count * 4, hipMemcpyDeviceToHost, s));
            HIP_CHECK(hipMemcpyAsync(val_after, val0, count * 4, hipMemcpyDeviceToHost, s));
        }
        HIP_CHECK(hipMemcpyAsync(out, d_out, n_out * 4, hipMemcpyDeviceToHost, s));
        if (out2) HIP_CHECK(hipMemcpyAsync(out2, d_out2, n_out * 4, hipMemcpyDeviceToHost, s));
        uint32_t listed = 0;
        if (want_narrow) {
            HIP_CHECK(hipMemcpyAsync(narrow, codes.narrow, n_out * 2, hipMemcpyDeviceToHost, s));
            HIP_CHECK(hipMemcpyAsync(&listed, codes.list.count, 4, hipMemcpyDeviceToHost, s));
            HIP_CHECK(hipStreamSynchronize(s));
            HIP_CHECK(hipMemcpyAsync(list_items, codes.list.items, std::min<size_t>(listed, list_cap) * 8, hipMemcpyDeviceToHost, s));
        }
        HIP_CHECK(hipStreamSynchronize(s));
        ctx.prof.collect();
        report[0] = (uint32_t)rep.form;
        report[1] = rep.packed_tried;
        report[2] = rep.escaped;
        report[3] = rep.list_overflow;
        report[4] = rep.lookback_gave_up;
        report[5] = (uint32_t)rep.nbits;
        report[6] = (uint32_t)rep.wb;
        report[7] = (uint32_t)rep.partition_passes;
        report[8] = result;
        report[9] = plan_made;
        report[10] = listed;
    });
}

int nolzss_debug_group_sort(const uint8_t *text, size_t n, uint32_t *sa, const uint32_t *slot, const uint32_t *grp, size_t m,
                            uint32_t h0, int pivot, uint32_t max_rounds, uint32_t depth_cap, const uint32_t *lcp_mark, int device,
                            uint32_t *out_lo, uint32_t *lcp_list, uint32_t *min_depth, uint32_t *info) {
    return guarded([&] {
        if (!text || !sa || !min_depth || (m && (!slot || !grp || !out_lo || !lcp_list))) throw std::invalid_argument("null argument");
        if (n == 0 || n > kMaxText) throw std::invalid_argument("1 .. 2^32 - 2^19 - 1 symbols");
        if (m > n) throw std::invalid_argument("more list entries than suffixes");
        if (max_rounds > kGroupSortRounds) throw std::invalid_argument("more rounds than the kernels' budget");
        // the list as the kernels rely on it: ascending slots, every group on consecutive list positions and on the slots
        // from its head slot on, at least two members, every suffix below n
        for (size_t a = 0, first = 0; a < m; ++a) {
            const uint32_t g = grp[a], s = slot[a];
            if (g > s || s >= n) throw std::invalid_argument("a list entry with grp <= slot < n violated");
            if (sa[s] >= n) throw std::invalid_argument("a listed slot holds no suffix of the text");
            const bool head = a == 0 || grp[a - 1] != g;
            if (a > 0 && s <= slot[a - 1]) throw std::invalid_argument("the list is not in ascending slot order");
            if (head) first = a;
            if (s != g + (a - first)) throw std::invalid_argument("a group does not hold the slots from its head slot on");
            if ((a + 1 == m || grp[a + 1] != g) && a == first) throw std::invalid_argument("a listed group of one member");
        }
        *min_depth = 0xffffffffu;
        Session ses(device, nullptr);
        Context &ctx = ses.ctx();
        hipStream_t s = ctx.stream;
        // text and packed text, sa and the marks, the list and its outputs, three queues of two arrays (a region per shard)
        ctx.arena.reserve(n * 12 + m * 16 + 24 * (m + 256 * (size_t)kQShards) + (size_t(64) << 20));
        ArenaRewind rewind(ctx.arena);
        uint8_t *d_text = ctx.arena.alloc<uint8_t>(n);
        upload_bytes(ctx, d_text, text, n);
        const PackedText packed = pack_text(ctx, d_text, n);
        if (info) {
            info[0] = (uint32_t)packed.bits;
            info[1] = packed.terms.count;
            info[2] = packed.segmented;
        }
        // (what suffix_array.hip refuses in front of these rounds: the terminator index travels in 16 bits)
        if (packed.terms.count > 0x10000u) throw std::invalid_argument("at most 65536 terminators");
        if (m == 0) return;
        uint32_t *d_sa = ctx.arena.alloc<uint32_t>(n), *d_mark = lcp_mark ? ctx.arena.alloc<uint32_t>(n) : nullptr;
        uint32_t *d_slot = ctx.arena.alloc<uint32_t>(m), *d_grp = ctx.arena.alloc<uint32_t>(m);
        uint32_t *d_lo = ctx.arena.alloc<uint32_t>(m), *d_lcp = ctx.arena.alloc<uint32_t>(m), *d_depth = ctx.arena.alloc<uint32_t>(1);
        HIP_CHECK(hipMemcpyAsync(d_sa, sa, n * 4, hipMemcpyHostToDevice, s));
        if (lcp_mark) HIP_CHECK(hipMemcpyAsync(d_mark, lcp_mark, n * 4, hipMemcpyHostToDevice, s));
        HIP_CHECK(hipMemcpyAsync(d_slot, slot, m * 4, hipMemcpyHostToDevice, s));
        HIP_CHECK(hipMemcpyAsync(d_grp, grp, m * 4, hipMemcpyHostToDevice, s));
        group_sort_rounds(ctx, packed, d_slot, d_grp, (uint32_t)m, d_sa, h0, pivot != 0, max_rounds, depth_cap, d_mark, d_lo, d_lcp, d_depth);
        HIP_CHECK(hipMemcpyAsync(sa, d_sa, n * 4, hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipMemcpyAsync(out_lo, d_lo, m * 4, hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipMemcpyAsync(lcp_list, d_lcp, m * 4, hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipMemcpyAsync(min_depth, d_depth, 4, hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipStreamSynchronize(s));
        ctx.prof.collect();
    });
}

int nolzss_debug_direct_round(const uint8_t *text, size_t n, uint32_t *sa, const uint32_t *slot, const uint32_t *grp, size_t m,
                              uint32_t h0, uint32_t cap, uint32_t flags, const uint32_t *lcp_in, uint32_t fill, int device,
                              uint32_t *lcp, uint32_t *rank_by_slot, uint32_t *new_slot, uint32_t *new_grp, uint32_t *new_m,
                              uint32_t *min_depth, uint32_t *info) {
    return guarded([&] {
        if (!text || !sa || !lcp_in || !lcp || !rank_by_slot || !new_m || !min_depth || (m && (!slot || !grp || !new_slot || !new_grp)))
            throw std::invalid_argument("null argument");
        if (n == 0 || n > kMaxText) throw std::invalid_argument("1 .. 2^32 - 2^19 - 1 symbols");
        if (m > n) throw std::invalid_argument("more list entries than suffixes");
        if (flags & ~(uint32_t)(NOLZSS_DIRECT_ROUND_NO_STRAGGLERS | NOLZSS_DIRECT_ROUND_TIMED | NOLZSS_DIRECT_ROUND_WITH_RANKS))
            throw std::invalid_argument("an unknown flag");
        // (32 words of text, the deepest cap NOLZSS_REFINE_WORDS allows: 1024 symbols at 2 bits here, where the width is not
        // known yet; once more behind the packing, for the width the text has)
        if (cap <= h0 || cap - h0 > 32u * 32u) throw std::invalid_argument("h0 < cap <= h0 + 32 words of text");
        // the list as the kernel relies on it: ascending slots, every group on consecutive list positions and on the slots
        // from its head slot on, at least two members (any number of them), every suffix below n and h0 symbols long
        for (size_t a = 0, first = 0; a < m; ++a) {
            const uint32_t g = grp[a], s = slot[a];
            if (g > s || s >= n) throw std::invalid_argument("a list entry with grp <= slot < n violated");
            if (sa[s] >= n || (uint64_t)sa[s] + h0 > n) throw std::invalid_argument("a listed slot holds no suffix of h0 symbols");
            const bool head = a == 0 || grp[a - 1] != g;
            if (a > 0 && s <= slot[a - 1]) throw std::invalid_argument("the list is not in ascending slot order");
            if (head) first = a;
            if (s != g + (a - first)) throw std::invalid_argument("a group does not hold the slots from its head slot on");
            if ((a + 1 == m || grp[a + 1] != g) && a == first) throw std::invalid_argument("a listed group of one member");
        }
        *new_m = 0;
        min_depth[0] = min_depth[1] = 0xffffffffu;
        min_depth[2] = 0;
        Session ses(device, nullptr);
        Context &ctx = ses.ctx();
        hipStream_t s = ctx.stream;
        // text and packed text, sa / lcp / ranks, the two lists, a region of kRefineThreads entries per tile (slot and head)
        ctx.arena.reserve(n * 16 + m * 16 + 2 * 4 * (size_t)kRefineThreads * (m / kRefineTile + 1) + (size_t(64) << 20));
        ArenaRewind rewind(ctx.arena);
        uint8_t *d_text = ctx.arena.alloc<uint8_t>(n);
        upload_bytes(ctx, d_text, text, n);
        const PackedText packed = pack_text(ctx, d_text, n);
        // (a caller whose groups do not agree on h0 symbols in front of their terminators can send a member up to cap - h0
        // symbols past the end of the text, 32 words of it at the most, and a fetch takes kRefineWords + 1: they land here,
        // not beyond the padding of the packed text, which is the arena's last allocation so far)
        (void)ctx.arena.alloc<uint64_t>(32 + kRefineWords + 1);
        if (info) {
            info[0] = (uint32_t)packed.bits;
            info[1] = packed.terms.count;
            info[2] = packed.segmented;
        }
        // (what suffix_array.hip refuses in front of the direct rounds: the terminator index travels in 16 bits.  Only a
        // mirror of that guard: pack_text makes at most 251 entries of a text that arrives as bytes.)
        if (packed.terms.count > 0x10000u) throw std::invalid_argument("at most 65536 terminators");
        if (cap - h0 > 32u * (64u / (uint32_t)packed.bits)) throw std::invalid_argument("h0 < cap <= h0 + 32 words of text");
        uint32_t *d_sa = ctx.arena.alloc<uint32_t>(n), *d_lcp = ctx.arena.alloc<uint32_t>(n), *d_rank = ctx.arena.alloc<uint32_t>(n);
        HIP_CHECK(hipMemcpyAsync(d_lcp, lcp_in, n * 4, hipMemcpyHostToDevice, s));
        HIP_CHECK(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(d_rank), (int)fill, n, s));
        if (m > 0) {
            uint32_t *d_slot = ctx.arena.alloc<uint32_t>(m), *d_grp = ctx.arena.alloc<uint32_t>(m);
            uint32_t *d_new_slot = ctx.arena.alloc<uint32_t>(m), *d_new_grp = ctx.arena.alloc<uint32_t>(m);
            uint32_t *d_out = ctx.arena.alloc<uint32_t>(4);  // the new m, min_depth[3]
            HIP_CHECK(hipMemcpyAsync(d_sa, sa, n * 4, hipMemcpyHostToDevice, s));
            HIP_CHECK(hipMemcpyAsync(d_slot, slot, m * 4, hipMemcpyHostToDevice, s));
            HIP_CHECK(hipMemcpyAsync(d_grp, grp, m * 4, hipMemcpyHostToDevice, s));
            direct_round_launch(ctx, packed, d_slot, d_grp, (uint32_t)m, d_sa, d_lcp, (flags & NOLZSS_DIRECT_ROUND_WITH_RANKS) ? d_rank : nullptr,
                                h0, cap, (flags & NOLZSS_DIRECT_ROUND_NO_STRAGGLERS) != 0, (flags & NOLZSS_DIRECT_ROUND_TIMED) != 0,
                                d_new_slot, d_new_grp, d_out, d_out + 1);
            uint32_t out4[4] = {0, 0, 0, 0};
            ctx.read_back(d_out, out4, 4);
            if (out4[0] > m) throw HipError("direct round: more survivors than list entries");
            *new_m = out4[0];
            for (int k = 0; k < 3; ++k) min_depth[k] = out4[k + 1];
            HIP_CHECK(hipMemcpyAsync(sa, d_sa, n * 4, hipMemcpyDeviceToHost, s));
            HIP_CHECK(hipMemcpyAsync(new_slot, d_new_slot, (size_t)out4[0] * 4, hipMemcpyDeviceToHost, s));
            HIP_CHECK(hipMemcpyAsync(new_grp, d_new_grp, (size_t)out4[0] * 4, hipMemcpyDeviceToHost, s));
        }
        HIP_CHECK(hipMemcpyAsync(lcp, d_lcp, n * 4, hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipMemcpyAsync(rank_by_slot, d_rank, n * 4, hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipStreamSynchronize(s));
        ctx.prof.collect();
    });
}

int nolzss_debug_chain(const uint32_t *codes, size_t n, size_t start_pos, int width, uint32_t poison, const uint64_t *list,
                       size_t list_len, size_t listed, uint32_t list_max, int with_strand, const uint32_t *bounds, size_t k,
                       int device, uint32_t *z, uint32_t *starts, uint32_t *lengths, uint32_t *hist, uint64_t *tail,
                       uint32_t *tail_count, uint32_t *widened, uint32_t *counts) {
    return guarded([&] {
        const bool widen = list_max != 0;
        if (!z || (n && !codes)) throw std::invalid_argument("null argument");
        if (width != 16 && width != 32) throw std::invalid_argument("codes of 16 or of 32 bits");
        if (n > kMaxText) throw std::invalid_argument("too many codes: the device pipeline uses 32-bit indices");
        if (poison > 0xffffu) throw std::invalid_argument("the poison is a half-word");
        if (hist && (!tail || !tail_count)) throw std::invalid_argument("a histogram needs its tail list and the count of it");
        if ((k && (!bounds || !counts)) || k >= (size_t(1) << 31)) throw std::invalid_argument("k ranges need 2k bounds and k counts");
        for (size_t j = 0; j + 1 < 2 * k; ++j)
            if (bounds[j] > bounds[j + 1]) throw std::invalid_argument("the bounds do not ascend");
        if (widen) {
            if (width != 16 || list_max > 0xffffu) throw std::invalid_argument("a wide-code list goes with 16-bit codes saturated at 1 .. 0xffff");
            if ((list_len && !list) || listed > list_len || list_len >= (size_t(1) << 32))
                throw std::invalid_argument("listed entries beyond the list, or no list");
        } else if (list || list_len || listed || widened) {
            throw std::invalid_argument("a wide-code list and the widened codes need list_max");
        }
        if (width == 16) {
            const uint32_t top = widen ? list_max : 0xfffeu;  // (without a list no code may reach the saturation value)
            for (size_t i = 0; i < n; ++i)
                if (codes[i] > top) throw std::invalid_argument(widen ? "a 16-bit code above list_max" : "a code >= 0xffff among 16-bit codes");
        }
        *z = 0;
        if (tail_count) *tail_count = 0;
        const size_t bins = with_strand ? 2 * (size_t)kLengthHistBins : (size_t)kLengthHistBins;
        if (hist) std::fill(hist, hist + bins, 0u);
        if (counts) std::fill(counts, counts + k, 0u);
        if (n == 0) return;

        Session ses(device, nullptr);
        Context &ctx = ses.ctx();
        hipStream_t s = ctx.stream;
        // the codes (and their widened copy), the cursor's arrays (exits, bitmaps, four words per node) and the outputs
        ctx.arena.reserve(n * 48 + list_len * 8 + k * 12 + (size_t(64) << 20));
        ArenaRewind rewind(ctx.arena);
        LstarCodes lc;
        if (width == 32) {
            lc = LstarCodes::of(ctx.arena.alloc<uint32_t>(n));
            HIP_CHECK(hipMemcpyAsync(lc.wide, codes, n * 4, hipMemcpyHostToDevice, s));
        } else {
            std::vector<uint16_t> half(n + 8, (uint16_t)poison);  // (padded as alloc_lstar pads the array)
            for (size_t i = 0; i < n; ++i) half[i] = (uint16_t)codes[i];
            lc.narrow = ctx.arena.alloc<uint16_t>(n + 8);
            lc.width = 16;
            HIP_CHECK(hipMemcpyAsync(lc.narrow, half.data(), (n + 8) * 2, hipMemcpyHostToDevice, s));
            HIP_CHECK(hipStreamSynchronize(s));  // half is a local vector
        }
        if (widen) {  // as build_lstar hands the codes on when the list holds entries
            const uint32_t count = (uint32_t)listed;
            lc.list.cap = (uint32_t)std::max<size_t>(list_len, 1);
            lc.list.items = ctx.arena.alloc<uint64_t>(lc.list.cap);
            lc.list.count = ctx.arena.alloc<uint32_t>(1);
            lc.list.max = list_max;
            HIP_CHECK(hipMemcpyAsync(lc.list.items, list, list_len * 8, hipMemcpyHostToDevice, s));
            HIP_CHECK(hipMemcpyAsync(lc.list.count, &count, 4, hipMemcpyHostToDevice, s));
            HIP_CHECK(hipStreamSynchronize(s));  // count is a local
            lc.wide = widened_lstar(ctx, lc, (uint32_t)n, count);
            lc.width = 32;
            if (widened) HIP_CHECK(hipMemcpyAsync(widened, lc.wide, n * 4, hipMemcpyDeviceToHost, s));
        }
        const Chain chain = mark_chain(ctx, (uint32_t)n, (uint32_t)std::min(start_pos, n), lc);
        *z = chain.z;
        uint32_t *d_order = nullptr, *d_hist = nullptr;
        ChainLengthsOut lo;
        if (chain.z && (hist || lengths)) {
            if (hist) {
                lo.tail_cap = length_tail_cap((uint32_t)n);
                d_hist = ctx.arena.alloc<uint32_t>(bins + 1);
                lo.hist = d_hist;
                lo.tail_count = d_hist + bins;
                lo.tail = ctx.arena.alloc<uint64_t>(lo.tail_cap);
                HIP_CHECK(hipMemsetAsync(d_hist, 0, (bins + 1) * 4, s));
            }
            if (lengths) lo.order = &d_order;
            chain_lengths(ctx, chain, lo, with_strand != 0);  // (16-bit codes: refused there)
        }
        if (chain.z && (starts || k)) {
            const uint32_t *d_starts = chain_starts(ctx, chain);
            if (starts) HIP_CHECK(hipMemcpyAsync(starts, d_starts, (size_t)chain.z * 4, hipMemcpyDeviceToHost, s));
            if (k) {
                uint32_t *d_bounds = ctx.arena.alloc<uint32_t>(2 * k), *d_counts = ctx.arena.alloc<uint32_t>(k);
                HIP_CHECK(hipMemcpyAsync(d_bounds, bounds, 2 * k * 4, hipMemcpyHostToDevice, s));
                rlz_count_per_target(ctx, d_starts, chain.z, d_bounds, (uint32_t)k, d_counts);
                HIP_CHECK(hipMemcpyAsync(counts, d_counts, k * 4, hipMemcpyDeviceToHost, s));
            }
        }
        if (d_order) HIP_CHECK(hipMemcpyAsync(lengths, d_order, (size_t)chain.z * 4, hipMemcpyDeviceToHost, s));
        if (d_hist) {
            HIP_CHECK(hipMemcpyAsync(hist, d_hist, bins * 4, hipMemcpyDeviceToHost, s));
            HIP_CHECK(hipMemcpyAsync(tail_count, d_hist + bins, 4, hipMemcpyDeviceToHost, s));
            HIP_CHECK(hipStreamSynchronize(s));
            if (*tail_count > lo.tail_cap) throw std::logic_error("debug_chain: more long factors than the tail list holds");
            HIP_CHECK(hipMemcpyAsync(tail, lo.tail, (size_t)*tail_count * 8, hipMemcpyDeviceToHost, s));
        }
        HIP_CHECK(hipStreamSynchronize(s));
        ctx.prof.collect();
    });
}

int nolzss_debug_cursor(int device, uint32_t *info) {
    return guarded([&] {
        if (!info) throw std::invalid_argument("output pointer is null");
        Session ses(device, nullptr);
        info[0] = ses.ctx().cursor_path;
        info[1] = ses.ctx().cursor_failed_tiles;
    });
}

int nolzss_debug_arena(int device, size_t *capacity, size_t *peak) {
    return guarded([&] {
        if (!capacity || !peak) throw std::invalid_argument("output pointer is null");
        Session ses(device, nullptr);
        *capacity = ses.ctx().arena.capacity();
        *peak = ses.ctx().arena.peak();
    });
}

int nolzss_debug_device_buffers(size_t *buffers, size_t *bytes) {
    return guarded([&] {
        if (!buffers || !bytes) throw std::invalid_argument("output pointer is null");
        *buffers = g_device_buffers.load();
        *bytes = g_device_buffer_bytes.load();
    });
}

int nolzss_debug_scan(uint32_t *data, size_t n, int mode, int device) {
    return guarded([&] {
        if (n == 0) return;
        if (!data) throw std::invalid_argument("null array");
        Session ses(device, nullptr);
        Context &ctx = ses.ctx();
        ctx.arena.reserve(n * 8 + (size_t(64) << 20));
        const size_t mark = ctx.arena.mark();
        uint32_t *d = ctx.arena.alloc<uint32_t>(n);
        HIP_CHECK(hipMemcpyAsync(d, data, n * 4, hipMemcpyHostToDevice, ctx.stream));
        if (mode == 0)
            scan_exclusive_add_u32(d, d, n, nullptr, ctx.arena, ctx.stream);
        else
            scan_inclusive_max_u32(d, d, n, ctx.arena, ctx.stream);
        HIP_CHECK(hipMemcpyAsync(data, d, n * 4, hipMemcpyDeviceToHost, ctx.stream));
        HIP_CHECK(hipStreamSynchronize(ctx.stream));
        ctx.arena.rewind(mark);
    });
}

}  // extern "C"
