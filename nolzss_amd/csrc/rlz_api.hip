// rlz_api.hip -- relative LZ: the layout of the prepared string, the run over it and the per-target split
// (part of the C ABI layer of libnolzss_hip.so, include/nolzss_hip.h; shared declarations: api_internal.hpp;
// the kernels: rlz.hip; DESIGN.md 5, "Relative LZ against a reference block")
#include "api_internal.hpp"

namespace nolzss {
namespace api {

constexpr size_t kMaxSentinels = 250;

// S = Rblk s T1 s .. Tk s [pad] rc-block s; every check of the refusal table happens here, before any device is touched
void rlz_prepare(const char *const *refs, const size_t *ref_lens, size_t m, const char *const *targets,
                 const size_t *target_lens, size_t k, bool with_rc, RlzPrepared &out) {
    if (m == 0) throw std::invalid_argument("relative LZ needs at least one reference sequence");
    if (!refs || !ref_lens || (k && (!targets || !target_lens))) throw std::invalid_argument("sequence array is null");
    if (m > kMaxSentinels || k > kMaxSentinels || (with_rc ? 2 * m + k + 1 : m + k) > kMaxSentinels)
        throw std::invalid_argument(
            "Too many sequences: relative LZ has 250 sentinels (2 x references + targets + 1 with reverse complement, "
            "references + targets without)");
    size_t ref_bases = 0, target_bases = 0;
    for (size_t i = 0; i < m; ++i) {
        if (ref_lens[i] && !refs[i]) throw std::invalid_argument("sequence pointer is null");
        ref_bases += ref_lens[i];
    }
    for (size_t j = 0; j < k; ++j) {
        if (target_lens[j] && !targets[j]) throw std::invalid_argument("sequence pointer is null");
        target_bases += target_lens[j];
    }
    if (ref_bases == 0) throw std::invalid_argument("the reference block is empty");
    const size_t B = ref_bases + (m - 1);
    const size_t after_targets = B + 1 + target_bases + k;
    const size_t pad = (with_rc && ((B - 1 + after_targets) & 1)) ? 1 : 0;  // B - 1 + E must be even
    const size_t E = after_targets + pad;
    const size_t total = with_rc ? E + B + 1 : after_targets;
    if (total > kMaxText) throw std::invalid_argument("text too long: the device pipeline uses 32-bit indices");
    for (size_t i = 0; i < m + k; ++i) {
        const char *q = i < m ? refs[i] : targets[i - m];
        const size_t len = i < m ? ref_lens[i] : target_lens[i - m];
        const size_t bad = first_invalid_nucleotide(q, len);
        if (bad < len)
            throw std::runtime_error("Invalid nucleotide '" + std::string(1, q[bad]) + "' found in sequence " +
                                     std::to_string(i));
    }
    out.S.resize(total);
    out.target_offsets.clear();
    uint8_t *S = out.S.data();
    size_t at = 0, sidx = 0;
    for (size_t i = 0; i < m; ++i) {
        if (i) S[at++] = rc_sentinel(sidx++);
        copy_upper(S + at, refs[i], ref_lens[i]);
        at += ref_lens[i];
    }
    S[at++] = rc_sentinel(sidx++);
    for (size_t j = 0; j < k; ++j) {
        out.target_offsets.push_back(at);
        copy_upper(S + at, targets[j], target_lens[j]);
        at += target_lens[j];
        S[at++] = rc_sentinel(sidx++);
    }
    if (with_rc) {
        if (pad) S[at++] = rc_sentinel(sidx++);
        for (size_t i = m; i-- > 0;) {  // the exact mirror of Rblk: rc(Rm) s .. s rc(R1)
            copy_reverse_complement(S + at, refs[i], ref_lens[i]);
            at += ref_lens[i];
            S[at++] = rc_sentinel(sidx++);
        }
    }
    out.lay.total = (uint32_t)total;
    out.lay.block_length = (uint32_t)B;
    out.lay.rc_block_start = (uint32_t)(with_rc ? E : total);
    out.lay.chain_end = (uint32_t)(after_targets - 1);
    out.lay.rcN = (uint32_t)(with_rc ? (B - 1 + E) / 2 : 0);
    out.lay.with_rc = with_rc;
}

namespace {

struct RlzRun {
    std::vector<size_t> counts, first;  // per target: records, and the index of its first record in block
    FactorBlock block;
};

// One pipeline run; want_factors: every record comes down (the sentinel literals between the targets with them) and is
// split by searching the ascending starts for the target offsets; otherwise the starts are counted per target on the
// device and only the k counts cross PCIe.  h_codes (optional): nolzss_debug_rlz_codes.
void rlz_run(const RlzPrepared &p, const size_t *target_lens, size_t k, bool want_factors, int device, RlzRun &out,
             uint32_t *h_codes) {
    out.counts.assign(k, 0);
    out.first.assign(k, 0);
    if (k == 0) return;
    const size_t total = p.S.size();
    Session ses(device, nullptr);
    Context &ctx = ses.ctx();
    reserve_arena_for(ctx, total, total);  // (as run_plain_host)
    uint8_t *d_S = ctx.arena.alloc<uint8_t>(total);
    {
        ProfScope ps(ctx.profiler(), "text_h2d", ctx.stream);
        upload_bytes(ctx, d_S, p.S.data(), total);
    }
    ChainRequest rq;
    (want_factors ? rq.records : rq.starts) = true;
    run_rlz_pipeline(ctx, d_S, p.lay, rq, h_codes);
    const uint32_t z = rq.z;
    if (want_factors) {
        out.block = download_factors(ctx, rq.d_records, z);
        HIP_CHECK(hipStreamSynchronize(ctx.stream));
        const nolzss_factor *f = out.block.get();
        auto first_at = [&](uint64_t pos) {
            return (size_t)(std::lower_bound(f, f + z, pos, [](const nolzss_factor &a, uint64_t x) { return a.start < x; }) - f);
        };
        for (size_t j = 0; j < k; ++j) {
            out.first[j] = first_at(p.target_offsets[j]);
            out.counts[j] = first_at(p.target_offsets[j] + target_lens[j]) - out.first[j];
        }
    } else {
        if (z) {
            std::vector<uint32_t> bounds(2 * k), counts(k);
            for (size_t j = 0; j < k; ++j) {
                bounds[2 * j] = (uint32_t)p.target_offsets[j];
                bounds[2 * j + 1] = (uint32_t)(p.target_offsets[j] + target_lens[j]);
            }
            uint32_t *d_bounds = ctx.arena.alloc<uint32_t>(2 * k), *d_counts = ctx.arena.alloc<uint32_t>(k);
            HIP_CHECK(hipMemcpyAsync(d_bounds, bounds.data(), bounds.size() * sizeof(uint32_t), hipMemcpyHostToDevice, ctx.stream));
            rlz_count_per_target(ctx, rq.d_starts, z, d_bounds, (uint32_t)k, d_counts);
            HIP_CHECK(hipMemcpyAsync(counts.data(), d_counts, k * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx.stream));
            HIP_CHECK(hipStreamSynchronize(ctx.stream));  // (bounds and counts are local vectors)
            for (size_t j = 0; j < k; ++j) out.counts[j] = counts[j];
        }
        HIP_CHECK(hipStreamSynchronize(ctx.stream));
    }
    ctx.prof.collect();
}

template <typename T> T *calloc_array(size_t count) {
    T *p = static_cast<T *>(std::calloc(count ? count : 1, sizeof(T)));
    if (!p) throw std::bad_alloc();
    return p;
}

char *id_blob(const std::vector<std::string> &ids, size_t *bytes) {
    std::string blob;
    for (const auto &id : ids) blob.append(id).push_back('\0');
    char *p = static_cast<char *>(std::malloc(blob.size() + 1));
    if (!p) throw std::bad_alloc();
    std::memcpy(p, blob.data(), blob.size());
    *bytes = blob.size();
    return p;
}

void rlz_factorize(const char *const *refs, const size_t *ref_lens, size_t m, const char *const *targets,
                   const size_t *target_lens, size_t k, bool with_rc, bool want_factors, int device,
                   const FastaParse *ref_parse, const FastaParse *tgt_parse, nolzss_rlz_result *out) {
    RlzPrepared p;
    rlz_prepare(refs, ref_lens, m, targets, target_lens, k, with_rc, p);
    RlzRun run;
    rlz_run(p, target_lens, k, want_factors, device, run, nullptr);
    nolzss_rlz_result res;
    std::memset(&res, 0, sizeof res);
    try {
        res.num_targets = k;
        res.block_length = p.lay.block_length;
        res.target_offsets = calloc_array<uint64_t>(k);
        res.target_lengths = calloc_array<uint64_t>(k);
        res.counts = calloc_array<size_t>(k);
        if (want_factors) res.factors = calloc_array<nolzss_factor *>(k);
        for (size_t j = 0; j < k; ++j) {
            res.target_offsets[j] = p.target_offsets[j];
            res.target_lengths[j] = target_lens[j];
            res.counts[j] = run.counts[j];
            if (want_factors) res.factors[j] = run.block ? run.block.get() + run.first[j] : nullptr;
        }
        if (ref_parse) {
            res.reference_ids = id_blob(ref_parse->ids, &res.reference_ids_bytes);
            res.num_references = ref_parse->ids.size();
            res.target_ids = id_blob(tgt_parse->ids, &res.target_ids_bytes);
        }
    } catch (...) {
        nolzss_free_rlz_result(&res);
        throw;
    }
    res.block = run.block.release();  // ownership moves to the caller
    *out = res;
}

}  // namespace
}  // namespace api
}  // namespace nolzss

using namespace nolzss;
using namespace nolzss::api;

extern "C" {

int nolzss_rlz_prepare(const char *const *refs, const size_t *ref_lens, size_t m, const char *const *targets,
                       const size_t *target_lens, size_t k, int with_rc, uint8_t **S, size_t *S_len,
                       uint64_t **target_offsets, size_t *block_length, size_t *rc_block_start, size_t *rcN) {
    return guarded([&] {
        if (!S || !S_len || !target_offsets || !block_length || !rc_block_start || !rcN)
            throw std::invalid_argument("output pointer is null");
        *S = nullptr;
        *target_offsets = nullptr;
        *S_len = *block_length = *rc_block_start = *rcN = 0;
        RlzPrepared p;
        rlz_prepare(refs, ref_lens, m, targets, target_lens, k, with_rc != 0, p);
        uint8_t *s = static_cast<uint8_t *>(std::malloc(p.S.size()));
        uint64_t *off = static_cast<uint64_t *>(std::malloc(k ? k * sizeof(uint64_t) : 8));
        if (!s || !off) {
            std::free(s);
            std::free(off);
            throw std::bad_alloc();
        }
        std::memcpy(s, p.S.data(), p.S.size());
        if (k) std::memcpy(off, p.target_offsets.data(), k * sizeof(uint64_t));
        *S = s;
        *S_len = p.S.size();
        *target_offsets = off;
        *block_length = p.lay.block_length;
        *rc_block_start = p.lay.rc_block_start;
        *rcN = p.lay.rcN;
    });
}

int nolzss_rlz_factorize(const char *const *refs, const size_t *ref_lens, size_t m, const char *const *targets,
                         const size_t *target_lens, size_t k, int with_rc, int want_factors, int device,
                         nolzss_rlz_result *out) {
    return guarded([&] {
        if (!out) throw std::invalid_argument("output pointer is null");
        std::memset(out, 0, sizeof *out);
        rlz_factorize(refs, ref_lens, m, targets, target_lens, k, with_rc != 0, want_factors != 0, device, nullptr, nullptr,
                      out);
    });
}

int nolzss_rlz_factorize_fasta(const char *reference_fasta_path, const char *target_fasta_path, int with_rc,
                               int sanitize_mode, int want_factors, int device, nolzss_rlz_result *out) {
    return guarded([&] {
        if (!out) throw std::invalid_argument("output pointer is null");
        std::memset(out, 0, sizeof *out);
        if (sanitize_mode != 0 && sanitize_mode != 1) throw std::invalid_argument("sanitize_mode must be 0 or 1");
        const FastaParse ref = parse_fasta(reference_fasta_path, sanitize_mode == 1);
        const FastaParse tgt = parse_fasta(target_fasta_path, sanitize_mode == 1);
        std::vector<const char *> ptrs;
        std::vector<size_t> lens;
        for (const FastaParse *parse : {&ref, &tgt})
            for (const auto &q : parse->sequences) {
                ptrs.push_back(q.data());
                lens.push_back(q.size());
            }
        const size_t m = ref.sequences.size(), k = tgt.sequences.size();
        rlz_factorize(ptrs.data(), lens.data(), m, ptrs.data() + m, lens.data() + m, k, with_rc != 0, want_factors != 0,
                      device, &ref, &tgt, out);
    });
}

void nolzss_free_rlz_result(nolzss_rlz_result *r) {
    if (!r) return;
    free_block(r->block);
    std::free(r->target_offsets);
    std::free(r->target_lengths);
    std::free(r->counts);
    std::free(r->factors);
    std::free(r->reference_ids);
    std::free(r->target_ids);
    std::memset(r, 0, sizeof *r);
}

int nolzss_debug_rlz_codes(const char *const *refs, const size_t *ref_lens, size_t m, const char *const *targets,
                           const size_t *target_lens, size_t k, int with_rc, int device, uint32_t *code) {
    return guarded([&] {
        RlzPrepared p;
        rlz_prepare(refs, ref_lens, m, targets, target_lens, k, with_rc != 0, p);
        if (k == 0) return;
        if (!code) throw std::invalid_argument("output pointer is null");
        RlzRun run;
        rlz_run(p, target_lens, k, false, device, run, code);
    });
}

}  // extern "C"
