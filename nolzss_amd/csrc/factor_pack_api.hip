// factor_pack_api.hip -- the compact container of factor records at the C ABI: host records packed on the device, a
// text factorized and packed without its 24-byte records ever leaving the device, and the sections expanded into
// records or decoded into the text (part of the C ABI layer of libnolzss_hip.so, include/nolzss_hip.h,
// nolzss_factors_pack / nolzss_factorize_packed / nolzss_factors_unpack / nolzss_decode_packed; the kernels:
// factor_pack.hip; DESIGN.md 5, "Factor records: the compact container").
#include "factor_pack.hpp"
#include "rlz_archive_pack.hpp"
#include "rlz_handles.hpp"

using namespace nolzss;
using namespace nolzss::api;

namespace {

// NOLZSS_ERR_NOMEM with a message (not a std::exception: guarded() lets it through to the entry point)
struct ArenaFull {
    std::string msg;
    explicit ArenaFull(const std::string &m) : msg(m) {}
    const char *what() const { return msg.c_str(); }
};

// The sections and the decoded text are host blocks as the factor records are (alloc_factor_block: huge pages that
// nothing zero-fills first; the data section of the benchmark text holds 260 MB), released with free_block / nolzss_free.
struct FreeBytes {
    void operator()(uint8_t *p) const { free_block(p); }
};
using Bytes = std::unique_ptr<uint8_t, FreeBytes>;

Bytes alloc_bytes(size_t n) {
    Bytes p(static_cast<uint8_t *>(alloc_factor_block(n ? n : 1)));
    if (!p) throw std::bad_alloc();
    return p;
}

constexpr uint32_t kLiteralsStored = 0, kLiteralsTwoBit = 1, kLiteralsAbsent = 2;

std::string rule_message(const char *who, uint64_t index, uint32_t rule) {
    return std::string(who) + ": record " + std::to_string(index) + " breaks " + factor_pack_rule_text(rule);
}

// arena bytes of a pack of z records (rank, diagonals, offsets, at most 9 data bytes and half a control byte each, the
// literals raw and at 2 bits, the tile sums of the scans) and of an unpack (offset, rank, length, position, steps and
// their sums; the records themselves are the caller's)
size_t pack_arena_bytes(size_t z) { return 28 * z + (size_t(1) << 20); }
size_t unpack_arena_bytes(size_t z) { return 34 * z + (size_t(1) << 20); }

void reserve_or_full(Context &ctx, size_t bytes, const char *who) {
    try {
        reserve_arena_for(ctx, 0, bytes);
    } catch (const std::invalid_argument &) {
        throw ArenaFull(std::string(who) + ": the device cannot hold " + std::to_string(bytes) + " bytes of records, sections and work arrays");
    }
}

struct Sections {
    Bytes control, data, literals;
    uint64_t data_bytes = 0, literal_bytes = 0, n_literals = 0;
    uint32_t literal_mode = kLiteralsTwoBit;
};

struct LiteralCountOff {};  // the records do not hold n_lit literals (the caller words it: it knows where the records are)

// z >= 1 records in device memory -> the sections in host buffers.  d_lit: the n_lit literal symbols in record order
// (device), or null for a factor file without them.  Arena temporaries stay (the Session rewinds).
void pack_on_device(Context &ctx, const Rec *d_recs, size_t z, const uint8_t *d_lit, size_t n_lit, const char *who, Sections &out) {
    hipStream_t s = ctx.stream;
    const FactorPackPlan plan = factor_pack_plan(ctx, d_recs, z);
    if (plan.data_bytes > 0xffffffffull)
        throw std::invalid_argument(std::string(who) + ": the data section would hold " + std::to_string(plan.data_bytes) +
                                    " bytes, 2^32 or more are refused");
    out.data_bytes = plan.data_bytes;
    out.n_literals = z - plan.copies;
    if (d_lit && out.n_literals != n_lit) throw LiteralCountOff{};  // before anything is written
    const size_t cb = (z + 1) / 2;
    out.control = alloc_bytes(cb);
    out.data = alloc_bytes((size_t)out.data_bytes);
    uint8_t *d_control = ctx.arena.alloc<uint8_t>(cb);
    uint8_t *d_data = ctx.arena.alloc<uint8_t>(out.data_bytes ? (size_t)out.data_bytes : 1);
    factor_pack_write(ctx, d_recs, z, plan, d_control, d_data);
    {
        ProfScope ps(ctx.profiler(), "factors_packed_d2h", s, (double)cb + (double)out.data_bytes);
        download_bytes(ctx, out.control.get(), d_control, cb);
        if (out.data_bytes) download_bytes(ctx, out.data.get(), d_data, (size_t)out.data_bytes);
    }
    if (!d_lit) {
        out.literal_mode = kLiteralsAbsent;
        out.literal_bytes = 0;
        out.literals = alloc_bytes(0);
        return;
    }
    uint8_t *d_two = ctx.arena.alloc<uint8_t>(factor_quarter(n_lit) + 1);
    out.literal_mode = factor_pack_literals(ctx, d_lit, n_lit, d_two) ? kLiteralsTwoBit : kLiteralsStored;
    out.literal_bytes = out.literal_mode == kLiteralsTwoBit ? factor_quarter(n_lit) : n_lit;
    out.literals = alloc_bytes((size_t)out.literal_bytes);
    if (out.literal_bytes) {
        ProfScope ps(ctx.profiler(), "factors_packed_d2h", s, (double)out.literal_bytes);
        download_bytes(ctx, out.literals.get(), out.literal_mode == kLiteralsTwoBit ? d_two : d_lit, (size_t)out.literal_bytes);
    }
}

void fill(nolzss_packed_factors *out, Sections &sec, uint64_t first_start, uint64_t z, uint64_t decoded) {
    out->literal_mode = sec.literal_mode;
    out->first_start = first_start;
    out->z = z;
    out->n_literals = sec.n_literals;
    out->decoded = decoded;
    out->control_bytes = (z + 1) / 2;
    out->data_bytes = sec.data_bytes;
    out->literal_bytes = sec.literal_bytes;
    out->control = sec.control.release();
    out->data = sec.data.release();
    out->literals = sec.literals.release();
}

void fill_empty(nolzss_packed_factors *out, bool store_literals) {
    Sections sec;
    sec.control = alloc_bytes(0);
    sec.data = alloc_bytes(0);
    sec.literals = alloc_bytes(0);
    sec.literal_mode = store_literals ? kLiteralsTwoBit : kLiteralsAbsent;
    fill(out, sec, 0, 0, 0);
}

// the message of a literal count that is off, in nolzss_decode's words (the host holds the records)
std::string literal_count_message(const nolzss_factor *f, size_t z, size_t n_literals) {
    size_t seen = 0;
    for (size_t k = 0; k < z; ++k)
        if (f[k].ref == f[k].start && seen++ == n_literals)
            return "pack_factors: record " + std::to_string(k) + " breaks literal count: it is literal number " +
                   std::to_string(n_literals + 1) + " and n_literals is " + std::to_string(n_literals);
    return "pack_factors: record " + std::to_string(z) + " (behind the last) breaks literal count: the " + std::to_string(z) +
           " records hold " + std::to_string(seen) + " literals and n_literals is " + std::to_string(n_literals);
}

void pack_host(const nolzss_factor *factors, size_t z, const uint8_t *literals, size_t n_literals, bool store_literals,
               int device, nolzss_packed_factors *out) {
    if (z && !factors) throw std::invalid_argument("factors pointer is null");
    if (store_literals && n_literals && !literals) throw std::invalid_argument("literals pointer is null");
    if (z > kMaxText || n_literals > kMaxText)
        throw std::invalid_argument("text too long: the device pipeline uses 32-bit indices");
    if (z == 0) {  // no record: no device
        if (store_literals && n_literals) throw std::invalid_argument(literal_count_message(factors, 0, n_literals));
        fill_empty(out, store_literals);
        return;
    }
    const uint64_t first_start = factors[0].start;
    const nolzss_factor &last = factors[z - 1];
    const uint64_t n = last.start + last.length;
    if (first_start > kMaxText || n < last.start || n > kMaxText)
        throw std::invalid_argument("text too long: the device pipeline uses 32-bit indices");
    DeviceRestore restore;
    Session ses(device, nullptr);
    Context &ctx = ses.ctx();
    hipStream_t s = ctx.stream;
    Sections sec;
    try {
        ProfScope whole(ctx.profiler(), "factors_pack_all", s);
        reserve_or_full(ctx, sizeof(Rec) * z + n_literals + pack_arena_bytes(z), "pack_factors");
        Rec *d_recs = ctx.arena.alloc<Rec>(z);
        uint8_t *d_lit = ctx.arena.alloc<uint8_t>(n_literals ? n_literals : 1);
        {
            ProfScope ps(ctx.profiler(), "records_h2d", s, 24.0 * (double)z);
            upload_bytes(ctx, d_recs, factors, sizeof(Rec) * z);
            if (store_literals && n_literals) upload_bytes(ctx, d_lit, literals, n_literals);
        }
        // whatever the format cannot carry is refused before a byte is packed
        const uint64_t bad = factor_check_records(ctx, d_recs, z, kMaxText);
        if (bad != ~0ull) throw std::invalid_argument(rule_message("pack_factors", bad >> 4, (uint32_t)(bad & 15u)));
        try {
            pack_on_device(ctx, d_recs, z, store_literals ? d_lit : nullptr, store_literals ? n_literals : 0, "pack_factors", sec);
        } catch (const LiteralCountOff &) {
            throw std::invalid_argument(literal_count_message(factors, z, n_literals));
        }
    } catch (...) {
        (void)hipStreamSynchronize(s);  // (the uploads read the caller's buffers)
        throw;
    }
    HIP_CHECK(hipStreamSynchronize(s));
    HIP_CHECK(hipGetLastError());
    ctx.prof.collect();
    fill(out, sec, first_start, z, n - first_start);
}

// text: host bytes (uploaded) or null with d_resident set.  The factorization of nolzss_roundtrip: the records stay
// where the pipeline left them, above its work arrays, and the pack takes what is left of the arena.
void factorize_packed(const uint8_t *text, const uint8_t *d_resident, size_t n, bool with_rc, bool store_literals, int device,
                      void *stream, nolzss_packed_factors *out) {
    const uint8_t *given = d_resident ? d_resident : text;
    if (n && !given) throw std::invalid_argument("text pointer is null");
    if (!check_text_source(given, n, with_rc)) {
        fill_empty(out, store_literals);
        return;
    }
    DeviceRestore restore;
    Session ses(device, stream);
    Context &ctx = ses.ctx();
    hipStream_t s = ctx.stream;
    if (d_resident && !stream) order_behind_default_stream(ctx);
    Sections sec;
    size_t zc = 0;
    {
        ProfScope whole(ctx.profiler(), "factorize_packed_all", s);
        const size_t m = with_rc ? 2 * n + 2 : n;
        reserve_arena_for(ctx, m, (with_rc ? m : 0) + (d_resident ? 0 : n));
        const uint8_t *d_T = d_resident;
        if (!d_resident) {
            uint8_t *up = ctx.arena.alloc<uint8_t>(n);
            ProfScope ps(ctx.profiler(), "text_h2d", s);
            upload_bytes(ctx, up, text, n);
            d_T = up;
        }
        ChainRequest rq;
        rq.records = true;
        const uint8_t *d_text = d_T;  // what the records describe: the bytes, or the upper-cased strand of the prepared string
        if (with_rc) {
            uint8_t *d_S = ctx.arena.alloc<uint8_t>(m);
            const uint32_t bad = prepare_single_rc_on_device(ctx, d_T, (uint32_t)n, d_S);
            if (bad != 0xffffffffu) {  // (as dna_w_rc_common)
                uint8_t c = 0;
                if (text) c = text[bad];
                else HIP_CHECK(hipMemcpy(&c, d_T + bad, 1, hipMemcpyDeviceToHost));
                throw std::runtime_error("Invalid nucleotide '" + std::string(1, (char)c) + "' found in sequence 0");
            }
            d_text = d_S;
            run_rc_pipeline(ctx, d_S, m, 0, rq);
        } else {
            run_plain(ctx, d_T, n, 0, rq);
        }
        zc = rq.z;
        if (zc == 0 || !rq.d_records) throw std::runtime_error("factorize_packed: the pipeline left no records");
        const size_t need = zc + pack_arena_bytes(zc);
        const size_t left = ctx.arena.capacity() - ctx.arena.mark();
        if (left < need)
            throw ArenaFull("factorize_packed: the device arena has " + std::to_string(left) + " bytes left behind the factorization of " +
                            std::to_string(n) + " symbols, the pack of " + std::to_string(zc) + " records needs " + std::to_string(need));
        const Rec *recs = static_cast<const Rec *>(rq.d_records);
        uint8_t *d_lit = nullptr;
        size_t n_lit = 0;
        if (store_literals) {
            d_lit = ctx.arena.alloc<uint8_t>(zc);
            n_lit = gather_literals(ctx, recs, zc, d_text, d_lit);
        }
        try {
            pack_on_device(ctx, recs, zc, d_lit, n_lit, "factorize_packed", sec);
        } catch (const LiteralCountOff &) {
            throw std::runtime_error("factorize_packed: the literal gather and the pack disagree about the pipeline's own records");
        }
    }
    HIP_CHECK(hipStreamSynchronize(s));
    HIP_CHECK(hipGetLastError());
    ctx.prof.collect();
    fill(out, sec, 0, zc, n);
}

// ---- the way back -----------------------------------------------------------------------------------------------------
// The host checks of UNTRUSTED sections: every device read below is bounded by these sizes.
void check_sections(const nolzss_packed_factors &a) {
    if (a.literal_mode > 2) throw std::invalid_argument("packed factors: literal_mode is none of 0, 1, 2");
    if (a.first_start > kMaxText || a.decoded > kMaxText || a.first_start + a.decoded > kMaxText || a.z > kMaxText ||
        a.n_literals > kMaxText)
        throw std::invalid_argument("text too long: the device pipeline uses 32-bit indices");
    auto size_is = [](const char *name, uint64_t have, uint64_t want) {
        if (have != want)
            throw std::invalid_argument(std::string("packed factors: the ") + name + " section holds " + std::to_string(have) +
                                        " bytes, the counts ask for " + std::to_string(want));
    };
    size_is("control", a.control_bytes, (a.z + 1) / 2);
    size_is("literal", a.literal_bytes,
            a.literal_mode == kLiteralsTwoBit ? factor_quarter(a.n_literals) : a.literal_mode == kLiteralsStored ? a.n_literals : 0);
    if (a.data_bytes > 0xffffffffull) throw std::invalid_argument("packed factors: a data section of 2^32 bytes or more");
    if ((a.control_bytes && !a.control) || (a.data_bytes && !a.data) || (a.literal_bytes && !a.literals))
        throw std::invalid_argument("packed factors: a section pointer is null");
    if (a.z == 0) {  // nothing for a device to judge
        if (a.data_bytes) throw std::invalid_argument(rule_message("packed factors", 0, kFacDataSize));
        if (a.n_literals)
            throw std::invalid_argument("packed factors: record 0 (behind the last) breaks literal count: the 0 records hold 0 "
                                        "literals and n_literals is " + std::to_string(a.n_literals));
        if (a.decoded) throw std::invalid_argument(rule_message("packed factors", 0, kFacDecoded));
    }
}

struct Unpacked {
    Rec *d_recs = nullptr;
    uint8_t *d_lit = nullptr;  // n_literals symbols (null for literal_mode 2)
};

// z >= 1, sections checked, arena reserved: upload, expand, judge.  Arena memory stays (the Session rewinds).
Unpacked unpack_on_device(Context &ctx, const nolzss_packed_factors &a) {
    hipStream_t s = ctx.stream;
    const size_t z = (size_t)a.z, nlit = (size_t)a.n_literals;
    Unpacked u;
    uint8_t *d_control = ctx.arena.alloc<uint8_t>((size_t)a.control_bytes);
    uint8_t *d_data = ctx.arena.alloc<uint8_t>(a.data_bytes ? (size_t)a.data_bytes : 1);
    uint8_t *d_packed = ctx.arena.alloc<uint8_t>(a.literal_bytes ? (size_t)a.literal_bytes : 1);
    u.d_recs = ctx.arena.alloc<Rec>(z);
    {
        ProfScope ps(ctx.profiler(), "factors_packed_h2d", s, (double)(a.control_bytes + a.data_bytes + a.literal_bytes));
        upload_bytes(ctx, d_control, a.control, (size_t)a.control_bytes);
        if (a.data_bytes) upload_bytes(ctx, d_data, a.data, (size_t)a.data_bytes);
        if (a.literal_bytes) upload_bytes(ctx, d_packed, a.literals, (size_t)a.literal_bytes);
    }
    try {
        if (a.literal_mode == kLiteralsTwoBit) {
            u.d_lit = ctx.arena.alloc<uint8_t>(nlit ? nlit : 1);
            ProfScope ps(ctx.profiler(), "factors_unpack_literals", s, 1.25 * (double)nlit);
            packed_quarter_unpack(ctx, d_packed, nlit, u.d_lit);
        } else if (a.literal_mode == kLiteralsStored) {
            u.d_lit = d_packed;
        }
        FactorUnpackIn in{};
        in.control = d_control;
        in.data = d_data;
        in.data_bytes = a.data_bytes;
        in.n_literals = a.n_literals;
        in.decoded = a.decoded;
        in.first_start = (uint32_t)a.first_start;
        const FactorUnpackOut res = factor_unpack_records(ctx, in, z, u.d_recs);
        if (res.bad != ~0ull) {
            const uint64_t index = res.bad >> 4;
            const uint32_t rule = (uint32_t)(res.bad & 15u);
            std::string msg = rule_message("packed factors", index, rule);
            if (rule == kFacDecoded)
                msg += ": the " + std::to_string(z) + " records cover " + std::to_string(res.covered) + " positions and decoded is " +
                       std::to_string(a.decoded);
            throw std::invalid_argument(msg);
        }
        if (z - res.copies != a.n_literals)
            throw std::invalid_argument("packed factors: record " + std::to_string(z) + " (behind the last) breaks literal count: the " +
                                        std::to_string(z) + " records hold " + std::to_string(z - res.copies) +
                                        " literals and n_literals is " + std::to_string(a.n_literals));
    } catch (...) {
        (void)hipStreamSynchronize(s);  // (the uploads read the caller's sections)
        throw;
    }
    return u;
}

void unpack_host(const nolzss_packed_factors *in, int device, nolzss_factor **factors, size_t *z_out, uint8_t **literals,
                 size_t *n_literals) {
    if (!factors || !z_out || !literals || !n_literals) throw std::invalid_argument("output pointer is null");
    *factors = nullptr;
    *z_out = 0;
    *literals = nullptr;
    *n_literals = 0;
    if (!in) throw std::invalid_argument("packed factors pointer is null");
    const nolzss_packed_factors &a = *in;
    check_sections(a);
    if (a.z == 0) return;
    const size_t z = (size_t)a.z, nlit = (size_t)a.n_literals;
    DeviceRestore restore;
    Session ses(device, nullptr);
    Context &ctx = ses.ctx();
    FactorBlock block;
    Bytes lit;
    {
        ProfScope whole(ctx.profiler(), "factors_unpack_all", ctx.stream);
        reserve_or_full(ctx, sizeof(Rec) * z + a.control_bytes + a.data_bytes + a.literal_bytes + nlit + unpack_arena_bytes(z),
                        "unpack_factors");
        const Unpacked u = unpack_on_device(ctx, a);
        block = download_factors(ctx, u.d_recs, z);
        if (u.d_lit) {
            lit = alloc_bytes(nlit);
            if (nlit) download_bytes(ctx, lit.get(), u.d_lit, nlit);
        }
    }
    HIP_CHECK(hipStreamSynchronize(ctx.stream));
    HIP_CHECK(hipGetLastError());
    ctx.prof.collect();
    *factors = block.release();
    *z_out = z;
    *literals = lit.release();
    *n_literals = nlit;
}

void decode_packed(const nolzss_packed_factors *in, const uint8_t *prefix, size_t prefix_len, int device, uint8_t **text,
                   size_t *n_out, nolzss_decode_info *info) {
    if (!text || !n_out) throw std::invalid_argument("output pointer is null");
    *text = nullptr;
    *n_out = 0;
    if (info) std::memset(info, 0, sizeof *info);
    if (!in) throw std::invalid_argument("packed factors pointer is null");
    if (prefix_len && !prefix) throw std::invalid_argument("prefix pointer is null");
    const nolzss_packed_factors &a = *in;
    check_sections(a);
    if (a.literal_mode == kLiteralsAbsent)
        throw std::invalid_argument("decode_packed: literal_mode 2: the sections do not hold the literal symbols, nothing can be decoded");
    if ((uint64_t)prefix_len != a.first_start)
        throw std::invalid_argument("decode_packed: the prefix holds " + std::to_string(prefix_len) + " bytes and first_start is " +
                                    std::to_string(a.first_start));
    const size_t z = (size_t)a.z, nlit = (size_t)a.n_literals, n = prefix_len + (size_t)a.decoded;
    Bytes h = alloc_bytes(n);
    if (z == 0) {  // the prefix alone: no device
        if (prefix_len) std::memcpy(h.get(), prefix, prefix_len);
        *text = h.release();
        *n_out = prefix_len;
        if (info) info->n = prefix_len;
        return;
    }
    DeviceRestore restore;
    Session ses(device, nullptr);
    Context &ctx = ses.ctx();
    hipStream_t s = ctx.stream;
    DecodeStats st;
    {
        ProfScope whole(ctx.profiler(), "decode_packed_all", s);
        reserve_or_full(ctx, sizeof(Rec) * z + a.control_bytes + a.data_bytes + a.literal_bytes + nlit + unpack_arena_bytes(z) + n +
                                 decode_arena_bytes(z, (size_t)a.decoded), "decode_packed");
        uint8_t *d_out = ctx.arena.alloc<uint8_t>(n + 1);
        if (prefix_len) upload_bytes(ctx, d_out, prefix, prefix_len);
        try {
            const Unpacked u = unpack_on_device(ctx, a);
            st = decode_on_device(ctx, u.d_recs, z, u.d_lit, nlit, d_out, prefix_len, n);
        } catch (const DecodeRefusal &e) {
            (void)hipStreamSynchronize(s);
            if (e.rule == kDecodeComplement)
                throw std::invalid_argument("decode_packed: position " + std::to_string(e.position) +
                                            " breaks complement of a non-nucleotide: its chain is reverse-complemented an odd number "
                                            "of times and ends in a byte that is not A, C, G or T");
            throw std::invalid_argument(std::string("decode_packed: ") + e.what());
        } catch (...) {
            (void)hipStreamSynchronize(s);  // (the prefix upload reads the caller's buffer)
            throw;
        }
        ProfScope ps(ctx.profiler(), "text_d2h", s, (double)n);
        download_bytes(ctx, h.get(), d_out, n);
    }
    HIP_CHECK(hipStreamSynchronize(s));
    ctx.prof.collect();
    *text = h.release();
    *n_out = n;
    if (info) {
        info->n = n;
        info->z = z;
        info->n_literals = st.n_literals;
        info->resolved_at_expand = st.resolved_at_expand;
        info->rounds = st.rounds;
        info->max_active = st.max_active;
    }
}

template <typename F> int guarded_nomem(F &&f) {
    try {
        return guarded(f);
    } catch (const ArenaFull &e) {
        return set_error(NOLZSS_ERR_NOMEM, e.what());
    }
}

}  // namespace

extern "C" {

int nolzss_factors_pack(const nolzss_factor *factors, size_t z, const uint8_t *literals, size_t n_literals, int store_literals,
                        int device, nolzss_packed_factors *out) {
    return guarded_nomem([&] {
        if (!out) throw std::invalid_argument("output pointer is null");
        std::memset(out, 0, sizeof *out);
        pack_host(factors, z, literals, n_literals, store_literals != 0, device, out);
    });
}

int nolzss_factorize_packed(const uint8_t *text, size_t n, int with_rc, int store_literals, int device, nolzss_packed_factors *out) {
    return guarded_nomem([&] {
        if (!out) throw std::invalid_argument("output pointer is null");
        std::memset(out, 0, sizeof *out);
        factorize_packed(text, nullptr, n, with_rc != 0, store_literals != 0, device, nullptr, out);
    });
}

int nolzss_factorize_packed_device(const void *d_text, size_t n, int with_rc, int store_literals, int device, void *stream,
                                   nolzss_packed_factors *out) {
    return guarded_nomem([&] {
        if (!out) throw std::invalid_argument("output pointer is null");
        std::memset(out, 0, sizeof *out);
        if (n && !d_text) throw std::invalid_argument("text pointer is null");
        factorize_packed(nullptr, static_cast<const uint8_t *>(d_text), n, with_rc != 0, store_literals != 0, device, stream, out);
    });
}

void nolzss_free_packed_factors(nolzss_packed_factors *p) {
    if (!p) return;
    free_block(p->control);
    free_block(p->data);
    free_block(p->literals);
    std::memset(p, 0, sizeof *p);
}

int nolzss_factors_unpack(const nolzss_packed_factors *in, int device, nolzss_factor **factors, size_t *z, uint8_t **literals,
                          size_t *n_literals) {
    return guarded_nomem([&] { unpack_host(in, device, factors, z, literals, n_literals); });
}

int nolzss_decode_packed(const nolzss_packed_factors *in, const uint8_t *prefix, size_t prefix_len, int device, uint8_t **text,
                         size_t *n, nolzss_decode_info *info) {
    return guarded_nomem([&] { decode_packed(in, prefix, prefix_len, device, text, n, info); });
}

}  // extern "C"
