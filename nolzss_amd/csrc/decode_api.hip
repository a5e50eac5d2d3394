// decode_api.hip -- the decoder's entry points: host records and literals up, text down; the device-resident round
// trip factorize -> literal gather -> decode -> compare (part of the C ABI layer of libnolzss_hip.so,
// include/nolzss_hip.h; shared declarations: api_internal.hpp; the kernels: decode.hip)
#include "decode.hpp"

namespace nolzss {
namespace api {
namespace {

// NOLZSS_ERR_NOMEM with a message (not a std::exception: guarded() lets it through to the entry point)
struct ArenaFull {
    std::string msg;
    explicit ArenaFull(const std::string &m) : msg(m) {}
    const char *what() const { return msg.c_str(); }
};

bool tile_skip() {  // NOLZSS_DECODE_TILE_SKIP=0: every jump round runs over every tile (A/B measurements)
    const char *e = getenv("NOLZSS_DECODE_TILE_SKIP");
    return !(e && *e == '0');
}

void fill_info(nolzss_decode_info *info, size_t n, size_t z, const DecodeStats &st) {
    if (!info) return;
    info->n = n;
    info->z = z;
    info->n_literals = st.n_literals;
    info->resolved_at_expand = st.resolved_at_expand;
    info->rounds = st.rounds;
    info->max_active = st.max_active;
}

// the message of a refusal that decode_on_device leaves to the owner of the records
std::string name_refusal(const DecodeRefusal &e, const nolzss_factor *f, size_t z, size_t n_literals) {
    if (e.rule == kDecodeLiteralCount) {
        size_t seen = 0;
        for (size_t k = 0; k < z; ++k)
            if (f[k].ref == f[k].start && seen++ == n_literals)
                return "decode: record " + std::to_string(k) + " breaks literal count: it is literal number " +
                       std::to_string(n_literals + 1) + " and n_literals is " + std::to_string(n_literals);
        return "decode: record " + std::to_string(z) + " (behind the last) breaks literal count: the " + std::to_string(z) +
               " records hold " + std::to_string(seen) + " literals and n_literals is " + std::to_string(n_literals);
    }
    if (e.rule == kDecodeComplement) {
        const size_t k = (size_t)(std::upper_bound(f, f + z, e.position,
                                                   [](uint64_t x, const nolzss_factor &a) { return x < a.start; }) - f) - 1;
        return "decode: record " + std::to_string(k) + " breaks complement of a non-nucleotide: the chain of position " +
               std::to_string(e.position) + " is reverse-complemented an odd number of times and ends in a byte that is not A, C, G or T";
    }
    return e.what();
}

void decode_host(const nolzss_factor *factors, size_t z, const uint8_t *literals, size_t n_literals, const uint8_t *prefix,
                 size_t prefix_len, int device, uint8_t **text, size_t *n_out, nolzss_decode_info *info) {
    if (!text || !n_out) throw std::invalid_argument("output pointer is null");
    *text = nullptr;
    *n_out = 0;
    if (info) std::memset(info, 0, sizeof *info);
    if (z && !factors) throw std::invalid_argument("factors pointer is null");
    if (n_literals && !literals) throw std::invalid_argument("literals pointer is null");
    if (prefix_len && !prefix) throw std::invalid_argument("prefix pointer is null");
    if (prefix_len > kMaxText || z > kMaxText)
        throw std::invalid_argument("text too long: the device pipeline uses 32-bit indices");
    if (z == 0) {  // the prefix alone: no device
        if (n_literals)
            throw std::invalid_argument("decode: record 0 (behind the last) breaks literal count: the 0 records hold 0 "
                                        "literals and n_literals is " + std::to_string(n_literals));
        uint8_t *h = static_cast<uint8_t *>(std::malloc(prefix_len ? prefix_len : 1));
        if (!h) throw std::bad_alloc();
        if (prefix_len) std::memcpy(h, prefix, prefix_len);
        *text = h;
        *n_out = prefix_len;
        if (info) info->n = prefix_len;
        return;
    }
    const nolzss_factor &last = factors[z - 1];
    const uint64_t n = last.start + last.length;
    if (n < last.start || n > kMaxText || n_literals > kMaxText)
        throw std::invalid_argument("text too long: the device pipeline uses 32-bit indices");
    // (n below prefix_len + z cannot tile: the check kernel names the record, nothing is sized by n before it)
    const size_t decoded = n > prefix_len ? n - prefix_len : 0;
    Session ses(device, nullptr);
    Context &ctx = ses.ctx();
    const size_t bytes = sizeof(Rec) * z + n_literals + (size_t)n + decode_arena_bytes(z, decoded) + (size_t(1) << 20);
    try {
        reserve_arena_for(ctx, 0, bytes);
    } catch (const std::invalid_argument &) {
        throw ArenaFull("decode: the device cannot hold " + std::to_string(bytes) + " bytes of records, literals, text and "
                        "state words");
    }
    Rec *d_recs = ctx.arena.alloc<Rec>(z);
    uint8_t *d_lit = ctx.arena.alloc<uint8_t>(n_literals ? n_literals : 1);
    uint8_t *d_out = ctx.arena.alloc<uint8_t>(std::max<size_t>((size_t)n, prefix_len) + 1);
    {
        ProfScope ps(ctx.profiler(), "records_h2d", ctx.stream, 24.0 * (double)z);
        upload_bytes(ctx, d_recs, factors, sizeof(Rec) * z);
    }
    if (n_literals) upload_bytes(ctx, d_lit, literals, n_literals);
    if (prefix_len) upload_bytes(ctx, d_out, prefix, prefix_len);
    DecodeStats st;
    try {
        st = decode_on_device(ctx, d_recs, z, d_lit, n_literals, d_out, prefix_len, (size_t)n, tile_skip());
    } catch (const DecodeRefusal &e) {
        (void)hipStreamSynchronize(ctx.stream);  // (the uploads read the caller's buffers)
        throw std::invalid_argument(name_refusal(e, factors, z, n_literals));
    }
    uint8_t *h = static_cast<uint8_t *>(std::malloc((size_t)n));
    if (!h) throw std::bad_alloc();
    try {
        ProfScope ps(ctx.profiler(), "text_d2h", ctx.stream, (double)n);
        download_bytes(ctx, h, d_out, (size_t)n);
    } catch (...) {
        std::free(h);
        throw;
    }
    ctx.prof.collect();
    *text = h;
    *n_out = (size_t)n;
    fill_info(info, (size_t)n, z, st);
}

// text: host bytes (uploaded) or null with d_resident set
void roundtrip(const uint8_t *text, const uint8_t *d_resident, size_t n, bool with_rc, int device, void *stream, size_t *z,
               uint64_t *mismatches, uint64_t *first_mismatch, nolzss_decode_info *info) {
    if (!z || !mismatches || !first_mismatch) throw std::invalid_argument("output pointer is null");
    *z = 0;
    *mismatches = 0;
    *first_mismatch = ~0ull;
    if (info) std::memset(info, 0, sizeof *info);
    const uint8_t *given = d_resident ? d_resident : text;
    if (n && !given) throw std::invalid_argument("text pointer is null");
    if (!check_text_source(given, n, with_rc)) return;
    Session ses(device, stream);
    Context &ctx = ses.ctx();
    if (d_resident && !stream) order_behind_default_stream(ctx);
    const size_t m = with_rc ? 2 * n + 2 : n;
    reserve_arena_for(ctx, m, (with_rc ? m : 0) + (d_resident ? 0 : n));
    const uint8_t *d_T = d_resident;
    if (!d_resident) {
        uint8_t *up = ctx.arena.alloc<uint8_t>(n);
        ProfScope ps(ctx.profiler(), "text_h2d", ctx.stream);
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
    const size_t zc = rq.z;
    const void *d_recs = rq.d_records;
    *z = zc;
    if (zc == 0 || !d_recs) throw std::runtime_error("round trip: the pipeline left no records");
    // the records stay where the pipeline left them, above its work arrays: the decoder takes what is left of the arena
    const size_t need = zc + n + decode_arena_bytes(zc, n) + 4096;
    const size_t left = ctx.arena.capacity() - ctx.arena.mark();
    if (left < need)
        throw ArenaFull("round trip: the device arena has " + std::to_string(left) + " bytes left behind the factorization of " +
                        std::to_string(n) + " symbols, records plus decode state need " + std::to_string(need));
    const Rec *recs = static_cast<const Rec *>(d_recs);
    uint8_t *d_lit = ctx.arena.alloc<uint8_t>(zc);
    uint8_t *d_out = ctx.arena.alloc<uint8_t>(n);
    const size_t n_lit = gather_literals(ctx, recs, zc, d_text, d_lit);
    DecodeStats st;
    try {
        st = decode_on_device(ctx, recs, zc, d_lit, n_lit, d_out, 0, n, tile_skip());
    } catch (const DecodeRefusal &e) {
        throw std::runtime_error(std::string("round trip: the decoder refused the pipeline's own records (rule ") +
                                 std::to_string((int)e.rule) + ", record " + std::to_string(e.record) + ", position " +
                                 std::to_string(e.position) + ") " + e.what());
    }
    count_mismatches(ctx, d_text, d_out, n, mismatches, first_mismatch);
    ctx.prof.collect();
    fill_info(info, n, zc, st);
}

}  // namespace
}  // namespace api
}  // namespace nolzss

using namespace nolzss;
using namespace nolzss::api;

extern "C" {

int nolzss_literal_symbols(const uint8_t *text, size_t n, const nolzss_factor *factors, size_t z, uint8_t **literals,
                           size_t *n_literals) {
    return guarded([&] {
        if (!literals || !n_literals) throw std::invalid_argument("output pointer is null");
        *literals = nullptr;
        *n_literals = 0;
        if (n && !text) throw std::invalid_argument("text pointer is null");
        if (z && !factors) throw std::invalid_argument("factors pointer is null");
        size_t count = 0;
        for (size_t k = 0; k < z; ++k)
            if (factors[k].ref == factors[k].start) {
                if (factors[k].start >= n)
                    throw std::invalid_argument("literal_symbols: record " + std::to_string(k) + " starts at " +
                                                std::to_string(factors[k].start) + ", beyond the text of " + std::to_string(n) +
                                                " bytes");
                ++count;
            }
        uint8_t *h = static_cast<uint8_t *>(std::malloc(count ? count : 1));
        if (!h) throw std::bad_alloc();
        size_t j = 0;
        for (size_t k = 0; k < z; ++k)
            if (factors[k].ref == factors[k].start) h[j++] = text[factors[k].start];
        *literals = h;
        *n_literals = count;
    });
}

int nolzss_decode(const nolzss_factor *factors, size_t z, const uint8_t *literals, size_t n_literals, const uint8_t *prefix,
                  size_t prefix_len, int device, uint8_t **text, size_t *n, nolzss_decode_info *info) {
    try {
        return guarded([&] { decode_host(factors, z, literals, n_literals, prefix, prefix_len, device, text, n, info); });
    } catch (const ArenaFull &e) {
        return set_error(NOLZSS_ERR_NOMEM, e.what());
    }
}

int nolzss_roundtrip(const uint8_t *text, size_t n, int with_rc, int device, size_t *z, uint64_t *mismatches,
                     uint64_t *first_mismatch, nolzss_decode_info *info) {
    try {
        return guarded([&] { roundtrip(text, nullptr, n, with_rc != 0, device, nullptr, z, mismatches, first_mismatch, info); });
    } catch (const ArenaFull &e) {
        return set_error(NOLZSS_ERR_NOMEM, e.what());
    }
}

int nolzss_roundtrip_device(const void *d_text, size_t n, int with_rc, int device, void *stream, size_t *z,
                            uint64_t *mismatches, uint64_t *first_mismatch, nolzss_decode_info *info) {
    try {
        return guarded([&] {
            if (n && !d_text) throw std::invalid_argument("text pointer is null");
            roundtrip(nullptr, static_cast<const uint8_t *>(d_text), n, with_rc != 0, device, stream, z, mismatches,
                      first_mismatch, info);
        });
    } catch (const ArenaFull &e) {
        return set_error(NOLZSS_ERR_NOMEM, e.what());
    }
}

int nolzss_debug_count_mismatches(const uint8_t *a, const uint8_t *b, size_t n, int device, uint64_t *count,
                                  uint64_t *first) {
    return guarded([&] {
        if (!count || !first) throw std::invalid_argument("output pointer is null");
        *count = 0;
        *first = ~0ull;
        if (n && (!a || !b)) throw std::invalid_argument("array pointer is null");
        if (n == 0) return;
        Session ses(device, nullptr);
        Context &ctx = ses.ctx();
        reserve_arena_for(ctx, 0, 2 * n + (size_t(1) << 20));
        uint8_t *d_a = ctx.arena.alloc<uint8_t>(n), *d_b = ctx.arena.alloc<uint8_t>(n);
        upload_bytes(ctx, d_a, a, n);
        upload_bytes(ctx, d_b, b, n);
        count_mismatches(ctx, d_a, d_b, n, count, first);
        ctx.prof.collect();
    });
}

}  // extern "C"
