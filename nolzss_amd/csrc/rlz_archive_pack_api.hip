// rlz_archive_pack_api.hip -- the compact container at the C ABI: any archive handle packed on the device into the four
// sections of the file, and those sections opened as a handle that behaves as one of nolzss_rlz_archive_open_records
// (part of the C ABI layer of libnolzss_hip.so, include/nolzss_hip.h, nolzss_rlz_archive_pack / _open_packed; the
// kernels: rlz_archive_pack.hip; DESIGN.md 5, "Relative-LZ archive: the compact container").  Only the compact streams
// cross PCIe: the 24-byte records of export and open_records do not exist here.
#include "rlz_archive_pack.hpp"
#include "rlz_handles.hpp"

using namespace nolzss;
using namespace nolzss::api;

namespace {

struct FreeBytes {
    void operator()(uint8_t *p) const { std::free(p); }
};
using Bytes = std::unique_ptr<uint8_t, FreeBytes>;

Bytes alloc_bytes(size_t n) {
    Bytes p(static_cast<uint8_t *>(std::malloc(n ? n : 1)));
    if (!p) throw std::bad_alloc();
    return p;
}

inline int host_base_code(uint8_t c) { return c == 'A' ? 0 : c == 'C' ? 1 : c == 'G' ? 2 : c == 'T' ? 3 : 4; }

// An archive without records holds no records to pack: its block goes through the host.  -> mode
uint32_t pack_block_host(const uint8_t *block, size_t B, Bytes &section, uint64_t &bytes, uint64_t &seps) {
    std::vector<uint32_t> list;
    bool raw = false;
    for (size_t p = 0; p < B && !raw; ++p) {
        if (block[p] == 1) list.push_back((uint32_t)p);
        else raw = host_base_code(block[p]) > 3;
    }
    if (raw) {
        section = alloc_bytes(B);
        std::memcpy(section.get(), block, B);
        bytes = B;
        seps = 0;
        return 0;
    }
    const size_t q = packed_quarter(B);
    bytes = q + 4 * list.size();
    seps = list.size();
    section = alloc_bytes(bytes);
    std::memset(section.get(), 0, bytes);
    for (size_t p = 0; p < B; ++p) section.get()[p >> 2] |= (uint8_t)((host_base_code(block[p]) & 3) << (2 * (p & 3)));
    if (!list.empty()) std::memcpy(section.get() + q, list.data(), 4 * list.size());  // (little-endian host)
    return 1;
}

std::string rule_message(uint64_t index, uint32_t rule, const char *what = "record") {
    return std::string("rlz archive: ") + what + " " + std::to_string(index) + " breaks " + packed_rule_text(rule);
}

void unpack_block_host(const nolzss_rlz_archive_packed &in, std::vector<uint8_t> &block) {
    const size_t B = (size_t)in.block_length;
    block.resize(B);
    if (!in.block_mode) {
        if (B) std::memcpy(block.data(), in.block, B);
        return;
    }
    for (size_t p = 0; p < B; ++p) block[p] = (uint8_t)"ACGT"[(in.block[p >> 2] >> (2 * (p & 3))) & 3];
    const uint8_t *list = in.block + packed_quarter(B);
    uint64_t last = 0;
    for (uint64_t t = 0; t < in.num_separators; ++t) {
        uint32_t p;
        std::memcpy(&p, list + 4 * t, 4);
        if (p >= B || (t && p <= last)) throw std::invalid_argument(rule_message(t, kPackSeparatorList, "separator"));
        block[p] = 1;
        last = p;
    }
}

void pack_archive(const nolzss_rlz_archive &h, nolzss_rlz_archive_packed *out) {
    const size_t z = (size_t)h.z, B = (size_t)h.block_len, nlit = (size_t)h.n_literals;
    Bytes block, control, data, literals;
    uint64_t block_bytes = 0, data_bytes = 0, literal_bytes = 0, seps = 0;
    uint32_t block_mode = 1, literal_mode = 1;
    if (z == 0) {  // no record: no kernel (the block of an archive over an index comes down as it is)
        std::vector<uint8_t> tmp;
        const uint8_t *src = h.h_block.data();
        if (h.block && B) {
            tmp.resize(B);
            DeviceRestore restore;
            Session ses(h.device, nullptr);
            download_bytes(ses.ctx(), tmp.data(), h.block.as<uint8_t>(), B);
            src = tmp.data();
        }
        block_mode = pack_block_host(src, B, block, block_bytes, seps);
        control = alloc_bytes(0);
        data = alloc_bytes(0);
        literals = alloc_bytes(0);
    } else {
        DeviceRestore restore;
        Session ses(h.device, nullptr);
        Context &ctx = ses.ctx();
        hipStream_t s = ctx.stream;
        {  // (the scope closes before the stream is waited for and the profiler collected)
            ProfScope whole(ctx.profiler(), "rlz_archive_pack_all", s);
            // rank, offset and literal index 4 z each, diagonals 8 z, at most 9 z data bytes and z / 2 control bytes; the
            // literals raw and packed; the block's flags 4 B, its bases B / 4, its separators at most 4 B
            reserve_arena_for(ctx, 0, 30 * z + 2 * nlit + 9 * B + (size_t(4) << 20));
            const ArchiveRec *d_recs = h.recs.as<ArchiveRec>();
            const PackPlan plan = packed_plan(ctx, d_recs, z, (uint32_t)B, z - nlit);
            if (plan.data_bytes > 0xffffffffull)
                throw std::invalid_argument("rlz archive: the data stream of the compact form would hold " +
                                            std::to_string(plan.data_bytes) + " bytes, 2^32 or more are refused");
            data_bytes = plan.data_bytes;
            const size_t cb = (z + 1) / 2;
            control = alloc_bytes(cb);
            data = alloc_bytes((size_t)data_bytes);
            uint8_t *d_control = ctx.arena.alloc<uint8_t>(cb);
            uint8_t *d_data = ctx.arena.alloc<uint8_t>(data_bytes ? (size_t)data_bytes : 1);
            packed_write(ctx, d_recs, z, plan, d_control, d_data);
            {
                ProfScope ps(ctx.profiler(), "packed_d2h", s, (double)cb + (double)data_bytes);
                download_bytes(ctx, control.get(), d_control, cb);
                if (data_bytes) download_bytes(ctx, data.get(), d_data, (size_t)data_bytes);
            }
            uint8_t *d_raw = ctx.arena.alloc<uint8_t>(nlit ? nlit : 1);
            uint8_t *d_two = ctx.arena.alloc<uint8_t>(packed_quarter(nlit) + 1);
            literal_mode = packed_literals(ctx, d_recs, z, nlit, d_raw, d_two);
            literal_bytes = literal_mode ? packed_quarter(nlit) : nlit;
            literals = alloc_bytes((size_t)literal_bytes);
            if (literal_bytes) download_bytes(ctx, literals.get(), literal_mode ? d_two : d_raw, (size_t)literal_bytes);
            uint8_t *d_quarter = ctx.arena.alloc<uint8_t>(packed_quarter(B) + 1);
            uint32_t *d_seps = nullptr;
            uint32_t num_seps = 0;
            block_mode = packed_block(ctx, h.block.as<uint8_t>(), B, d_quarter, &d_seps, &num_seps);
            seps = block_mode ? num_seps : 0;
            block_bytes = block_mode ? packed_quarter(B) + 4 * (uint64_t)num_seps : B;
            block = alloc_bytes((size_t)block_bytes);
            ProfScope ps(ctx.profiler(), "packed_d2h", s, (double)block_bytes);
            if (!block_mode) {
                download_bytes(ctx, block.get(), h.block.as<uint8_t>(), B);
            } else {
                if (B) download_bytes(ctx, block.get(), d_quarter, packed_quarter(B));
                if (num_seps) download_bytes(ctx, block.get() + packed_quarter(B), d_seps, 4 * (size_t)num_seps);
            }
        }
        HIP_CHECK(hipStreamSynchronize(s));
        HIP_CHECK(hipGetLastError());
        ctx.prof.collect();
    }
    out->block_mode = block_mode;
    out->literal_mode = literal_mode;
    out->block_length = B;
    out->z = z;
    out->n_literals = nlit;
    out->decoded = h.decoded;
    out->num_separators = seps;
    out->block_bytes = block_bytes;
    out->control_bytes = (z + 1) / 2;
    out->data_bytes = data_bytes;
    out->literal_bytes = literal_bytes;
    out->block = block.release();
    out->control = control.release();
    out->data = data.release();
    out->literals = literals.release();
}

void open_packed(const nolzss_rlz_archive_packed *in, const uint64_t *target_lengths, size_t k, int device,
                 nolzss_rlz_archive **out) {
    if (!out) throw std::invalid_argument("output pointer is null");
    *out = nullptr;
    if (!in) throw std::invalid_argument("packed archive pointer is null");
    if (k && !target_lengths) throw std::invalid_argument("target_lengths pointer is null");
    const nolzss_rlz_archive_packed &a = *in;
    const uint64_t B = a.block_length, z = a.z, nlit = a.n_literals, decoded = a.decoded;
    if (B > kMaxText || decoded > kMaxText || B + decoded > kMaxText || nlit > kMaxText)
        throw std::invalid_argument("text too long: the device pipeline uses 32-bit indices");
    if (z > 0xffffffffull) throw std::invalid_argument("z: the position sample indexes records in 32 bits, 2^32 or more are refused");
    if (k > kMaxText) throw std::invalid_argument("too many targets: the device pipeline uses 32-bit indices");
    if (a.block_mode > 1 || a.literal_mode > 1) throw std::invalid_argument("rlz archive: packed: a mode is neither 0 nor 1");
    // the sizes of the sections, from the counts alone: every read below is bounded by them
    auto size_is = [](const char *name, uint64_t have, uint64_t want) {
        if (have != want)
            throw std::invalid_argument(std::string("rlz archive: packed: the ") + name + " section holds " + std::to_string(have) +
                                        " bytes, the counts ask for " + std::to_string(want));
    };
    if (!a.block_mode && a.num_separators) throw std::invalid_argument("rlz archive: packed: a raw block has no separator list");
    if (a.num_separators > B) throw std::invalid_argument("rlz archive: packed: more separators than block bytes");
    size_is("block", a.block_bytes, a.block_mode ? packed_quarter(B) + 4 * a.num_separators : B);
    size_is("control", a.control_bytes, (z + 1) / 2);
    size_is("literal", a.literal_bytes, a.literal_mode ? packed_quarter(nlit) : nlit);
    if (a.data_bytes > 0xffffffffull) throw std::invalid_argument("rlz archive: packed: a data section of 2^32 bytes or more");
    if ((a.block_bytes && !a.block) || (a.control_bytes && !a.control) || (a.data_bytes && !a.data) ||
        (a.literal_bytes && !a.literals))
        throw std::invalid_argument("rlz archive: packed: a section pointer is null");

    std::unique_ptr<nolzss_rlz_archive> h(new nolzss_rlz_archive);
    h->device = device;
    h->z = z;
    h->block_len = B;
    h->n_literals = nlit;
    h->decoded = decoded;
    h->lengths.assign(target_lengths, target_lengths + k);
    h->bases.resize(k + 1);
    uint64_t sum = 0;
    bool overflow = false;
    for (size_t j = 0; j < k; ++j) {
        h->bases[j] = sum;
        overflow |= sum + target_lengths[j] < sum;
        sum += target_lengths[j];
    }
    h->bases[k] = sum;
    auto sum_message = [&](uint64_t covered) {
        return "rlz archive: record " + std::to_string(z) + " (behind the last) breaks target boundary: the target lengths sum to " +
               std::to_string(sum) + ", the header counts " + std::to_string(decoded) + " and the records cover " +
               std::to_string(covered) + " bytes behind the block";
    };
    if (z == 0) {  // an empty archive: no device
        if (a.data_bytes) throw std::invalid_argument(rule_message(0, kPackDataSize));
        if (nlit) throw std::invalid_argument(rule_message(0, kPackLiteralCount));
        if (sum || overflow || decoded) throw std::invalid_argument(sum_message(0));
        unpack_block_host(a, h->h_block);
        *out = h.release();
        return;
    }
    std::vector<uint64_t> bounds(k + 1);  // decoded positions; saturating, a sum beyond 2^64 cannot be met by the records
    for (size_t j = 0; j <= k; ++j) bounds[j] = overflow ? (j ? ~0ull : 0) : h->bases[j];

    with_index_session(device, "rlz_archive_open_packed", [&](Context &ctx) {
        hipStream_t s = ctx.stream;
        const size_t samples = archive_samples((size_t)decoded);
        // the sections; offset, rank, length and position 4 z each, steps and their sums 16 z at most
        reserve_arena_for(ctx, 0, a.block_bytes + a.control_bytes + a.data_bytes + a.literal_bytes + sizeof(uint64_t) * (k + 1) +
                                      34 * z + (size_t(4) << 20));
        uint8_t *d_section = ctx.arena.alloc<uint8_t>(a.block_bytes ? a.block_bytes : 1);
        uint8_t *d_control = ctx.arena.alloc<uint8_t>(a.control_bytes);
        uint8_t *d_data = ctx.arena.alloc<uint8_t>(a.data_bytes ? a.data_bytes : 1);
        uint8_t *d_lit = ctx.arena.alloc<uint8_t>(a.literal_bytes ? a.literal_bytes : 1);
        uint64_t *d_bounds = ctx.arena.alloc<uint64_t>(k + 1);
        h->block.alloc(ctx, B ? B : 1);
        h->recs.alloc(ctx, sizeof(ArchiveRec) * z);
        h->sample.alloc(ctx, sizeof(uint32_t) * (samples ? samples : 1));
        h->cap_samples = samples;
        ArchiveRec *d_recs = h->recs.as<ArchiveRec>();
        {
            ProfScope ps(ctx.profiler(), "packed_h2d", s,
                         (double)(a.block_bytes + a.control_bytes + a.data_bytes + a.literal_bytes));
            if (a.block_mode) {
                if (a.block_bytes) upload_bytes(ctx, d_section, a.block, a.block_bytes);
            } else if (B) {
                upload_bytes(ctx, h->block.as<uint8_t>(), a.block, B);
            }
            upload_bytes(ctx, d_control, a.control, a.control_bytes);
            if (a.data_bytes) upload_bytes(ctx, d_data, a.data, a.data_bytes);
            if (a.literal_bytes) upload_bytes(ctx, d_lit, a.literals, a.literal_bytes);
            upload_bytes(ctx, d_bounds, bounds.data(), sizeof(uint64_t) * (k + 1));
        }
        try {
            if (a.block_mode) {
                const uint64_t bad = unpack_block(ctx, d_section, B, (uint32_t)a.num_separators, h->block.as<uint8_t>());
                if (bad != ~0ull) throw std::invalid_argument(rule_message(bad >> 4, (uint32_t)(bad & 15u), "separator"));
            }
            UnpackIn ui{};
            ui.control = d_control;
            ui.data = d_data;
            ui.literals = d_lit;
            ui.data_bytes = a.data_bytes;
            ui.n_literals = nlit;
            ui.literal_mode = a.literal_mode;
            ui.B = (uint32_t)B;
            ui.bounds = d_bounds;
            ui.k = (uint32_t)k;
            const UnpackOut res = unpack_records(ctx, ui, z, d_recs);
            if (res.bad != ~0ull) throw std::invalid_argument(rule_message(res.bad >> 4, (uint32_t)(res.bad & 15u)));
            if (z - res.copies != nlit)
                throw std::invalid_argument(rule_message(z, kPackLiteralCount) + ": the " + std::to_string(z) + " records hold " +
                                            std::to_string(z - res.copies) + " literals and n_literals is " + std::to_string(nlit));
            if (overflow || sum != decoded || res.covered != decoded) throw std::invalid_argument(sum_message(res.covered));
            archive_extend_sample(ctx, d_recs, 0u, (uint32_t)z, 0u, (uint32_t)samples, h->sample.as<uint32_t>());
        } catch (...) {
            (void)hipStreamSynchronize(s);  // nothing still reads the caller's sections or writes the handle's arrays when they go
            throw;
        }
    });
    *out = h.release();
}

}  // namespace

extern "C" {

int nolzss_rlz_archive_pack(const nolzss_rlz_archive *h, nolzss_rlz_archive_packed *out) {
    return guarded([&] {
        if (!out) throw std::invalid_argument("output pointer is null");
        std::memset(out, 0, sizeof *out);
        if (!h) throw std::invalid_argument("handle is null");
        pack_archive(*h, out);
    });
}

void nolzss_free_rlz_archive_packed(nolzss_rlz_archive_packed *p) {
    if (!p) return;
    std::free(p->block);
    std::free(p->control);
    std::free(p->data);
    std::free(p->literals);
    std::memset(p, 0, sizeof *p);
}

int nolzss_rlz_archive_open_packed(const nolzss_rlz_archive_packed *in, const uint64_t *target_lengths, size_t k, int device,
                                   nolzss_rlz_archive **h) {
    return guarded([&] { open_packed(in, target_lengths, k, device, h); });
}

}  // extern "C"
