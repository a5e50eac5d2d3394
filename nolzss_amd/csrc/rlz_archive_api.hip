// rlz_archive_api.hip -- the relative-LZ archive handle and its entry points: host records in, a resident form kept in
// device allocations of the handle's own, batches of ranges out (part of the C ABI layer of libnolzss_hip.so,
// include/nolzss_hip.h, nolzss_rlz_archive_*; the kernels: rlz_archive.hip; DESIGN.md 5, "Relative-LZ archive: ranges
// from resident records").  Export hands the host form back; open_index and append_index live in rlz_index_api.hip,
// next to the match they run ("Relative-LZ archive: batches appended from the index").
#include "rlz_handles.hpp"

using namespace nolzss;
using namespace nolzss::api;

namespace {

std::string literal_count_message(const nolzss_factor *f, size_t z, size_t n_literals) {
    size_t seen = 0;
    for (size_t k = 0; k < z; ++k)
        if (f[k].ref == f[k].start && seen++ == n_literals)
            return "rlz archive: record " + std::to_string(k) + " breaks literal count: it is literal number " +
                   std::to_string(n_literals + 1) + " and n_literals is " + std::to_string(n_literals);
    return "rlz archive: record " + std::to_string(z) + " (behind the last) breaks literal count: the " + std::to_string(z) +
           " records hold " + std::to_string(seen) + " literals and n_literals is " + std::to_string(n_literals);
}

std::string length_sum_message(size_t z, uint64_t sum, uint64_t decoded) {
    return "rlz archive: record " + std::to_string(z) + " (behind the last) breaks target boundary: the target lengths sum to " +
           std::to_string(sum) + " and the records cover " + std::to_string(decoded) + " bytes behind the block";
}

void open_records(const uint8_t *block, size_t block_len, const nolzss_factor *records, size_t z, const uint8_t *literals,
                  size_t n_literals, const uint64_t *target_lengths, size_t k, int device, nolzss_rlz_archive **out) {
    if (!out) throw std::invalid_argument("output pointer is null");
    *out = nullptr;
    if (block_len && !block) throw std::invalid_argument("block pointer is null");
    if (z && !records) throw std::invalid_argument("records pointer is null");
    if (n_literals && !literals) throw std::invalid_argument("literals pointer is null");
    if (k && !target_lengths) throw std::invalid_argument("target_lengths pointer is null");
    if (block_len > kMaxText) throw std::invalid_argument("text too long: the device pipeline uses 32-bit indices");
    if (z > 0xffffffffull) throw std::invalid_argument("z: the position sample indexes records in 32 bits, 2^32 or more are refused");
    if (k > kMaxText) throw std::invalid_argument("too many targets: the device pipeline uses 32-bit indices");

    std::unique_ptr<nolzss_rlz_archive> h(new nolzss_rlz_archive);
    h->device = device;
    h->z = z;
    h->block_len = block_len;
    h->n_literals = n_literals;
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

    if (z == 0) {  // an empty archive: no device
        if (n_literals) throw std::invalid_argument(literal_count_message(records, 0, n_literals));
        if (sum || overflow) throw std::invalid_argument(length_sum_message(0, sum, 0));
        h->h_block.assign(block, block + block_len);  // (export hands it back; device_bytes stays 0)
        *out = h.release();
        return;
    }
    const nolzss_factor &last = records[z - 1];
    const uint64_t n = last.start + last.length;
    if (n < last.start || n > kMaxText || n_literals > kMaxText)
        throw std::invalid_argument("text too long: the device pipeline uses 32-bit indices");
    // (n below block_len + z cannot tile: the check kernel names the record, nothing is sized by n before it)
    const uint64_t decoded = n > block_len ? n - block_len : 0;
    h->decoded = decoded;
    std::vector<uint64_t> bounds(k + 1);  // absolute; saturating, a sum beyond 2^64 cannot be met by the records anyway
    for (size_t j = 0; j <= k; ++j) bounds[j] = overflow || h->bases[j] > ~0ull - block_len ? ~0ull : block_len + h->bases[j];

    DeviceRestore restore;
    Session ses(device, nullptr);
    Context &ctx = ses.ctx();
    hipStream_t s = ctx.stream;
    ProfScope whole(ctx.profiler(), "rlz_archive_open", s);
    const size_t samples = archive_samples((size_t)decoded);
    reserve_arena_for(ctx, 0, sizeof(Rec) * z + n_literals + sizeof(uint64_t) * (k + 1) + 4 * z + 4 * (z / 4096 + 2) * 2 +
                                  (size_t(1) << 20));
    Rec *d_raw = ctx.arena.alloc<Rec>(z);
    uint8_t *d_lit = ctx.arena.alloc<uint8_t>(n_literals ? n_literals : 1);
    uint64_t *d_bounds = ctx.arena.alloc<uint64_t>(k + 1);
    uint32_t *lit_flags = ctx.arena.alloc<uint32_t>(z);
    {
        ProfScope ps(ctx.profiler(), "records_h2d", s, 24.0 * (double)z);
        upload_bytes(ctx, d_raw, records, sizeof(Rec) * z);
    }
    if (n_literals) upload_bytes(ctx, d_lit, literals, n_literals);
    upload_bytes(ctx, d_bounds, bounds.data(), sizeof(uint64_t) * (k + 1));
    const ArchiveCheck chk = archive_check(ctx, d_raw, z, block_len, n, d_bounds, k, lit_flags);  // (waits for the uploads)
    if (chk.bad != ~0ull) {
        const uint64_t rec = chk.bad >> 3;
        throw std::invalid_argument("rlz archive: record " + std::to_string(rec) + " breaks " +
                                    archive_rule_text((uint32_t)(chk.bad & 7u)));
    }
    if (chk.literals != n_literals) throw std::invalid_argument(literal_count_message(records, z, n_literals));
    if (overflow || sum != decoded) throw std::invalid_argument(length_sum_message(z, sum, decoded));

    const size_t block_bytes = block_len ? block_len : 1;
    h->d_block = static_cast<uint8_t *>(device_alloc(ctx, block_bytes));
    h->d_recs = static_cast<ArchiveRec *>(device_alloc(ctx, sizeof(ArchiveRec) * z));
    h->d_sample = static_cast<uint32_t *>(device_alloc(ctx, sizeof(uint32_t) * samples));
    h->device_bytes = block_bytes + sizeof(ArchiveRec) * z + sizeof(uint32_t) * samples;
    h->cap_recs = z;
    h->cap_samples = samples;
    if (block_len) upload_bytes(ctx, h->d_block, block, block_len);
    archive_pack(ctx, d_raw, z, block_len, n, lit_flags, d_lit, h->d_recs, h->d_sample);
    HIP_CHECK(hipStreamSynchronize(s));
    ctx.prof.collect();
    *out = h.release();
}

// The ranges of one call against the handle's target table -> prefix sums of the lengths (q + 1) and the decoded
// position of each range's first byte (q).  Returns the total.
uint64_t plan_ranges(const nolzss_rlz_archive &h, const nolzss_rlz_range *ranges, size_t q, std::vector<uint32_t> &plan) {
    if (q && !ranges) throw std::invalid_argument("ranges pointer is null");
    if (q > 0xfffffffeull) throw std::invalid_argument("rlz archive: 2^32 - 1 or more ranges in one call");
    const uint64_t k = h.lengths.size();
    uint64_t total = 0;
    for (size_t i = 0; i < q; ++i) {
        const nolzss_rlz_range &r = ranges[i];
        auto who = [i] { return "rlz archive: range " + std::to_string(i); };  // (built for a refused range only)
        if (r.target >= k)
            throw std::invalid_argument(who() + ": target " + std::to_string(r.target) + " of an archive of " + std::to_string(k) +
                                        " targets");
        if (r.lo > r.hi)
            throw std::invalid_argument(who() + ": lo exceeds hi (" + std::to_string(r.lo) + " > " + std::to_string(r.hi) + ")");
        if (r.hi > h.lengths[r.target])
            throw std::invalid_argument(who() + ": hi exceeds the length of target " + std::to_string(r.target) + " (" +
                                        std::to_string(r.hi) + " > " + std::to_string(h.lengths[r.target]) + ")");
        total += r.hi - r.lo;
        if (total > 0xffffffffull)
            throw std::invalid_argument(who() + ": the call reaches 2^32 bytes of output here, split it");
    }
    plan.resize(2 * q + 1);
    uint32_t at = 0;
    for (size_t i = 0; i < q; ++i) {
        plan[i] = at;
        plan[q + 1 + i] = (uint32_t)(h.bases[ranges[i].target] + ranges[i].lo);
        at += (uint32_t)(ranges[i].hi - ranges[i].lo);
    }
    plan[q] = at;
    return total;
}

std::string complement_message(const nolzss_rlz_range *ranges, uint64_t key) {
    const uint64_t i = key >> 32, byte = key & 0xffffffffull;
    return "rlz archive: range " + std::to_string(i) + " breaks complement of a non-nucleotide: position " +
           std::to_string(ranges[i].lo + byte) + " of target " + std::to_string(ranges[i].target) + " (byte " +
           std::to_string(byte) + " of the range) is a reverse-complement copy of a byte that is not A, C, G or T";
}

// to_device: into capacity bytes at d_user, the caller's device memory; else the bytes come back in a malloc'ed host array
void extract(const nolzss_rlz_archive &h, const nolzss_rlz_range *ranges, size_t q, bool to_device, uint8_t *d_user,
             size_t capacity, void *stream, uint8_t **bytes, uint64_t **offsets, uint64_t *total_out) {
    std::vector<uint32_t> plan;
    const uint64_t total = plan_ranges(h, ranges, q, plan);
    if (to_device) {
        if (capacity < total)
            throw std::invalid_argument("rlz archive: range " + std::to_string(q) + " (behind the last): d_out_capacity " +
                                        std::to_string(capacity) + " is below the " + std::to_string(total) + " bytes of the call");
        if (total && !d_user) throw std::invalid_argument("d_out is null");
    }
    uint8_t *h_bytes = nullptr;
    uint64_t *h_offsets = nullptr;
    if (!to_device) {
        h_bytes = static_cast<uint8_t *>(std::malloc(total ? total : 1));
        h_offsets = static_cast<uint64_t *>(std::malloc(sizeof(uint64_t) * (q + 1)));
        if (!h_bytes || !h_offsets) {
            std::free(h_bytes);
            std::free(h_offsets);
            throw std::bad_alloc();
        }
        for (size_t i = 0; i <= q; ++i) h_offsets[i] = plan[i];
    }
    try {
        if (total) {
            DeviceRestore restore;
            Session ses(h.device, stream);
            Context &ctx = ses.ctx();
            hipStream_t s = ctx.stream;
            if (to_device && !stream) order_behind_default_stream(ctx);
            reserve_arena_for(ctx, 0, sizeof(uint32_t) * plan.size() + (to_device ? 0 : total) + (size_t(1) << 20));
            uint32_t *d_plan = ctx.arena.alloc<uint32_t>(plan.size());
            unsigned long long *d_err = ctx.arena.alloc<unsigned long long>(1);
            uint8_t *d_out = to_device ? d_user : ctx.arena.alloc<uint8_t>(total);
            {
                ProfScope ps(ctx.profiler(), "ranges_h2d", s, 4.0 * (double)plan.size());
                upload_bytes(ctx, d_plan, plan.data(), sizeof(uint32_t) * plan.size());
            }
            HIP_CHECK(hipMemsetAsync(d_err, 0xff, sizeof(unsigned long long), s));
            const ArchiveView v{h.d_block, h.d_recs, h.d_sample, (uint32_t)h.z, (uint32_t)archive_samples((size_t)h.decoded)};
            archive_extract(ctx, v, d_plan, d_plan + q + 1, (uint32_t)q, (uint32_t)total, d_out, d_err);
            uint32_t e[2];
            ctx.read_back(reinterpret_cast<const uint32_t *>(d_err), e, 2);  // (waits for the kernel)
            const uint64_t key = (uint64_t)e[0] | ((uint64_t)e[1] << 32);
            if (key != ~0ull) throw std::invalid_argument(complement_message(ranges, key));
            if (h_bytes) {
                ProfScope ps(ctx.profiler(), "text_d2h", s, (double)total);
                download_bytes(ctx, h_bytes, d_out, (size_t)total);
            }
            ctx.prof.collect();
        }
    } catch (...) {
        std::free(h_bytes);
        std::free(h_offsets);
        throw;
    }
    if (!to_device) {
        *bytes = h_bytes;
        *offsets = h_offsets;
    }
    *total_out = total;
}

// The host form back: block, 24-byte records and the literal stream, each downloaded once.
void export_archive(const nolzss_rlz_archive &h, uint8_t **block, size_t *block_len, nolzss_factor **records, size_t *z,
                    uint8_t **literals, size_t *n_literals) {
    const size_t zz = (size_t)h.z, nlit = (size_t)h.n_literals, blen = (size_t)h.block_len;
    std::unique_ptr<uint8_t, FreeBlock> h_blk(static_cast<uint8_t *>(std::malloc(blen ? blen : 1)));
    std::unique_ptr<uint8_t, FreeBlock> h_lit(static_cast<uint8_t *>(std::malloc(nlit ? nlit : 1)));
    FactorBlock h_recs(static_cast<nolzss_factor *>(alloc_factor_block(sizeof(nolzss_factor) * (zz ? zz : 1))));
    if (!h_blk || !h_lit || !h_recs) throw std::bad_alloc();
    if (!h.d_block) {  // no records and no device memory: the host copy of the block
        if (blen) std::memcpy(h_blk.get(), h.h_block.data(), blen);
    } else {
        DeviceRestore restore;
        Session ses(h.device, nullptr);
        Context &ctx = ses.ctx();
        hipStream_t s = ctx.stream;
        {  // (the scope closes before the stream is waited for and the profiler collected)
            ProfScope whole(ctx.profiler(), "rlz_archive_export_all", s);
            const size_t chunk = zz < kRecordChunk ? zz : kRecordChunk;
            reserve_arena_for(ctx, 0, sizeof(uint32_t) * zz + nlit + sizeof(Rec) * chunk + (size_t(4) << 20));
            if (blen) {
                ProfScope ps(ctx.profiler(), "block_d2h", s, (double)blen);
                download_bytes(ctx, h_blk.get(), h.d_block, blen);
            }
            if (zz) {
                uint32_t *d_index = ctx.arena.alloc<uint32_t>(zz);
                uint8_t *d_lit = ctx.arena.alloc<uint8_t>(nlit ? nlit : 1);
                Rec *d_out = ctx.arena.alloc<Rec>(chunk);
                const uint64_t found = archive_literal_index(ctx, h.d_recs, zz, d_index);
                if (found != h.n_literals)
                    throw HipError("rlz archive: the resident records do not hold the literals the handle counts");
                for (size_t c0 = 0; c0 < zz; c0 += chunk) {
                    const size_t cnt = zz - c0 < chunk ? zz - c0 : chunk;
                    archive_export_records(ctx, h.d_recs, c0, cnt, h.block_len, d_index, d_out, d_lit);
                    ProfScope ps(ctx.profiler(), "factors_d2h", s, (double)(sizeof(Rec) * cnt));
                    download_bytes(ctx, h_recs.get() + c0, d_out, sizeof(Rec) * cnt);  // (waits: d_out is free again)
                }
                if (nlit) download_bytes(ctx, h_lit.get(), d_lit, nlit);
            }
        }
        HIP_CHECK(hipStreamSynchronize(s));
        ctx.prof.collect();
    }
    *block = h_blk.release();
    *block_len = blen;
    *records = h_recs.release();
    *z = zz;
    *literals = h_lit.release();
    *n_literals = nlit;
}

}  // namespace

extern "C" {

int nolzss_rlz_archive_open_records(const uint8_t *block, size_t block_len, const nolzss_factor *records, size_t z,
                                    const uint8_t *literals, size_t n_literals, const uint64_t *target_lengths, size_t k,
                                    int device, nolzss_rlz_archive **h) {
    return guarded([&] { open_records(block, block_len, records, z, literals, n_literals, target_lengths, k, device, h); });
}

int nolzss_rlz_archive_info(const nolzss_rlz_archive *h, nolzss_rlz_archive_summary *info) {
    return guarded([&] {
        if (!h || !info) throw std::invalid_argument("handle or output pointer is null");
        std::memset(info, 0, sizeof *info);
        info->num_targets = h->lengths.size();
        info->block_length = h->block_len;
        info->z = h->z;
        info->n_literals = h->n_literals;
        info->total_length = h->bases.back();
        info->target_lengths = h->lengths.empty() ? nullptr : h->lengths.data();
        info->device = h->device;
        info->device_bytes = h->device_bytes;
    });
}

int nolzss_rlz_archive_extract(const nolzss_rlz_archive *h, const nolzss_rlz_range *ranges, size_t q, uint8_t **bytes,
                               uint64_t **offsets, uint64_t *total) {
    return guarded([&] {
        if (!bytes || !offsets || !total) throw std::invalid_argument("output pointer is null");
        *bytes = nullptr;
        *offsets = nullptr;
        *total = 0;
        if (!h) throw std::invalid_argument("handle is null");
        extract(*h, ranges, q, false, nullptr, 0, nullptr, bytes, offsets, total);
    });
}

int nolzss_rlz_archive_extract_device(const nolzss_rlz_archive *h, const nolzss_rlz_range *ranges, size_t q, void *d_out,
                                      size_t d_out_capacity, void *stream, uint64_t *total) {
    return guarded([&] {
        if (!total) throw std::invalid_argument("output pointer is null");
        *total = 0;
        if (!h) throw std::invalid_argument("handle is null");
        extract(*h, ranges, q, true, static_cast<uint8_t *>(d_out), d_out_capacity, stream, nullptr, nullptr, total);
    });
}

int nolzss_rlz_archive_export(const nolzss_rlz_archive *h, uint8_t **block, size_t *block_len, nolzss_factor **records,
                              size_t *z, uint8_t **literals, size_t *n_literals) {
    return guarded([&] {
        if (!block || !block_len || !records || !z || !literals || !n_literals)
            throw std::invalid_argument("output pointer is null");
        *block = nullptr;
        *records = nullptr;
        *literals = nullptr;
        *block_len = *z = *n_literals = 0;
        if (!h) throw std::invalid_argument("handle is null");
        export_archive(*h, block, block_len, records, z, literals, n_literals);
    });
}

int nolzss_rlz_archive_close(nolzss_rlz_archive *h) {
    return guarded([&] { delete h; });
}

}  // extern "C"
