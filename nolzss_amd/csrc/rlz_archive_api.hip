// rlz_archive_api.hip -- the relative-LZ archive handle and its entry points: host records in, a resident form kept in
// device allocations of the handle's own, batches of ranges out (part of the C ABI layer of libnolzss_hip.so,
// include/nolzss_hip.h, nolzss_rlz_archive_*; the kernels: rlz_archive.hip; DESIGN.md 5, "Relative-LZ archive: ranges
// from resident records").  Export hands the host form back.  Also nolzss_rlz_archive_open_index / _append_index: the
// archive opened over an index and the batches appended to it on the device, which run the index's match
// (search_batch, rlz_index_api.hip; DESIGN.md 5, "Relative-LZ archive: batches appended from the index").
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
        h->h_block.assign(block, block + block_len);  // (export hands it back)
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

    h->block.alloc(ctx, block_len ? block_len : 1);
    h->recs.alloc(ctx, sizeof(ArchiveRec) * z);
    h->sample.alloc(ctx, sizeof(uint32_t) * samples);
    h->cap_samples = samples;
    if (block_len) upload_bytes(ctx, h->block.get(), block, block_len);
    archive_pack(ctx, d_raw, z, block_len, n, lit_flags, d_lit, h->recs.as<ArchiveRec>(), h->sample.as<uint32_t>());
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
            archive_extract(ctx, h.view(), d_plan, d_plan + q + 1, (uint32_t)q, (uint32_t)total, d_out, d_err);
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
    HostBlock<uint8_t> h_blk = host_block<uint8_t>(blen), h_lit = host_block<uint8_t>(nlit);
    FactorBlock h_recs = host_block<nolzss_factor>(zz);
    if (!h.block) {  // no records and no device memory: the host copy of the block
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
                download_bytes(ctx, h_blk.get(), h.block.get(), blen);
            }
            if (zz) {
                uint32_t *d_index = ctx.arena.alloc<uint32_t>(zz);
                uint8_t *d_lit = ctx.arena.alloc<uint8_t>(nlit ? nlit : 1);
                Rec *d_out = ctx.arena.alloc<Rec>(chunk);
                const uint64_t found = archive_literal_index(ctx, h.recs.as<ArchiveRec>(), zz, d_index);
                if (found != h.n_literals)
                    throw HipError("rlz archive: the resident records do not hold the literals the handle counts");
                download_produced(ctx, "factors_d2h", h_recs.get(), d_out, zz, sizeof(Rec), chunk, [&](size_t c0, size_t cnt) {
                    archive_export_records(ctx, h.recs.as<ArchiveRec>(), c0, cnt, h.block_len, d_index, d_out, d_lit);
                });
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

// ---- the archive over an index: open, and batches appended on the device -------------------------------------------
void archive_open_index(const nolzss_rlz_index &ix, nolzss_rlz_archive **out) {
    if (!out) throw std::invalid_argument("output pointer is null");
    *out = nullptr;
    std::unique_ptr<nolzss_rlz_archive> h(new nolzss_rlz_archive);
    h->device = ix.device;
    h->block_len = ix.view.B;
    h->index_serial = ix.serial;
    h->bases.assign(1, 0);
    with_index_session(ix.device, "rlz_archive_open_index", [&](Context &ctx) {
        h->block.alloc(ctx, ix.view.B ? ix.view.B : 1);
        archive_unpack_block(ctx, ix.view.text, ix.view.B, h->block.as<uint8_t>());
    });
    *out = h.release();
}

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
    info->capacity_records = a.cap_recs();
    info->device_bytes = a.device_bytes();
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
    // the arrays that replace the handle's when it grows: swapped in at the commit, so what they hold on the way out goes
    DeviceBuf fresh_recs, fresh_sample;
    ArchiveRec *recs = a.recs.as<ArchiveRec>();
    uint32_t *sample = a.sample.as<uint32_t>();
    size_t cap_recs = a.cap_recs(), cap_samples = a.cap_samples;
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
            fresh_recs.alloc(ctx, sizeof(ArchiveRec) * cap_recs);
            recs = fresh_recs.as<ArchiveRec>();
            if (a.z) HIP_CHECK(hipMemcpyAsync(recs, a.recs.get(), sizeof(ArchiveRec) * a.z, hipMemcpyDeviceToDevice, s));
        }
        if (samples_new > cap_samples) {
            cap_samples = std::max<size_t>(samples_new, 2 * cap_samples);
            fresh_sample.alloc(ctx, sizeof(uint32_t) * cap_samples);
            sample = fresh_sample.as<uint32_t>();
            if (samples_old)
                HIP_CHECK(hipMemcpyAsync(sample, a.sample.get(), sizeof(uint32_t) * samples_old, hipMemcpyDeviceToDevice, s));
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
    const bool moved = fresh_recs || fresh_sample;
    if (fresh_recs) a.recs.swap(fresh_recs);
    if (fresh_sample) a.sample.swap(fresh_sample);
    a.cap_samples = cap_samples;
    a.z = z_new;
    a.n_literals += lit_added;
    for (size_t j = 0; j < k; ++j) {
        a.lengths.push_back(target_lens[j]);
        a.decoded += target_lens[j];
        a.bases.push_back(a.decoded);
    }
    fill_append_info(a, info, k, added, lit_added, bases, moved);
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
        info->device_bytes = h->device_bytes();
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

int nolzss_rlz_archive_close(nolzss_rlz_archive *h) {
    return guarded([&] { delete h; });
}

}  // extern "C"
