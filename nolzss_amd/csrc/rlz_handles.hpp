// rlz_handles.hpp -- the resident relative-LZ handles and what the translation units of their entry points share: the
// index and its match (rlz_index_api.hip), its pattern queries (rlz_index_query_api.hip), the repeats of its reference
// (rlz_index_repeats_api.hip) and its seed queries
// (rlz_index_seeds_api.hip); the archive (rlz_archive_api.hip), whose appends run that match; a finder reads both
// (rlz_find_api.hip); a pileup reduces the alignments of the index (rlz_pileup_api.hip); a cohort packs the calls of
// pileups into bit planes and compares them (rlz_cohort_api.hip).  DESIGN.md 5, "Relative-LZ archive: batches appended from the index" and "Relative-LZ archive:
// locate through the parse".
#pragma once
#include <functional>

#include "api_internal.hpp"
#include "rlz_archive.hpp"
#include "rlz_find.hpp"
#include "rlz_index.hpp"

// Every handle keeps its device memory in DeviceBufs (device_buf.hpp; DESIGN.md 5, "Relative-LZ handles: who owns device
// memory"), so none has a destructor of its own, and zero bytes read as an empty handle.

// The index handle: everything a match reads, in one allocation; the view's pointers lead into it.  A match changes
// nothing here.
struct nolzss_rlz_index {
    int device = 0;
    uint64_t m = 0;
    uint64_t serial = 0;  // process-wide, given at open: an archive opened over this index remembers it
    nolzss::api::DeviceBuf base;
    nolzss::RlzIndexView view;
};

// The archive handle: the block, the packed records and the position sample.  The per-target table stays on the host:
// it is read when the ranges of a call are turned into decoded positions and prefix sums, which is all the kernel sees
// of the targets.
struct nolzss_rlz_archive {
    int device = 0;
    uint64_t z = 0, block_len = 0, n_literals = 0, decoded = 0;
    std::vector<uint64_t> lengths;  // k
    std::vector<uint64_t> bases;    // k + 1: decoded position of each target, then the decoded length
    nolzss::api::DeviceBuf block, recs, sample;
    std::vector<uint8_t> h_block;   // an archive without records holds no device memory: its block, for export
    // an archive opened over an index (index_serial != 0) grows by appends
    uint64_t index_serial = 0;
    size_t cap_samples = 0;  // words of the sample as reported: an open may allocate one word where it counts none
    size_t cap_recs() const { return recs.bytes() / sizeof(nolzss::ArchiveRec); }
    size_t device_bytes() const { return block.bytes() + recs.bytes() + sizeof(uint32_t) * cap_samples; }
    nolzss::ArchiveView view() const {
        return nolzss::ArchiveView{block.as<uint8_t>(), recs.as<nolzss::ArchiveRec>(), sample.as<uint32_t>(), (uint32_t)z,
                                   (uint32_t)nolzss::archive_samples((size_t)decoded)};
    }
};

// The finder handle: a snapshot of an archive opened over an index, for pattern queries in the targets (rlz_find_api.hip;
// DESIGN.md 5, "Relative-LZ archive: locate through the parse").  It points to the archive and the index it was opened
// over -- both must outlive it -- and holds the source table, the interval tables with the targets' decoded positions,
// and the index over the kernel text K.
struct nolzss_rlz_finder {
    int device = 0;
    const nolzss_rlz_archive *archive = nullptr;
    const nolzss_rlz_index *index = nullptr;
    uint64_t z = 0, targets = 0, decoded = 0;  // of the archive at the open: a query refuses an archive that has grown
    uint64_t M = 0, K_len = 0, intervals = 0;
    bool with_rc = false;
    nolzss::api::DeviceBuf tables;   // kstart, dstart, bases
    nolzss::api::DeviceBuf sources;  // lo, hi, rec and the upper levels of the max pyramid over hi
    nolzss::api::DeviceBuf kindex;   // everything kview points to
    nolzss::FinderView view;
    nolzss::RlzIndexView kview;
};

// The pileup handle: the counters of every position of the block of one index under one set of align parameters
// (rlz_pileup_api.hip; DESIGN.md 5, "Relative-LZ index: pileup").  It points to the index it was opened over, which must
// outlive it, and holds its counters in one allocation, zeroed at open.  `mu` serialises the calls on one pileup:
// several threads may add to it and read it, one at a time.
struct nolzss_rlz_pileup {
    int device = 0;
    const nolzss_rlz_index *index = nullptr;
    nolzss_rlz_align_params params{};
    nolzss::api::DeviceBuf base;
    nolzss::PileupView view;
    std::mutex mu;
    bool dirty = false;  // difference entries were added since the last resolve
    uint64_t targets = 0, alignments = 0, ops = 0, columns = 0, adds = 0;  // running totals
    // The insertion log: one event per I op of a kept alignment (none until the first event).  The allele table is built
    // from it on the first read after an add and kept until the next add.
    uint32_t flags = 0;  // NOLZSS_RLZ_PILEUP_*
    nolzss::api::DeviceBuf log, allele_table;
    uint64_t events = 0, alleles = 0;
    bool alleles_valid = false;
    uint64_t log_capacity() const { return log.bytes() / sizeof(nolzss::PileupEvent); }
};

// The cohort handle: the bit planes of the samples added so far over the block of one index (rlz_cohort_api.hip; DESIGN.md
// 5, "Relative-LZ index: cohort").  It points to the index it was opened over, which must outlive it, and remembers its
// serial; the planes lie sample-major in one allocation, none until the first add.  `mu` serialises the calls on one
// cohort.  Lock order: add_pileup takes the cohort's mutex first, then the pileup's, then the device's session; no call
// takes them the other way round.
struct nolzss_rlz_cohort {
    int device = 0;
    const nolzss_rlz_index *index = nullptr;
    uint64_t index_serial = 0;
    uint32_t B = 0;
    size_t W = 0;  // words of a plane: a sample keeps 3 W of them
    nolzss::api::DeviceBuf planes;
    uint64_t capacity = 0, first_capacity = 1;  // in samples; first_capacity: NOLZSS_RLZ_COHORT_SAMPLES or the default, read at open
    std::vector<nolzss_rlz_cohort_sample_info> samples;
    std::mutex mu;
};

// (the host tests pass 4096 zero bytes where a call hardly reads its handle)
static_assert(sizeof(nolzss_rlz_index) <= 4096 && sizeof(nolzss_rlz_archive) <= 4096 && sizeof(nolzss_rlz_finder) <= 4096 &&
                  sizeof(nolzss_rlz_pileup) <= 4096 && sizeof(nolzss_rlz_cohort) <= 4096,
              "a handle stays within the stand-in buffers of the host tests");

namespace nolzss {
namespace api {

// a Session makes the handle's device current: this puts the caller's back
struct DeviceRestore {
    int current = -1;
    bool known;
    DeviceRestore() : known(hipGetDevice(&current) == hipSuccess) {}
    ~DeviceRestore() {
        if (known) (void)hipSetDevice(current);
    }
};

constexpr size_t kRecordChunk = size_t(1) << 22;  // records per look-up chunk: 96 MiB of arena whatever the batch holds

// A batch of targets or patterns laid out for the device
constexpr uint8_t kSeparator = 1;  // between the targets of a batch: any byte but A, C, G, T
struct Batch {
    HostBytes tcat;                    // T1 s T2 s .. Tk s
    std::vector<uint32_t> separators;  // k positions in tcat
    std::vector<uint64_t> offsets;     // k: the first position of each target in tcat
};

// ---- the handle and its match (rlz_index_api.hip) ------------------------------------------------------------------
uint32_t choose_prefix(size_t index_length);  // the prefix table's key for an index text of that length
// device memory per batch position: packed text 1/4, code 4, rank 4, the chain's exits, bitmaps and node lists (12 on
// ordinary batches, 24 when every position is a node), the factor starts 4 -- not the 52 of a suffix sort
constexpr size_t kBatchBytesPerPosition = 36;
#pragma GCC visibility push(hidden)  // (between the translation units of the library: no new dynamic symbol)
// every check of a match, in the order the header states them, and the batch laid out
void prepare_batch(const nolzss_rlz_index &h, const char *const *targets, const size_t *target_lens, size_t k, Batch &b);
// the batch bytes into the arena (text_h2d) and packed with the ends of its targets or patterns as terminators
uint8_t *upload_and_pack(Context &ctx, const Batch &b, PackedText &packed);
// What every use of a match starts with: the batch up, packed with the target ends as terminators, and searched.
struct Searched {
    uint8_t *d_T;              // the batch bytes (upper case, separators)
    uint32_t *d_len, *d_rank;  // per position: the longest match and a rank that attains it
    PackedText batch;          // the packed batch: its terminator table holds the target ends
};
Searched search_batch(Context &ctx, const nolzss_rlz_index &h, const Batch &b);
// max_hits as the kernels take it: 0 and anything beyond 32 bits mean no cap
inline uint32_t hit_cap(uint64_t max_hits) {
    return (max_hits == 0 || max_hits >= 0xffffffffull) ? 0xffffffffu : (uint32_t)max_hits;
}
// true when `extra` bytes were beyond the arena: it was reserved anew and emptied, and the caller starts over in it
bool regrow_arena(Context &ctx, size_t extra);
// `count` records of `size` bytes from device memory into a host array, NOLZSS_RLZ_LOCATE_CHUNK records per copy
void download_records(Context &ctx, const char *scope, void *h_dst, const void *d_src, size_t count, size_t size);
// ... `chunk` at a time through d_stage, which produce(first, count) fills before each copy
void download_produced(Context &ctx, const char *scope, void *h_dst, const void *d_stage, size_t count, size_t size, size_t chunk,
                       const std::function<void(size_t, size_t)> &produce);
// `count` zeroed entries (one for count = 0) for a result that free_block releases; throws std::bad_alloc
template <typename T> T *calloc_array(size_t count) {
    T *p = static_cast<T *>(std::calloc(count ? count : 1, sizeof(T)));
    if (!p) throw std::bad_alloc();
    return p;
}
// f(ctx) in a session on `device` under the whole-call scope, then the stream's late errors and the profiler; the
// caller's device is current again on return
void with_index_session(int device, const char *scope, const std::function<void(Context &)> &f);
#pragma GCC visibility pop

// What a pattern query of the index and of the finder share (rlz_index_query_api.hip): the checks and the layout of a
// pattern batch, the chunk knobs, and the arena bytes of a batch of n positions and q patterns and of every expanded hit.
void prepare_patterns(const char *const *patterns, const size_t *pattern_lens, size_t q, Batch &b);
size_t chunk_knob(const char *name);
size_t pattern_batch_bytes(size_t n, size_t q);
constexpr size_t kLocateBytesPerHit = 25;
// What the seed-chain query and its debug hook (rlz_index_seeds_api.hip, debug_rlz.hip) share: the device's view of the
// parameters, and the chains of a run brought down into the host blocks of a result (anchor_offsets is allocated there;
// chunked by NOLZSS_RLZ_LOCATE_CHUNK).
ChainRules chain_rules(const nolzss_rlz_chain_params &p, uint64_t records, uint64_t B);
void deliver_chains(Context &ctx, const ChainsOut &run, nolzss_rlz_seed_chains_result &res);
// What the align query and the pileup (rlz_index_seeds_api.hip, rlz_pileup_api.hip) share.  The refusals of the
// parameters and of the batch's shape, each before any device work and in align's words; then, inside a session, the path
// of a batch of k >= 1 targets with at least one base up to its alignments, which stay in the arena with the packed batch:
// the refusals of the totals (returned as the message; `run` is then empty), the two arena reservations and the rerun
// rule.  extra_per_slot: bytes per column slot a consumer takes behind rlz_align_ops, reserved with the second
// reservation (an op is at most one per slot).
void check_align_params(const nolzss_rlz_align_params *params);
void check_align_batch_shape(const size_t *target_lens, size_t k);
struct AlignRun {
    AlignOut out;      // num_alignments == 0: no hit, no chain, or a refusal
    PackedText batch;  // the packed batch the alignments were computed from
    size_t num_jobs = 0, num_rows = 0;
};
std::string align_batch(Context &ctx, const nolzss_rlz_index &h, const Batch &b, size_t k, const nolzss_rlz_align_params &p,
                        size_t extra_per_slot, AlignRun &run);
// What the insertions and consensus queries of a pileup and their debug hook (rlz_pileup_api.hip, debug_rlz.hip) share:
// the refusals of the two rules, each before any device work, and the read-outs over resolved counters and an allele
// table of G entries (device memory), brought down into the host blocks of a result (chunked by NOLZSS_RLZ_LOCATE_CHUNK).
// A throw leaves what was allocated so far in the result: the caller frees it.  `records`: the reference records of
// the block.  Arena bytes the two take: kInsertionsArenaPerAllele per allele, kConsensusArenaPerBase per block base.
PileupRule check_pileup_rule(uint32_t min_count, uint64_t num, uint64_t den, const char *what);
ConsensusRule check_consensus_params(const nolzss_rlz_consensus_params *params);
constexpr size_t kAllelesArenaPerEvent = 100, kInsertionsArenaPerAllele = 9, kConsensusArenaPerBase = 9;
void deliver_insertions(Context &ctx, const PileupView &v, const PackedText &block, const PileupAllele *d_alleles, uint32_t G,
                        const PileupRule &rule, nolzss_rlz_insertions_result &out);
void deliver_consensus(Context &ctx, const PileupView &v, const PackedText &block, uint32_t records, const PileupAllele *d_alleles,
                       uint32_t G, const ConsensusRule &rule, bool want_map, nolzss_rlz_consensus_result &out);

}  // namespace api
}  // namespace nolzss
