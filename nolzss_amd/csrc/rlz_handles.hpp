// rlz_handles.hpp -- the resident relative-LZ handles, shared by the translation units of their entry points: an
// append matches a batch against the index (rlz_index_api.hip) and writes into the archive (rlz_archive_api.hip owns
// open_records, extract and export); a finder reads both (rlz_find_api.hip).  DESIGN.md 5, "Relative-LZ archive: batches
// appended from the index" and "Relative-LZ archive: locate through the parse".
#pragma once
#include "api_internal.hpp"
#include "rlz_archive.hpp"
#include "rlz_find.hpp"
#include "rlz_index.hpp"

// The index handle: everything a match reads, in ONE device allocation (not arena memory, which the next call on the
// device recycles); the view's pointers lead into it.  A match changes nothing here.
struct nolzss_rlz_index {
    int device = 0;
    uint64_t m = 0;
    uint64_t serial = 0;  // process-wide, given at open: an archive opened over this index remembers it
    void *d_base = nullptr;
    size_t device_bytes = 0;
    nolzss::RlzIndexView view;
    ~nolzss_rlz_index() {  // (the calling thread's current device stays what it was)
        if (!d_base) return;
        int current = -1;
        const bool known = hipGetDevice(&current) == hipSuccess;
        (void)hipSetDevice(device);
        (void)hipFree(d_base);
        if (known && current != device) (void)hipSetDevice(current);
    }
};

// The archive handle: the block, the packed records and the position sample in device allocations of its own (not arena
// memory, which the next call on the device recycles).  The per-target table stays on the host: it is read when the
// ranges of a call are turned into decoded positions and prefix sums, which is all the kernel sees of the targets.
struct nolzss_rlz_archive {
    int device = 0;
    uint64_t z = 0, block_len = 0, n_literals = 0, decoded = 0;
    std::vector<uint64_t> lengths;  // k
    std::vector<uint64_t> bases;    // k + 1: decoded position of each target, then the decoded length
    uint8_t *d_block = nullptr;
    nolzss::ArchiveRec *d_recs = nullptr;
    uint32_t *d_sample = nullptr;
    size_t device_bytes = 0;
    std::vector<uint8_t> h_block;   // an archive without records holds no device memory: its block, for export
    // an archive opened over an index (index_serial != 0) grows by appends: what its two arrays can hold
    uint64_t index_serial = 0;
    size_t cap_recs = 0, cap_samples = 0;
    ~nolzss_rlz_archive() {  // (the calling thread's current device stays what it was)
        if (!d_block && !d_recs && !d_sample) return;
        int current = -1;
        const bool known = hipGetDevice(&current) == hipSuccess;
        (void)hipSetDevice(device);
        if (d_block) (void)hipFree(d_block);
        if (d_recs) (void)hipFree(d_recs);
        if (d_sample) (void)hipFree(d_sample);
        if (known && current != device) (void)hipSetDevice(current);
    }
};

// The finder handle: a snapshot of an archive opened over an index, for pattern queries in the targets (rlz_find_api.hip;
// DESIGN.md 5, "Relative-LZ archive: locate through the parse").  It points to the archive and the index it was opened
// over -- both must outlive it -- and holds in device allocations of its own (not arena memory) the source table, the
// interval tables with the targets' decoded positions, and the index over the kernel text K.
struct nolzss_rlz_finder {
    int device = 0;
    const nolzss_rlz_archive *archive = nullptr;
    const nolzss_rlz_index *index = nullptr;
    uint64_t z = 0, targets = 0, decoded = 0;  // of the archive at the open: a query refuses an archive that has grown
    uint64_t M = 0, K_len = 0, intervals = 0;
    bool with_rc = false;
    void *d_tables = nullptr;  // kstart, dstart, bases
    void *d_sources = nullptr; // lo, hi, rec and the upper levels of the max pyramid over hi
    void *d_kindex = nullptr;  // everything kview points to
    size_t device_bytes = 0;
    nolzss::FinderView view;
    nolzss::RlzIndexView kview;
    ~nolzss_rlz_finder() {  // (the calling thread's current device stays what it was)
        if (!d_tables && !d_sources && !d_kindex) return;
        int current = -1;
        const bool known = hipGetDevice(&current) == hipSuccess;
        (void)hipSetDevice(device);
        if (d_tables) (void)hipFree(d_tables);
        if (d_sources) (void)hipFree(d_sources);
        if (d_kindex) (void)hipFree(d_kindex);
        if (known && current != device) (void)hipSetDevice(current);
    }
};

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

// A batch of targets or patterns laid out for the device (rlz_index_api.hip)
constexpr uint8_t kSeparator = 1;  // between the targets of a batch: any byte but A, C, G, T
struct Batch {
    HostBytes tcat;                    // T1 s T2 s .. Tk s
    std::vector<uint32_t> separators;  // k positions in tcat
    std::vector<uint64_t> offsets;     // k: the first position of each target in tcat
};
// What a pattern query of the index and of the finder share (rlz_index_api.hip): the checks and the layout of a pattern
// batch, the chunk knobs, and the arena bytes of a batch of n positions and q patterns and of every expanded hit.
void prepare_patterns(const char *const *patterns, const size_t *pattern_lens, size_t q, Batch &b);
uint32_t choose_prefix(size_t index_length);  // the prefix table's key for an index text of that length
size_t chunk_knob(const char *name);
size_t pattern_batch_bytes(size_t n, size_t q);
constexpr size_t kLocateBytesPerHit = 25;
// What the seed-chain query and its debug hook (debug_rlz.hip) share: the device's view of the parameters, and the chains
// of a run brought down into the host blocks of a result (anchor_offsets is allocated there; chunked by
// NOLZSS_RLZ_LOCATE_CHUNK).
ChainRules chain_rules(const nolzss_rlz_chain_params &p, uint64_t records, uint64_t B);
void deliver_chains(Context &ctx, const ChainsOut &run, nolzss_rlz_seed_chains_result &res);

}  // namespace api
}  // namespace nolzss
