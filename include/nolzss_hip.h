/*
 * nolzss_hip.h -- C ABI of libnolzss_hip.so, the MI355X (gfx950) drop-in for the compiled core
 * of OmerKerner/noLZSS on the factorize path.
 *
 * Each entry point replaces one function that the reference's pybind11 module `_noLZSS`
 * (reference: src/cpp/bindings.cpp) binds for this path; the citation next to a declaration
 * names the reference interface it stands in for.  Plain pointers and sizes only: no C++,
 * pybind or torch types cross this boundary.  INTEGRATION.md shows the pybind11 / ctypes stub
 * a maintainer of the reference would add to bind these.
 *
 * Conventions
 *   - every function returns a status code (NOLZSS_OK == 0); on failure
 *     nolzss_last_error() returns a thread-local message.  NOLZSS_ERR_INVALID_ARGUMENT maps to
 *     the reference's std::invalid_argument (Python ValueError), NOLZSS_ERR_RUNTIME to
 *     std::runtime_error (RuntimeError)  -- bindings.cpp relies on pybind11's default mapping.
 *   - input buffers are borrowed for the duration of the call (bindings.cpp:66-67);
 *   - output arrays are allocated by the library and released with nolzss_free();
 *   - `device` is a HIP device ordinal; the library keeps one context (stream + device arena)
 *     per device and serialises calls on it, so calls are safe from any host thread
 *     (the reference releases the GIL around compute, bindings.cpp:70).
 *   - there is NO CPU fallback: without a usable GPU every compute entry point fails with
 *     NOLZSS_ERR_DEVICE.
 */
#ifndef NOLZSS_HIP_H
#define NOLZSS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* reference: struct Factor, src/cpp/factorizer.hpp:147-151 (24-byte POD, also the on-disk record) */
typedef struct nolzss_factor {
    uint64_t start;
    uint64_t length;
    uint64_t ref;
} nolzss_factor;

/* reference: RC_MASK, src/cpp/factorizer.hpp:41 */
#define NOLZSS_RC_MASK (1ULL << 63)

enum {
    NOLZSS_OK = 0,
    NOLZSS_ERR_INVALID_ARGUMENT = 1,
    NOLZSS_ERR_RUNTIME = 2,
    NOLZSS_ERR_NOMEM = 3,
    NOLZSS_ERR_DEVICE = 4,
    NOLZSS_ERR_IO = 5,
    NOLZSS_ERR_UNSUPPORTED = 6 /* the caller's own (host) path must handle this input */
};

const char *nolzss_last_error(void);
/* reference: m.attr("__version__"), bindings.cpp:1513-1517 */
const char *nolzss_version(void);
void nolzss_free(void *p);
int nolzss_device_count(int *count);

/* ---- plain mode ------------------------------------------------------------------------ */
/* reference: noLZSS::factorize(string_view, start_pos), factorizer.cpp:378-384;
 *            bound as _noLZSS.factorize, bindings.cpp:56-77 */
int nolzss_factorize(const uint8_t *text, size_t n, size_t start_pos, int device,
                     nolzss_factor **out, size_t *z);
/* reference: noLZSS::count_factors, factorizer.cpp:337-343; bindings.cpp:122-141 */
int nolzss_count_factors(const uint8_t *text, size_t n, size_t start_pos, int device, size_t *z);
/* reference: noLZSS::factorize_file, factorizer.cpp:401-406; bindings.cpp:96-105 */
int nolzss_factorize_file(const char *path, size_t start_pos, int device, nolzss_factor **out,
                          size_t *z);
/* reference: noLZSS::count_factors_file, factorizer.cpp:359-363; bindings.cpp:157-164 */
int nolzss_count_factors_file(const char *path, size_t start_pos, int device, size_t *z);

/* Same computation with the text already resident in device memory (d_text is a device
 * pointer on `device`); `stream` is a hipStream_t or NULL for the context's own stream.  With NULL the
 * call is ordered behind everything already queued on the legacy default stream (torch's default
 * stream); a producer of d_text on another non-blocking stream must be synchronised by the caller or
 * hand in its stream.
 * emit = 0: count only (the count_factors path);
 * emit = 1: build all z factor records in HBM and stop there (no PCIe transfer);
 * emit = 2: also copy them into a malloc'ed host array returned through out_host.
 * Used by bench.py (inputs resident in HBM when the clock starts) and by the shard dispatcher. */
int nolzss_factorize_device(const void *d_text, size_t n, size_t start_pos, int device,
                            void *stream, int emit, nolzss_factor **out_host, size_t *z);

/* ---- reverse-complement DNA mode ---------------------------------------------------------- */
/* reference: prepare_multiple_dna_sequences_w_rc, factorizer.cpp:54-172; bindings.cpp:732-740.
 * S (malloc'ed, may hold any byte value) = T1 s0 ... Tk s(k-1) rc(Tk) sk ... rc(T1) s(2k-1). */
int nolzss_prepare_multiple_dna_w_rc(const char *const *seqs, const size_t *lens, size_t k,
                                     uint8_t **S, size_t *S_len, size_t *original_length,
                                     uint64_t **sentinel_positions, size_t *n_sentinels);
/* reference: noLZSS::factorize_multiple_dna_w_rc, factorizer.cpp:651-656 over
 *            detail::nolzss_multiple_dna_w_rc, factorizer_core.hpp:177-383; bindings.cpp:361-382 */
int nolzss_factorize_multiple_dna_w_rc(const uint8_t *S, size_t S_len, size_t start_pos,
                                       int device, nolzss_factor **out, size_t *z);
/* reference: count_factors_multiple_dna_w_rc, factorizer.cpp:700-705; bindings.cpp:427-446 */
int nolzss_count_factors_multiple_dna_w_rc(const uint8_t *S, size_t S_len, size_t start_pos,
                                           int device, size_t *z);
/* reference: noLZSS::factorize_dna_w_rc, factorizer.cpp:519-523; bindings.cpp:207-228 */
int nolzss_factorize_dna_w_rc(const uint8_t *text, size_t n, int device, nolzss_factor **out,
                              size_t *z);
/* reference: noLZSS::count_factors_dna_w_rc, factorizer.cpp:559-561; bindings.cpp:276-295 */
int nolzss_count_factors_dna_w_rc(const uint8_t *text, size_t n, int device, size_t *z);
/* noLZSS::factorize_dna_w_rc (factorizer.cpp:519-523) with the text already resident in device memory: the
 * counterpart of nolzss_factorize_device for the reverse-complement mode (same `stream` and `emit` meaning; the
 * prepared string T s0 rc(T) s1 of factorizer.cpp:54-172 is built on the device).  Used by bench.py (BASELINE
 * config 5 with the input in HBM when the clock starts). */
int nolzss_factorize_dna_w_rc_device(const void *d_text, size_t n, int device, void *stream, int emit,
                                     nolzss_factor **out_host, size_t *z);

/* ---- reference + target factorization (the chain simply starts at start_pos) */
/* reference: noLZSS::factorize_w_reference, factorizer.cpp:940-955; bindings.cpp:868-880.
 * combined = reference 0x01 target, factorized from |reference| + 1; positions are absolute. */
int nolzss_factorize_w_reference(const uint8_t *reference_seq, size_t reference_len,
                                 const uint8_t *target_seq, size_t target_len, int device,
                                 nolzss_factor **out, size_t *z);
/* reference: noLZSS::factorize_dna_w_reference_seq, factorizer.cpp:825-842; bindings.cpp:800-808.
 * prepare({reference, target}) with reverse complements, factorized from |reference| + 1. */
int nolzss_factorize_dna_w_reference_seq(const char *reference_seq, size_t reference_len,
                                         const char *target_seq, size_t target_len, int device,
                                         nolzss_factor **out, size_t *z);

/* ---- v2 binary factor files -------------------------------------------- */
/* File = z 24-byte records, optional metadata, 48-byte footer "noLZSSv2", num_factors,
 * num_sequences, num_sentinels, footer_size, total_length (factorizer.hpp:64-77).
 * reference: write_factors_binary_file, factorizer.cpp:424-459 (input FILE -> output file) */
int nolzss_write_factors_binary_file(const char *in_path, const char *out_path, int device, size_t *z);
/* reference: write_factors_binary_file_dna_w_rc, factorizer.cpp:597-635 */
int nolzss_write_factors_binary_file_dna_w_rc(const char *in_path, const char *out_path, int device,
                                              size_t *z);
/* reference: factorize_w_reference_file, factorizer.cpp:980-1021 */
int nolzss_factorize_w_reference_file(const uint8_t *reference_seq, size_t reference_len,
                                      const uint8_t *target_seq, size_t target_len,
                                      const char *out_path, int device, size_t *z);
/* reference: factorize_dna_w_reference_seq_file, factorizer.cpp:851-883 */
int nolzss_factorize_dna_w_reference_seq_file(const char *reference_seq, size_t reference_len,
                                              const char *target_seq, size_t target_len,
                                              const char *out_path, int device, size_t *z);

/* Writes z records + `extra` metadata bytes (may be NULL) + the 48-byte v2 footer. */
int nolzss_write_factor_file(const char *out_path, const nolzss_factor *factors, size_t z,
                             uint64_t num_sequences, uint64_t num_sentinels, uint64_t total_length,
                             const void *extra, size_t extra_len);

/* ---- concatenated multi-sequence FASTA with sentinel bookkeeping ---------- */
/* reference: prepare_multiple_dna_sequences_no_rc, factorizer.cpp:199-294; bindings.cpp (same shape
 * as the w_rc variant): S = T1 s0 T2 s1 ... Tk (no sentinel after the last sequence), <= 250. */
int nolzss_prepare_multiple_dna_no_rc(const char *const *seqs, const size_t *lens, size_t k,
                                      uint8_t **S, size_t *S_len, size_t *original_length,
                                      uint64_t **sentinel_positions, size_t *n_sentinels);

typedef struct nolzss_fasta_result {   /* FastaFactorizationResult, fasta_processor.hpp */
    nolzss_factor *factors;
    size_t num_factors;
    uint64_t *sentinel_factor_indices; /* indices into factors[] of the sentinel literals */
    size_t num_sentinels;
    char *sequence_ids;                /* num_sequences NUL-terminated ids, back to back */
    size_t sequence_ids_bytes;
    size_t num_sequences;
} nolzss_fasta_result;

/* reference: factorize_fasta_multiple_dna_w_rc / _no_rc, fasta_processor.cpp:298-341 over
 * parse_fasta_sequences_and_ids (:28-128) and identify_sentinel_factors (:131-163).
 * sanitize_mode: 0 = "remove_ambiguous" (default of the bindings), 1 = "strict". */
int nolzss_factorize_fasta_multiple_dna(const char *fasta_path, int with_rc, int sanitize_mode,
                                        int device, nolzss_fasta_result *out);
void nolzss_free_fasta_result(nolzss_fasta_result *r);
/* reference: write_factors_binary_file_fasta_multiple_dna_w_rc / _no_rc (fasta_processor.cpp:345-360
 * -> parallel_fasta_processor.cpp:64-257): records, names, sentinel indices, footer with
 * total_length = sum of factor lengths. */
int nolzss_write_factors_binary_file_fasta_multiple_dna(const char *fasta_path, const char *out_path,
                                                        int with_rc, int sanitize_mode, int device,
                                                        size_t *z);

/* reference: factorize_dna_rc_w_ref_fasta_files, fasta_processor.cpp:362-378 over
 * prepare_ref_target_dna_w_rc_from_fasta (:240-287): all reference records, then all target records,
 * prepared with reverse complements; factorization starts at the first target base. */
int nolzss_factorize_dna_rc_w_ref_fasta_files(const char *reference_fasta_path, const char *target_fasta_path,
                                              int sanitize_mode, int device, nolzss_fasta_result *out);
/* reference: write_factors_dna_w_reference_fasta_files_to_binary, fasta_processor.cpp:381-390 */
int nolzss_write_factors_dna_w_reference_fasta_files_to_binary(const char *reference_fasta_path,
                                                               const char *target_fasta_path,
                                                               const char *out_path, int sanitize_mode,
                                                               int device, size_t *z);

/* Per-sequence FASTA factorization (each record on its own; no concatenation).
 * reference: factorize_/count_factors_/write_factors_binary_file_fasta_dna_{w,no}_rc_per_sequence,
 * fasta_processor.cpp:430-561, parallel_fasta_processor.cpp:262-465.  factors[j] / counts[j] per
 * record (factors is NULL when want_factors == 0); with out_dir != NULL every record is also
 * written to out_dir/<sanitised id>.bin (one name, no sentinels, total_length = sum of lengths).
 * Kept from the reference: the no-rc variants drop the last base of every record
 * (fasta_processor.cpp:469-471). */
typedef struct nolzss_fasta_per_sequence_result {
    nolzss_factor **factors;
    size_t *counts;
    char *sequence_ids;
    size_t sequence_ids_bytes;
    size_t num_sequences;
} nolzss_fasta_per_sequence_result;
int nolzss_factorize_fasta_per_sequence(const char *fasta_path, int with_rc, int sanitize_mode,
                                        int want_factors, const char *out_dir, int device,
                                        nolzss_fasta_per_sequence_result *out);
void nolzss_free_fasta_per_sequence_result(nolzss_fasta_per_sequence_result *r);

/* ---- per-sequence batch (the FASTA shard unit) ------------------------------------------- */
/* reference: the per-sequence factorize() loop of genomics.read_nucleotide_fasta,
 *            src/noLZSS/genomics/fasta.py:110-122 (C++ analogue:
 *            parallel_fasta_processor.cpp:360-385).  Sequence j is factorized on
 *            devices[j % n_dev]-th device of the list in longest-first order; out[j] / z[j]
 *            are per sequence (out may be NULL for counts only).
 *            Short records (fewer than NOLZSS_BATCH_MERGE_BELOW bases, default 2^21) that hold only
 *            A/C/G/T are factorized TOGETHER, as independent sequences of one device run (same
 *            results; 35 -> 3000 Mbases/s for 4 Ki-base records): out[j] may therefore point into a
 *            block shared with other records.  Free ONLY with nolzss_free_batch(). */
int nolzss_factorize_batch(const uint8_t *const *texts, const size_t *lens, size_t m,
                           const int *devices, size_t n_dev, nolzss_factor ***out, size_t **z);
/* The same with the reverse complement of every record: record j as factorize_dna_w_rc would
 * (prepare_multiple_dna_sequences_w_rc({seq}) + factorize_multiple_dna_w_rc, the per-record step of
 * factorize_fasta_dna_w_rc_per_sequence, fasta_processor.cpp:446-451; lower case accepted, refs of
 * reverse-complement factors carry NOLZSS_RC_MASK).  Short records are merged in the layout of
 * factorizer.cpp:128-169 (T1 s T2 s .. Tk s rc(Tk) s .. rc(T1) s) for any number of records, each
 * record seeing only itself and its own reverse complement.  An invalid nucleotide fails the call
 * like the reference ("Invalid nucleotide ... found in sequence 0"). */
int nolzss_factorize_batch_dna_w_rc(const uint8_t *const *texts, const size_t *lens, size_t m,
                                    const int *devices, size_t n_dev, nolzss_factor ***out, size_t **z);
void nolzss_free_batch(nolzss_factor **out, size_t *z, size_t m);
/* Extension: per-record factor counts in BOTH modes, from ONE suffix array per pipeline run.
 * count_w_rc[j] == nolzss_count_factors_dna_w_rc(texts[j]), count_no_rc[j] == nolzss_count_factors(texts[j])
 * (both caller-allocated, m entries).  The plain-mode L* is a by-product of the reverse-complement run: over
 * S = T s0 rc(T) s1 every earlier source of a position of T lies in T and no match runs past s0, so the plain
 * L* of S at i < |T| is the plain L* of T ("Both counts from one suffix sort").
 * Records: upper-case A/C/G/T only.  Planned and dealt like nolzss_factorize_batch_dna_w_rc (merged runs for
 * short records, single runs dealt longest-first over the device list).  Empty records give 0 / 0.  The first
 * record in input order that nolzss_count_factors_dna_w_rc refuses on its own fails the call with that
 * function's status and message (an invalid nucleotide: NOLZSS_ERR_RUNTIME, "Invalid nucleotide 'N' found in
 * sequence 0", RuntimeError in Python as there; a record too long for the reverse-complement path:
 * NOLZSS_ERR_INVALID_ARGUMENT).  Lower-case bases fail with NOLZSS_ERR_INVALID_ARGUMENT and a message of
 * their own: the plain count of `acgt` is not the plain count of `ACGT`.
 * reference: the per-record pair of compute_sequence_complexity_table, genomics/batch_factorize.py:370-429 */
int nolzss_count_factors_batch_both(const uint8_t *const *texts, const size_t *lens, size_t m,
                                    const int *devices, size_t n_dev, size_t *count_w_rc, size_t *count_no_rc);
/* The plain per-sequence batch with the records already in the memory of `device` (d_texts[j] = device
 * pointer to lens[j] bytes): no PCIe leg.  emit = 0 counts, emit = 1 also builds the factor records of
 * every record in HBM and stops there.  z[j] (caller-allocated, m entries) = factors of record j.  Used by
 * bench.py for the FASTA shard workload (inputs resident in HBM when the clock starts).
 * THIS CALL MAY SLEEP: records are merged into runs that several host threads ("lanes") submit, and when the first two
 * runs are of similar size the later lanes start up to NOLZSS_DEVICE_MERGE_STAGGER_MS (default 20 ms, scaled by the run
 * size) after the first, so that their bandwidth-bound and issue-bound phases overlap instead of coinciding. */
int nolzss_factorize_batch_device(const void *const *d_texts, const size_t *lens, size_t m, int device, int emit,
                                  size_t *z);

/* ---- genomics.read_nucleotide_fasta: FASTA file in, per-record factors out ---------------------- */
/* reference: read_nucleotide_fasta + _parse_fasta_content, src/noLZSS/genomics/fasta.py:28-126: parse
 * (id = first header word, bases upper-cased, white space dropped, a repeated id keeps its place and
 * takes the last record), check ^[ACGT]+$, then factorize() every record on its own (:110-122) -- here
 * as ONE per-sequence batch over the listed devices, the records read in one piece and handed to the
 * device as views of the read buffer.  Errors carry the reference's FASTAError texts ("Empty sequence
 * header at line N", "Sequence data before header at line N", "No valid sequences found in FASTA file",
 * "Sequence 'id' contains invalid nucleotides: {...}") with NOLZSS_ERR_RUNTIME; a file with non-ASCII
 * bytes returns NOLZSS_ERR_UNSUPPORTED (the Python layer then parses it itself).
 * Sharding (one process per GPU): with shard_count > 1 only the records that the longest-processing-
 * time-first plan gives to shard_index are factorized (owners[j] = shard of record j, the same on every
 * rank); counts[j] = 0 and factors[j] = NULL for the others, and the caller all-gathers the counts. */
typedef struct nolzss_nucleotide_fasta {
    char *sequence_ids;       /* num_sequences NUL-terminated ids, back to back, first-appearance order */
    size_t sequence_ids_bytes;
    size_t num_sequences;
    size_t *lengths;          /* bases per record */
    size_t *counts;           /* factors per record */
    size_t *owners;           /* shard that factorized the record */
    nolzss_factor **factors;  /* per record (NULL array when want_factors == 0) */
    void *keep;               /* owns the factor blocks */
} nolzss_nucleotide_fasta;
int nolzss_read_nucleotide_fasta(const char *path, const int *devices, size_t n_dev, int want_factors,
                                 size_t shard_index, size_t shard_count, nolzss_nucleotide_fasta *out);
void nolzss_free_nucleotide_fasta(nolzss_nucleotide_fasta *r);

/* ---- factor-length significance against a shuffled control ------------------------------------ */
/* reference: noLZSS.genomics.significance (src/noLZSS/genomics/significance.py) needs only the factor LENGTHS of a
 * genome and of a shuffled copy.  These calls give them without factor records: the lengths come straight from the
 * device's chain of factor starts ("Factor-length histograms and the keyed shuffle").
 *   fwd[L] / rc[L] (1 <= L < threshold): factors of length L on the forward / reverse-complement strand (rc is all
 *     zero in plain mode; index 0 is always 0);
 *   tail_lengths[j], tail_rc[j] (tail_count entries, ascending by (tail_rc, length)): the factors of length
 *     >= threshold;
 *   z = number of factors; lengths (lengths_count = z entries, the *_with_lengths calls only, NULL otherwise): the
 *     length of every factor in factor order.
 * Free with nolzss_free_length_hist(). */
typedef struct nolzss_length_hist {
    uint32_t threshold;
    uint64_t *fwd;
    uint64_t *rc;
    uint64_t *tail_lengths;
    uint8_t *tail_rc;
    size_t tail_count;
    size_t z;
    uint32_t *lengths;
    size_t lengths_count;
} nolzss_length_hist;
void nolzss_free_length_hist(nolzss_length_hist *h);
/* One text: plain mode (count_factors) or, with_rc != 0, the reverse-complement mode of count_factors_dna_w_rc, which
 * refuses the same texts with the same status and message.  shuffle != 0: the text is first permuted by the keyed
 * shuffle of nolzss_shuffle_dna(text, seed) (before the reverse complement is prepared). */
int nolzss_factor_length_histogram(const uint8_t *text, size_t n, int with_rc, int shuffle, uint64_t seed, int device,
                                   nolzss_length_hist *out);
/* The same without shuffle, with the lengths in factor order as well (one pipeline run). */
int nolzss_factor_length_histogram_with_lengths(const uint8_t *text, size_t n, int with_rc, int device,
                                                nolzss_length_hist *out);
/* The concatenated multiple-DNA FASTA form of nolzss_factorize_fasta_multiple_dna (same reader, sanitize_mode and
 * limits): the histogram of the factors of the prepared string S.  shuffle != 0: every record of S is permuted by
 * the keyed shuffle (record index = its place among the records of S), the sentinels stay where they are and the
 * reverse-complement half is rebuilt from the shuffled records -- S is then prepare(shuffled records). */
int nolzss_fasta_factor_length_histogram(const char *path, int with_rc, int sanitize_mode, int shuffle, uint64_t seed,
                                         int device, nolzss_length_hist *out);
int nolzss_fasta_factor_length_histogram_with_lengths(const char *path, int with_rc, int sanitize_mode, int device,
                                                      nolzss_length_hist *out);
/* The shuffled prepared string S of nolzss_fasta_factor_length_histogram (malloc'ed; nolzss_free). */
int nolzss_fasta_shuffled_text(const char *path, int with_rc, int sanitize_mode, uint64_t seed, int device,
                               uint8_t **S, size_t *S_len);
/* Lengths of the z factors in factor order (plain or reverse-complement mode, as above); *out: nolzss_free. */
int nolzss_factor_lengths(const uint8_t *text, size_t n, int with_rc, int device, uint32_t **out, size_t *z);
/* out[i] = text[pi(i)] for the keyed bijection pi of (seed, record 0) on [0, n) (any byte values; *out: nolzss_free). */
int nolzss_shuffle_dna(const uint8_t *text, size_t n, uint64_t seed, int device, uint8_t **out);

/* ---- strand-bias grid and space-scale histogram of the factors --------------------------------- */
/* reference: noLZSS.genomics.plots, _compute_strand_bias_grid (src/noLZSS/genomics/plots.py:1961-2075) and the 2-D
 * histogram of plot_space_scale_heatmap (:2559-2614).  Both read every factor and return a few thousand numbers: they
 * are binned on the device from the records the pipeline leaves there ("Strand-bias and space-scale
 * maps"), so no factor record crosses PCIe.
 *
 * Kept factors (:2149-2157): length >= min_factor_length, or a sentinel factor.  Everything below is over them.
 * Strand grid: the factor plane (x = start .. start + length, y = ref + (x - start) forward, ref + length - (x - start)
 *   reverse complement) cut into x_bins x y_bins cells over [0, x_max) x [0, y_max); x_max = y_max = total_length, or
 *   (total_length = 0) max(start + length) and max(ref + length).  forward_units / rc_units[yi * x_bins + xi] = the
 *   x-length of that strand's segments inside cell (yi, xi) in units of 1 / unit nucleotides, unit = x_bins * y_bins:
 *   every crossing of a cell edge is a multiple of 1 / unit, so the integers are exact and do not depend on the order
 *   of the adds.  Parts outside the extents are dropped.  1 <= x_bins, y_bins <= 4096; x_max, y_max <= 2^33.
 * Space-scale histogram: numpy.histogram2d(lengths, starts, bins=[length_edges, position_edges]) per strand:
 *   hist[li * n_position_bins + pi] counts edges[i] <= v < edges[i + 1], the last bin also v == edges[-1].  Edges: 2 to
 *   4097 (length) / 2 to 2^20 + 1 (position) non-decreasing finite float64.  position_edges = NULL: the reference's
 *   ladder (:2566-2574) over genome_end = the largest kept start, nb = max(position_min_bins, ceil(genome_end /
 *   position_bin_bp)), edges[k] = k * (genome_end / nb), edges[nb] = genome_end (= numpy.linspace(0, genome_end,
 *   nb + 1)); with genome_end = 0 or no kept factor there is no ladder: n_position_bins = 0 and no histogram.
 * One pipeline run serves both.  Free the result with nolzss_free_factor_maps(). */
typedef struct nolzss_factor_map_request {
    uint32_t x_bins, y_bins;       /* 0, 0: no strand grid */
    uint64_t total_length;         /* 0: extents from the kept factors */
    uint64_t min_factor_length;    /* 0 or 1: keep all */
    const double *length_edges;    /* NULL / 0: no space-scale histogram */
    size_t n_length_edges;
    const double *position_edges;  /* NULL / 0: the reference's ladder from the two fields below */
    size_t n_position_edges;
    uint32_t position_min_bins;    /* reference: 50 */
    uint64_t position_bin_bp;      /* reference: 1 000 000 */
} nolzss_factor_map_request;
typedef struct nolzss_factor_maps {
    uint64_t z, z_used;            /* factors, kept factors */
    uint64_t x_max, y_max, unit;   /* strand grid: extents used, x_bins * y_bins */
    uint32_t x_bins, y_bins;
    uint64_t *forward_units, *rc_units; /* y_bins * x_bins each (NULL without a grid request) */
    size_t n_length_bins, n_position_bins;
    uint64_t *hist_forward, *hist_rc;   /* n_length_bins * n_position_bins each (NULL without a histogram) */
    double *position_edges;             /* n_position_bins + 1, as used */
    uint64_t kept_forward, kept_rc;     /* kept factors per strand */
    uint64_t min_length, max_length, max_start; /* over the kept factors of both strands (0 if none) */
} nolzss_factor_maps;
void nolzss_free_factor_maps(nolzss_factor_maps *m);
/* The factors of nolzss_factorize (with_rc = 0) or nolzss_factorize_dna_w_rc: the refusals of nolzss_count_factors /
 * nolzss_count_factors_dna_w_rc with their status and message.  No sentinel factors. */
int nolzss_factor_maps_text(const uint8_t *text, size_t n, int with_rc, int device,
                            const nolzss_factor_map_request *request, nolzss_factor_maps *out);
/* The factors of nolzss_factorize_fasta_multiple_dna (same reader, sanitize_mode and limits); sentinel factors = the
 * factors that start at a sentinel of the prepared string. */
int nolzss_factor_maps_fasta(const char *path, int with_rc, int sanitize_mode, int device,
                             const nolzss_factor_map_request *request, nolzss_factor_maps *out);
/* Host records (a v2 factor file, a test), uploaded in chunks and binned by the same kernels; sentinel factors by
 * ascending factor index.  ref carries NOLZSS_RC_MASK. */
int nolzss_factor_maps_records(const nolzss_factor *factors, size_t z, const uint64_t *sentinel_factor_indices,
                               size_t n_sentinels, int device, const nolzss_factor_map_request *request,
                               nolzss_factor_maps *out);
/* Host only: the position ladder above (malloc'ed, *n = nb + 1 entries; nolzss_free). */
int nolzss_debug_position_edges(uint64_t genome_end, uint32_t min_bins, uint64_t bin_bp, double **edges, size_t *n);

/* ---- self dot-plot rasters from resident factors ------------------------------------------------ */
/* reference: the LZ factor plots of noLZSS.genomics.plots -- plot_multiple_seq_self_lz_factor_plot_from_file
 * (src/noLZSS/genomics/plots.py:352-900), its _simple twin (:905) and the reference/target plots (:1126, :1358).
 * Every factor is a segment from (start, ref) to (start + length, ref + length), a reverse-complement factor from
 * (start, ref + length) down to (start + length, ref); Datashader draws them with ds.max('length'), one layer per
 * strand (:559-595), a length-range slider filters them (:669-675), a hover overlay keeps the longest factor per x bin
 * (:600-666), and all of it is recomputed at every zoom or pan.  Here a handle keeps the records of one factorisation
 * in device memory (its own allocation: every other call may run between two renders) and a render turns one viewport
 * into exact integer rasters ("Self dot-plot rasters").
 *
 * Kept factors: length >= min_factor_length or a sentinel factor (:451-458), and len_lo <= length <= len_hi (len_hi =
 *   0: no upper bound; applied to sentinel factors too).
 * View: x in [x_lo, x_hi), y in [y_lo, y_hi) over nucleotide coordinates, width x height pixels; 1 <= width, height
 *   <= 4096; x_hi, y_hi <= 2^33; x_hi - x_lo >= width and y_hi - y_lo >= height (a pixel is at least one base wide).
 * Base pairs: factor (start, length, ref) matches base pair t, 0 <= t < length, at x = start + t, y = ref + t
 *   (forward) or y = ref + length - 1 - t (reverse complement).  It is in view when x and y are inside the windows;
 *   its pixel is px = floor((x - x_lo) * width / (x_hi - x_lo)), py = floor((y - y_lo) * height / (y_hi - y_lo)).
 * Rasters: uint32, [py * width + px], row 0 the lowest y.  max_*: the largest length (of the whole factor) among the
 *   kept factors of that strand with a base pair in the pixel, 0 = none.  count_* (want_counts): how many such
 *   factors, each counted once per pixel.  visible_*: kept factors with at least one base pair in view.
 * Hover table (hover_bins = B, 1 <= B <= 4096; 0: none): a visible kept factor of either strand with
 *   2 * x_lo <= 2 * start + length < 2 * x_hi falls in column floor((2 * start + length - 2 * x_lo) * B /
 *   (2 * (x_hi - x_lo))) -- the reference's midpoint binning in integers; per column the factor of the greatest
 *   length, ties to the smallest factor index: hover_start / hover_length / hover_ref[B] (ref carrying
 *   NOLZSS_RC_MASK), hover_length = 0 for an empty column.  Deviation: "visible" is "a base pair in view", where the
 *   reference tests the bounding box against the view padded by 10 % (:608-617); k_per_bin is 1, its default.
 * A source with more than 2^32 - 1 factors or a length of 2^32 or more is refused when the handle is opened. */
typedef struct nolzss_dotplot nolzss_dotplot;
typedef struct nolzss_dotplot_summary {
    uint64_t z;                       /* factors held */
    uint64_t x_max, y_max;            /* max(start + length), max(ref + length) */
    uint64_t min_length, max_length;  /* 0, 0 without factors */
    uint64_t kept_forward, kept_rc;   /* factors per strand at min_factor_length = 1 */
    int32_t device;
    const uint64_t *sentinel_starts;  /* starts of the sentinel factors, ascending and distinct (the reference,
                                       * :528-531, keeps the caller's index order); owned by the handle */
    size_t n_sentinel_starts;
} nolzss_dotplot_summary;
typedef struct nolzss_dotplot_view {
    uint64_t x_lo, x_hi, y_lo, y_hi;
    uint32_t width, height;
    uint64_t min_factor_length;       /* 0 or 1: keep all */
    uint64_t len_lo, len_hi;          /* len_hi = 0: no upper bound */
    int32_t want_counts;
    uint32_t hover_bins;              /* 0: no hover table */
} nolzss_dotplot_view;
typedef struct nolzss_dotplot_raster {
    uint32_t width, height, hover_bins;
    uint32_t *max_forward, *max_rc;       /* height * width each */
    uint32_t *count_forward, *count_rc;   /* NULL unless want_counts */
    uint64_t visible_forward, visible_rc;
    uint64_t *hover_start, *hover_length, *hover_ref; /* hover_bins each (NULL without a table) */
} nolzss_dotplot_raster;
/* The factors of nolzss_factorize (with_rc = 0) or nolzss_factorize_dna_w_rc, with the refusals of
 * nolzss_factor_maps_text; an empty text gives a valid handle with z = 0.  Close every handle. */
int nolzss_dotplot_open_text(const uint8_t *text, size_t n, int with_rc, int device, nolzss_dotplot **h);
/* The reader of nolzss_factor_maps_fasta; sentinel factors = the factors that start at a sentinel. */
int nolzss_dotplot_open_fasta(const char *path, int with_rc, int sanitize_mode, int device, nolzss_dotplot **h);
/* Host records (ref carrying NOLZSS_RC_MASK), uploaded once; sentinel factors by factor index. */
int nolzss_dotplot_open_records(const nolzss_factor *factors, size_t z, const uint64_t *sentinel_factor_indices,
                                size_t n_sentinels, int device, nolzss_dotplot **h);
int nolzss_dotplot_info(const nolzss_dotplot *h, nolzss_dotplot_summary *info);
/* Any number of renders per handle; the handle is not changed.  Free the result with the function below. */
int nolzss_dotplot_render(const nolzss_dotplot *h, const nolzss_dotplot_view *view, nolzss_dotplot_raster *out);
void nolzss_free_dotplot_raster(nolzss_dotplot_raster *out);
/* NULL is a no-op.  Renders of one handle may run from several threads, but the close must not overlap any other call
 * on that handle: it frees the records at once.  The calling thread's current device is left as it was. */
int nolzss_dotplot_close(nolzss_dotplot *h);

/* ---- relative LZ: many targets against one reference from one suffix sort ----------------------- */
/* Extension (the reference has no such mode); it sits next to the reference/target entry points
 * factorize_dna_w_reference_seq (factorizer.cpp:825-842) and factorize_dna_rc_w_ref_fasta_files
 * (fasta_processor.cpp:240-287, 362-378), which let target j copy from targets 1..j-1 and from itself.  Here every
 * target is parsed on its own against the reference block and nothing else ("Relative LZ against a
 * reference block"):
 *   Rblk = the m reference records joined by one separator each, B = |Rblk|; separators match nothing.
 *   At position p of target T: Lf = the largest L with T[p:p+L] in Rblk, Lr = the largest L with revcomp(T[p:p+L]) in
 *   Rblk (0 without with_rc).  max(Lf, Lr) = 0: a literal of length 1.  Lf >= Lr: a forward factor of length Lf whose
 *   ref is the leftmost occurrence in Rblk.  Otherwise a reverse-complement factor of length Lr whose ref is the
 *   leftmost occurrence of the reverse complement in Rblk, with NOLZSS_RC_MASK.  The next factor starts at p + length.
 * Prepared string: S = Rblk s T1 s .. Tk s [pad] rc-block s, every s a fresh sentinel (the sequence of
 * factorizer.cpp:110-125), rc-block = rc(Rm) s .. s rc(R1) at rc_block_start = E (with_rc only), pad = one more
 * sentinel when B - 1 + E would be odd; rcN = (B - 1 + E) / 2.  Without with_rc S ends behind the sentinel of Tk,
 * rc_block_start = S_len and rcN = 0.
 * Refusals: m == 0 or no reference base, more than 250 sentinels (with_rc: 2m + k + 1 > 250, else m + k > 250), S longer
 * than the 32-bit pipeline takes: NOLZSS_ERR_INVALID_ARGUMENT; "Invalid nucleotide 'x' found in sequence j" (j counts
 * the references first, then the targets): NOLZSS_ERR_RUNTIME.  Lower case is upper-cased (factorizer.cpp:86-95). */
/* Host only.  S, target_offsets (k entries: the first position of each target in S): malloc'ed, nolzss_free(). */
int nolzss_rlz_prepare(const char *const *refs, const size_t *ref_lens, size_t m, const char *const *targets,
                       const size_t *target_lens, size_t k, int with_rc, uint8_t **S, size_t *S_len,
                       uint64_t **target_offsets, size_t *block_length, size_t *rc_block_start, size_t *rcN);
typedef struct nolzss_rlz_result {
    size_t num_targets;
    uint64_t block_length;      /* B */
    uint64_t *target_offsets;   /* [num_targets] first position of each target in S */
    uint64_t *target_lengths;   /* [num_targets] */
    size_t *counts;             /* [num_targets] factors per target */
    nolzss_factor **factors;    /* [num_targets] pointers into block, or NULL without want_factors */
    nolzss_factor *block;       /* owns every record */
    /* nolzss_rlz_factorize_fasta only: NUL-terminated ids back to back */
    char *reference_ids;
    size_t reference_ids_bytes, num_references;
    char *target_ids;
    size_t target_ids_bytes;
} nolzss_rlz_result;
/* Records are in coordinates of S, like nolzss_factorize_w_reference: start is absolute, a match has ref < block_length
 * (plus NOLZSS_RC_MASK for a reverse-complement factor), a literal has ref = start.  k == 0 gives an empty result
 * without touching the device; with want_factors == 0 only the k counts leave the device. */
int nolzss_rlz_factorize(const char *const *refs, const size_t *ref_lens, size_t m, const char *const *targets,
                         const size_t *target_lens, size_t k, int with_rc, int want_factors, int device,
                         nolzss_rlz_result *out);
/* Reader, sanitize modes and error texts of nolzss_factorize_dna_rc_w_ref_fasta_files; fills the two id lists. */
int nolzss_rlz_factorize_fasta(const char *reference_fasta_path, const char *target_fasta_path, int with_rc,
                               int sanitize_mode, int want_factors, int device, nolzss_rlz_result *out);
void nolzss_free_rlz_result(nolzss_rlz_result *r);
/* The code (length in bits 0..30, bit 31 = reverse complement, 0 = literal) of every position of S below the sentinel
 * behind the last target: target_offsets[k - 1] + target_lens[k - 1] entries (nolzss_rlz_prepare), caller-allocated.
 * Only target positions are specified. */
int nolzss_debug_rlz_codes(const char *const *refs, const size_t *ref_lens, size_t m, const char *const *targets,
                           const size_t *target_lens, size_t k, int with_rc, int device, uint32_t *code);

/* ---- decoding: factors and literals back to text ------------------------------------------------ */
/* Extension (the reference has no decoder).  A factor record does not carry the symbol of a literal, so a
 * factorization is the z records plus the literal symbols in record order ("Decoding: factors and
 * literals back to text").  One contract serves every mode the library emits:
 *   Inputs: z records (start, length, ref), ref carrying NOLZSS_RC_MASK; n_literals bytes; a known prefix of
 *     prefix_len bytes (may be empty).
 *   Output: text[0 : n), n = prefix_len when z == 0, else start[z - 1] + length[z - 1]; text[0 : prefix_len) is the prefix.
 *   Tiling: start[0] == prefix_len, start[k + 1] == start[k] + length[k], length >= 1.
 *   Literal: ref == start (no mask).  It has length 1 and takes the next byte of `literals`, in record order; the
 *     number of literal records must equal n_literals.
 *   Copy: r = ref & ~NOLZSS_RC_MASK, r + length <= start (what every mode emits: sources end before the factor starts).
 *     Forward: text[start + t] = text[r + t].  Reverse complement (mask set): text[start + t] =
 *     comp(text[r + length - 1 - t]), comp = A<->T, C<->G on upper-case bytes.  A position whose chain of copies
 *     carries an odd number of complements and ends in any other byte is an error; an even number is the identity
 *     for every byte value, so plain-mode texts over all 256 values decode.
 *   Errors: every violation is NOLZSS_ERR_INVALID_ARGUMENT, the message names the first offending record index and
 *     the rule (tiling, literal length, source range, literal count, complement of a non-nucleotide); nothing is
 *     returned.  n beyond the 32-bit pipeline is refused up front.  z == 0 returns a copy of the prefix without
 *     touching a device.
 *   Per mode: nolzss_factorize, nolzss_factorize_dna_w_rc, nolzss_factorize_multiple_dna_w_rc and the concatenated
 *     FASTA forms: empty prefix (the result is S[:n], the sentinel literals come from the literal stream);
 *     nolzss_factorize_w_reference, nolzss_factorize_dna_w_reference_seq: prefix S[:start_pos]; relative LZ: prefix =
 *     the reference block, the targets laid end to end behind it (nolzss_amd.genomics.rlz.rlz_decode rebases). */
typedef struct nolzss_decode_info {
    uint64_t n, z, n_literals;
    uint64_t resolved_at_expand;   /* of the n - prefix_len decoded positions: resolved before the first jump round */
    uint64_t rounds;               /* jump launches */
    uint64_t max_active;           /* unresolved positions entering the first jump round */
} nolzss_decode_info;
/* Host only: literals[j] = text[start of the j-th literal record]; a literal record with start >= n is refused.
 * *literals: malloc'ed, nolzss_free. */
int nolzss_literal_symbols(const uint8_t *text, size_t n, const nolzss_factor *factors, size_t z,
                           uint8_t **literals, size_t *n_literals);
/* *text: malloc'ed, nolzss_free; info may be NULL. */
int nolzss_decode(const nolzss_factor *factors, size_t z, const uint8_t *literals, size_t n_literals,
                  const uint8_t *prefix, size_t prefix_len, int device, uint8_t **text, size_t *n,
                  nolzss_decode_info *info);
/* Factorize (with_rc: as nolzss_factorize_dna_w_rc, with its refusals; else as nolzss_factorize), keep the records in
 * device memory, gather the literals, decode and compare with the input, all on the device: only the numbers below
 * come back (with_rc: the comparison is with the upper-cased input, the strand the records describe).
 * first_mismatch = UINT64_MAX when there is none.  An empty text gives z = 0 and no mismatch.  If the
 * device arena cannot hold the records plus the decode state behind the factorization the call fails with
 * NOLZSS_ERR_NOMEM; there is no fallback. */
int nolzss_roundtrip(const uint8_t *text, size_t n, int with_rc, int device, size_t *z,
                     uint64_t *mismatches, uint64_t *first_mismatch, nolzss_decode_info *info);
/* The same with the text resident in device memory (`stream` as nolzss_factorize_device). */
int nolzss_roundtrip_device(const void *d_text, size_t n, int with_rc, int device, void *stream, size_t *z,
                            uint64_t *mismatches, uint64_t *first_mismatch, nolzss_decode_info *info);
/* Debug hook of the comparison kernel: host arrays up, the number of differing positions and the first one
 * (UINT64_MAX if none) back. */
int nolzss_debug_count_mismatches(const uint8_t *a, const uint8_t *b, size_t n, int device,
                                  uint64_t *count, uint64_t *first);

/* ---- factor records: the compact container ------------------------------------------------------ */
/* Extension.  A compact, canonical, byte-exact form of the records of nolzss_factorize, nolzss_factorize_dna_w_rc, the
 * multi-sequence forms and the reference + target forms (every mode whose records obey the contract of nolzss_decode
 * above), packed on the device and expanded on the device: with nolzss_factorize_packed the 24-byte records never cross
 * PCIe ("Factor records: the compact container").  It is a factor file, not a compressor: a factor of a
 * non-repetitive genome is about 18 bases long and carries a far reference, so the container comes out near the size of
 * the text at 2 bits per base, not below it; the gain is against the 24-byte records, and on repetitive collections.
 *   The format.  All integers little-endian, all arithmetic unsigned 32-bit with wrap-around unless stated otherwise.
 *     The records tile [first_start, first_start + decoded): p_0 = first_start, p_{i + 1} = p_i + L_i, so p is not
 *     stored; first_start is 0 for the plain and reverse-complement forms and start_pos for the reference + target
 *     forms.  Record i is a literal (ref == start, no mask, L = 1), a forward copy (ref = x) or a reverse-complement
 *     copy (ref = x | NOLZSS_RC_MASK); every copy has x + L <= p, the rule of nolzss_decode.  For a copy r = 1 (reverse
 *     complement) or 0, y = x (forward) or -(x + L) (the mirrored coordinate, in which a reverse-complement match reads
 *     forward), g = y - p.  With c the last copy before i (none: g_c = r_c = 0): e = g - g_c, v = (zigzag32(e) << 1) |
 *     (r ^ r_c), 33 bits, zigzag32(e) = (e << 1) ^ (int32(e) >> 31).  A copy that goes on colinearly behind any number
 *     of literals, on either strand, has v = 0.
 *   control: one nibble per record, record 2 j in the low and 2 j + 1 in the high nibble of byte j, (z + 1) / 2 bytes,
 *     the spare nibble of an odd z is 0.  nibble = a | b << 2; a: 0 a literal (b must be 0), 1 / 2 / 3: L in 1 / 2 / 4
 *     bytes; b: 0: v = 0, 1 / 2 / 3: v in 2 / 4 / 5 bytes (not the archive's 1 / 3 / 5: on one strand |e| < n, so 4
 *     bytes always suffice up to 2^30 symbols).  The packer uses the smallest class that holds the value, so the
 *     sections are a function of the records; the expander takes any well-formed code.
 *   data: per record, in order, the bytes of L, then those of v; a literal has none.
 *   literals: literal_mode 1: every literal symbol is A, C, G or T (also: there is none) and they lie four to a byte
 *     at 2 bits (A, C, G, T = 0 .. 3), the first in the low bits, unused bits 0; literal_mode 0: one byte per literal;
 *     literal_mode 2: the literals are not stored (a factor file like v2), n_literals is still the number of literal
 *     records.  The packer chooses 1 or 0, canonically; 2 is the caller's choice (store_literals == 0).
 *   The file (written and read by nolzss_amd.write_packed_factors / read_packed_factors, host only): a 72-byte header
 *     -- the magic "noLZFAC1", uint32 version = 1, uint32 flags (bits 0-1 literal_mode, the rest 0), then uint64
 *     first_start, z, n_literals, decoded, control_bytes, data_bytes, literal_bytes -- and control, data and literals,
 *     each padded with zeros to 8 bytes.  Nothing follows; sequence names and sentinel indices of the v2 footer are
 *     out of scope.
 *   nolzss_factors_pack: host records -> the three device-made sections as malloc'ed buffers (never NULL after a
 *     success); free with nolzss_free_packed_factors (NULL and an all-zero struct are no-ops; the struct is zeroed).
 *     first_start = start[0].  Whatever the format cannot carry is refused on the device before a byte is packed, in
 *     the words of nolzss_decode and naming the first offending record: tiling (start[k + 1] != start[k] + length[k],
 *     length == 0, an end beyond the 32-bit pipeline), literal length, source range (ref + length > start), and, with
 *     store_literals, a literal count other than n_literals.  Without store_literals `literals` is not read.  A data
 *     section of 2^32 bytes or more is refused before anything is written.  z == 0 is valid and launches nothing.
 *   nolzss_factorize_packed / _device: factorize as nolzss_roundtrip does (with_rc: as nolzss_factorize_dna_w_rc, with
 *     its refusals, the literals taken from the upper-cased strand), leave the records in device memory above the work
 *     arrays, gather the literals and pack there: only the three sections come down.  If the device arena cannot hold
 *     the pack behind the factorization the call fails with NOLZSS_ERR_NOMEM and names the sizes; there is no
 *     fallback.  An empty text gives z = 0.  `stream` as nolzss_factorize_device.
 *   nolzss_factors_unpack: the sections are UNTRUSTED.  The byte sizes of control and literals are first checked on
 *     the host against the counts, first_start, decoded, their sum, z and n_literals against the 32-bit pipeline, and
 *     every device read is bounded by these sizes and never by what a section says.  The rules, all checked on the
 *     device, judged in three steps of which the first that finds a violation names its smallest offending record,
 *     whatever the schedule: (1) from the nibbles alone: a literal nibble has b == 0, the spare nibble is 0, the data
 *     bytes the nibbles ask for are exactly data_bytes (compared before a data byte is read); (2) L >= 1, v has 33
 *     bits, then the exact 64-bit sum of L equals `decoded` (before a position is formed); (3) x + L <= p for a copy,
 *     in 64 bits after the 32-bit recovery, and no more literal records than n_literals.  A count that falls short
 *     names record z, "behind the last".  A violation returns NOLZSS_ERR_INVALID_ARGUMENT and nothing is returned.
 *     *factors: nolzss_free; *literals: malloc'ed, nolzss_free, NULL for literal_mode 2.
 *   nolzss_decode_packed: unpack into device memory and decode there as nolzss_decode does (its rule on complements
 *     included): the 24-byte records never cross PCIe.  literal_mode 2 and prefix_len != first_start are refused.
 *   The calling thread's current device is left as it was. */
typedef struct nolzss_packed_factors {
    uint32_t literal_mode, reserved;            /* reserved: 0 */
    uint64_t first_start, z, n_literals;
    uint64_t decoded;                           /* sum of the lengths of the records */
    uint8_t *control, *data, *literals;         /* malloc'ed by the packers; the caller's for unpack and decode_packed */
    uint64_t control_bytes, data_bytes, literal_bytes;
} nolzss_packed_factors;
int nolzss_factors_pack(const nolzss_factor *factors, size_t z, const uint8_t *literals, size_t n_literals,
                        int store_literals, int device, nolzss_packed_factors *out);
int nolzss_factorize_packed(const uint8_t *text, size_t n, int with_rc, int store_literals, int device,
                            nolzss_packed_factors *out);
int nolzss_factorize_packed_device(const void *d_text, size_t n, int with_rc, int store_literals, int device,
                                   void *stream, nolzss_packed_factors *out);
void nolzss_free_packed_factors(nolzss_packed_factors *p);
int nolzss_factors_unpack(const nolzss_packed_factors *in, int device, nolzss_factor **factors, size_t *z,
                          uint8_t **literals, size_t *n_literals);
int nolzss_decode_packed(const nolzss_packed_factors *in, const uint8_t *prefix, size_t prefix_len, int device,
                         uint8_t **text, size_t *n, nolzss_decode_info *info);

/* ---- relative-LZ archive: ranges of the targets from resident records --------------------------- */
/* Extension.  Every copy of a relative-LZ parse points into the reference block and never into a target, so any byte of
 * any target is one hop from the record that covers it.  A handle keeps the block and the records in device memory of
 * its own (every other call may run between two extracts) and an extract turns a batch of (target, lo, hi) ranges into
 * bytes with one launch: per output byte one search and one gathered byte, no state words and no jump rounds (DESIGN.md
 * 5, "Relative-LZ archive: ranges from resident records").
 *   Inputs of open_records: what nolzss_amd.genomics.rlz.absolute_records produces, the decoder's contract with
 *     prefix = block: the z records tile [block_len, n), the k targets lie end to end behind the block in order, a
 *     literal has ref == start and length 1 and takes the next byte of `literals`.
 *   Two rules beyond the decoder's.  Source inside the block: a copy has (ref & ~NOLZSS_RC_MASK) + length <= block_len
 *     (it replaces the decoder's source range rule: a self-referential factorisation, whose bytes are chains of hops
 *     of unbounded depth, is refused and not decoded slowly).  Target boundary: sum(target_lengths) == n - block_len
 *     and no record straddles the end of a target or lies behind the last one.  Empty targets, k == 0, and z == 0 with
 *     all lengths 0 are valid.
 *   Refusals at open: NOLZSS_ERR_INVALID_ARGUMENT, the message names the first offending record index and the rule
 *     (tiling, literal length, source inside the block, target boundary, literal count; lengths that do not sum name
 *     record z, "behind the last"); nothing is opened.  n beyond the 32-bit pipeline and z >= 2^32 are refused too.
 *   Ranges: bytes [lo, hi) of target `target`; they may be empty, overlap, repeat and come in any order.  Output:
 *     the ranges back to back, range i = bytes[offsets[i] : offsets[i + 1]), offsets[i + 1] - offsets[i] == hi - lo.
 *   Refusals at extract: NOLZSS_ERR_INVALID_ARGUMENT, the message names the first offending range index, nothing is
 *     written or returned: target >= k, lo > hi, hi > target_lengths[target], 2^32 or more bytes or ranges in one
 *     call, d_out_capacity < total.
 *   Complement of a non-nucleotide (a reverse-complement copy over a byte of the block that is not A, C, G or T, a
 *     separator for instance) is found by the kernel: the call fails with NOLZSS_ERR_INVALID_ARGUMENT, the message
 *     names the smallest (range index, byte) and its position inside the target, whatever the schedule; extract returns
 *     nothing, the contents of d_out are then unspecified.  The handle stays usable.
 *   Extracts of one handle may run from several threads, but a close must not overlap any other call on that handle.
 *   The calling thread's current device is left as it was. */
typedef struct nolzss_rlz_archive nolzss_rlz_archive;
typedef struct nolzss_rlz_range {
    uint64_t target, lo, hi;          /* bytes [lo, hi) of that target */
} nolzss_rlz_range;
typedef struct nolzss_rlz_archive_summary {
    uint64_t num_targets;
    uint64_t block_length;
    uint64_t z, n_literals;
    uint64_t total_length;            /* sum of the target lengths */
    const uint64_t *target_lengths;   /* num_targets entries, owned by the handle */
    int32_t device;
    uint64_t device_bytes;            /* device memory the handle holds: block, 16 bytes per record, position sample */
} nolzss_rlz_archive_summary;
int nolzss_rlz_archive_open_records(const uint8_t *block, size_t block_len, const nolzss_factor *records, size_t z,
                                    const uint8_t *literals, size_t n_literals, const uint64_t *target_lengths,
                                    size_t k, int device, nolzss_rlz_archive **h);
int nolzss_rlz_archive_info(const nolzss_rlz_archive *h, nolzss_rlz_archive_summary *info);
/* *bytes (total bytes) and *offsets (q + 1 entries): malloc'ed, nolzss_free.  q == 0, or ranges that are all empty,
 * return without touching the device. */
int nolzss_rlz_archive_extract(const nolzss_rlz_archive *h, const nolzss_rlz_range *ranges, size_t q, uint8_t **bytes,
                               uint64_t **offsets, uint64_t *total);
/* The same layout into d_out_capacity bytes of caller memory on the handle's device (`stream` as
 * nolzss_factorize_device; the call returns when the bytes are written).  Only the ranges go up and only an error
 * word comes back; *total = the bytes written.  One 16-byte store per 16 output bytes when d_out is 16-byte aligned. */
int nolzss_rlz_archive_extract_device(const nolzss_rlz_archive *h, const nolzss_rlz_range *ranges, size_t q,
                                      void *d_out, size_t d_out_capacity, void *stream, uint64_t *total);
/* NULL is a no-op. */
int nolzss_rlz_archive_close(nolzss_rlz_archive *h);

/* ---- relative-LZ index: target batches matched against a resident reference ---------------------- */
/* Extension.  Every target of a relative-LZ parse is matched against the reference block and nothing else, so the
 * suffixes of the targets never have to be sorted.  A handle keeps the index of the references in device memory of its
 * own -- the packed index text X, its suffix array, LCP array, the LCP / min / max pyramids and a prefix table -- and a
 * batch of targets is matched against it by search: no suffix sort runs in a match, and every other call may run
 * between two matches ("Relative-LZ index: targets matched against a resident reference").
 *   Index text: X = the string nolzss_rlz_prepare lays out for these references and no target: Rblk s rc(Rm) s .. s
 *     rc(R1) s with reverse complement (rc_block_start = B + 1, rcN = B, never a pad), Rblk s without.
 *   Result: record for record what nolzss_rlz_factorize returns for the same references and targets wherever that call
 *     accepts them; the semantics paragraph of its section applies unchanged.  A batch of k targets is laid out as
 *     Tcat = T1 s T2 s .. Tk s; position p of Tcat is absolute position B + 1 + p, the position it would have in S, so
 *     target_offsets, record starts and the literal rule (ref == start) are those of nolzss_rlz_factorize for any k.
 *   Refusals at open: those of nolzss_rlz_prepare with k = 0 (m == 0 or no reference base, more than 250 sentinels:
 *     2m + 1 > 250 with reverse complement, m > 250 without, X longer than the 32-bit pipeline takes:
 *     NOLZSS_ERR_INVALID_ARGUMENT; an invalid reference base: NOLZSS_ERR_RUNTIME), all before any device is touched;
 *     prefix_syms > 12: NOLZSS_ERR_INVALID_ARGUMENT.  prefix_syms = 0 picks P = clamp(floor(log4 |X|) - 1, 4, 12); 1..12
 *     force it (tests).  The prefix table has 4^P + 1 entries.
 *   Refusals of a match: a null array, or B + 1 + sum(len) + k beyond the 32-bit pipeline: NOLZSS_ERR_INVALID_ARGUMENT;
 *     "Invalid nucleotide 'x' found in sequence j" with j = m + the target's index: NOLZSS_ERR_RUNTIME.  Lower case is
 *     upper-cased.  There is no limit on k other than the length rule; k == 0 returns an empty result without touching
 *     the device; empty targets are kept, with 0 factors; with want_factors == 0 only the k counts leave the device.
 *   Several threads may match against one handle, but a close must not overlap any other call on that handle.  The
 *     calling thread's current device is left as it was. */
typedef struct nolzss_rlz_index nolzss_rlz_index;
typedef struct nolzss_rlz_index_summary {
    uint64_t num_references, block_length, index_length;  /* m, B, |X| */
    int32_t with_rc, device;
    uint32_t prefix_syms;             /* P actually used */
    uint64_t device_bytes;            /* everything the handle holds, one allocation */
} nolzss_rlz_index_summary;
int nolzss_rlz_index_open(const char *const *refs, const size_t *ref_lens, size_t m, int with_rc,
                          uint32_t prefix_syms, int device, nolzss_rlz_index **h);
/* Reader and sanitize modes of nolzss_rlz_factorize_fasta; every record of the file is a reference record. */
int nolzss_rlz_index_open_fasta(const char *reference_fasta_path, int with_rc, int sanitize_mode,
                                uint32_t prefix_syms, int device, nolzss_rlz_index **h);
int nolzss_rlz_index_info(const nolzss_rlz_index *h, nolzss_rlz_index_summary *info);
/* One batch; fills a nolzss_rlz_result exactly as nolzss_rlz_factorize does (no id lists; free it with
 * nolzss_free_rlz_result). */
int nolzss_rlz_index_factorize(const nolzss_rlz_index *h, const char *const *targets, const size_t *target_lens,
                               size_t k, int want_factors, nolzss_rlz_result *out);
/* The code (length in bits 0..30, bit 31 = reverse complement, 0 = no match) of every position of Tcat: sum(len) + k
 * entries, caller-allocated.  Only target positions are specified -- the counterpart of nolzss_debug_rlz_codes. */
int nolzss_rlz_index_codes(const nolzss_rlz_index *h, const char *const *targets, const size_t *target_lens,
                           size_t k, uint32_t *code);
/* Pattern count and locate: where a sequence occurs in the reference, and how often ("Relative-LZ index:
 * pattern count and locate").  Nothing is added to the handle; a batch of q patterns goes up as a target batch does.
 *   Patterns: nucleotide strings, case-insensitive, validated and upper-cased as targets are.
 *   Occurrences: a forward occurrence of pattern P at `position` means Rblk[position .. position + |P|) equals P and lies
 *     inside one reference record; a reverse-strand occurrence at `position` means that stretch equals rc(P), and is only
 *     reported by an index opened with reverse complement.  A pattern that is its own reverse complement is counted on
 *     both strands.  An empty pattern has count 0 and no hits; it is not an error.
 *   count: counts[j] = the occurrences of pattern j on both strands together (q entries, the caller's).
 *   locate: counts as above.  Every occurrence of a pattern with counts[j] <= max_hits is returned as (position, record,
 *     is_rc): position is the coordinate in Rblk, record the 0-based reference record.  max_hits == 0 means no cap.  A
 *     pattern with more than max_hits occurrences reports its count and NO hits, so which hits come back never depends
 *     on how tied suffixes are ordered.  Layout: hit_offsets has q + 1 entries (the caller's), pattern j owns hits
 *     [hit_offsets[j], hit_offsets[j + 1]), and inside a pattern the hits ascend by (position, is_rc), forward first;
 *     they are sorted on the device.  *hits: malloc'ed, nolzss_free; NULL when *num_hits = hit_offsets[q] is 0.
 *   Refusals before any device work: a null handle, array or output pointer: NOLZSS_ERR_INVALID_ARGUMENT; a locate of
 *     2^31 or more patterns in one batch (the sort key of a hit keeps its pattern in 31 bits):
 *     NOLZSS_ERR_INVALID_ARGUMENT; sum(len) + q beyond the 32-bit pipeline: NOLZSS_ERR_INVALID_ARGUMENT; "Invalid
 *     nucleotide 'x' found in pattern j" (j 0-based in this batch, the first such pattern): NOLZSS_ERR_RUNTIME.  The
 *     lengths alone decide the length rule and no pattern byte is read before it holds, so a batch that breaks both it
 *     and the nucleotide rule reports the length.  q == 0 succeeds without touching the device.
 *   Refusal of the total: when the hits to report number more than the 32-bit pipeline takes, the call returns
 *     NOLZSS_ERR_INVALID_ARGUMENT naming the total and pointing at max_hits; it is decided once the counts are known
 *     and before anything is expanded (counts and hit_offsets are then filled, *hits is NULL).
 *   An arena out-of-memory leaves the handle untouched, as a match does.  Several threads may query one handle; the
 *     calling thread's current device is left as it was.  NOLZSS_RLZ_LOCATE_CHUNK (tests): hit records per download. */
typedef struct nolzss_rlz_hit {
    uint64_t position;
    uint32_t record;
    uint32_t is_rc;
} nolzss_rlz_hit;
int nolzss_rlz_index_count(const nolzss_rlz_index *h, const char *const *patterns, const size_t *pattern_lens, size_t q,
                           uint64_t *counts);
int nolzss_rlz_index_locate(const nolzss_rlz_index *h, const char *const *patterns, const size_t *pattern_lens, size_t q,
                            uint64_t max_hits, uint64_t *counts, uint64_t *hit_offsets, nolzss_rlz_hit **hits,
                            size_t *num_hits);
/* Maximal repeats: what is repeated inside the reference itself, on either strand, how often and where (DESIGN.md 5,
 * "Relative-LZ index: maximal repeats").  Nothing goes up and nothing is added to the handle: the answer is read off the
 * resident suffix array, LCP array and pyramids.  Rblk, B, X, "forward occurrence at position a" and "reverse-strand
 * occurrence at position a" are those of the locate above.
 *   Occ(w), for a nucleotide string w, is the set of (a, is_rc) the locate would report for the pattern w without a cap;
 *     count(w) = |Occ(w)|.  A reverse-strand occurrence exists only on an index opened with reverse complement.
 *   Extensions of an occurrence of w, L = |w|.  Forward at a: the right extension is Rblk[a + L], or a unique end mark
 *     if the record ends there; the left extension is Rblk[a - 1], or a unique end mark if the record starts at a.
 *     Reverse strand at a: the right extension is the complement of Rblk[a - 1], the left extension the complement of
 *     Rblk[a + L], or a unique end mark each.  An end mark differs from every base and from every other end mark.
 *   Maximal repeat: count(w) >= 2, the occurrences do not all share one right extension, and they do not all share one
 *     left extension -- the strand-aware definition of DNA repeat finders.
 *   Reported: every maximal repeat w with |w| >= min_length and count(w) >= min_count, under two rules on an index with
 *     reverse complement.  (1) One of a mirror pair: Occ(rc(w)) is Occ(w) with the strands flipped, so w and rc(w) are
 *     the same repeat; with p(w) = the smallest forward position in Occ(w) (infinite without one), w is reported iff
 *     p(w) <= p(rc(w)).  Equality happens exactly when w == rc(w): such a record carries palindrome = 1.  (2) A
 *     palindrome at one locus is no repeat: a record with palindrome = 1 lists every locus on both strands and is
 *     reported only if count >= 4, i.e. at least two loci.  min_count applies to count as stated, before and
 *     independently of rule (2).
 *   Record: position = p(w) in Rblk coordinates, length = |w|, count = count(w), record = the 0-based reference record
 *     that holds position, palindrome.  The records ascend by (position, length): the key is unique and does not depend
 *     on how tied suffixes are ordered.
 *   Hits: as in the locate.  Every record with count <= max_hits (0: no cap) lists all of Occ(w) as nolzss_rlz_hit,
 *     CSR-style: record j owns hits [hit_offsets[j], hit_offsets[j + 1]), ascending by (position, is_rc), forward first;
 *     they are sorted on the device.  A record above the cap reports its count and NO hits.  repeats is NULL when
 *     num_repeats is 0, hits is NULL when num_hits is 0, hit_offsets holds its num_repeats + 1 entries after a success.
 *     Free the result with the free function below, whatever the status.
 *   repeat_count: *num_repeats = the records nolzss_rlz_index_repeats would report for the same min_length and
 *     min_count; only the flags are computed and one word comes down.  It is how a caller picks min_length.
 *   Refusals before any device work, NOLZSS_ERR_INVALID_ARGUMENT: a null handle or output pointer; min_length == 0;
 *     min_count < 2.
 *   Refusals once the counts are known and before anything is expanded, NOLZSS_ERR_INVALID_ARGUMENT: 2^31 or more
 *     records (the sort key of a hit keeps its record in 31 bits; the result is then empty); a hit total beyond the
 *     32-bit pipeline: the message names the total and points at max_hits and min_length, and the records, their counts
 *     and hit_offsets are still returned (hits is NULL and num_hits 0).
 *   An arena out-of-memory leaves the handle untouched, as a match does.  Several threads may query one handle; the
 *     calling thread's current device is left as it was.  NOLZSS_RLZ_LOCATE_CHUNK (tests): repeat records, and hit
 *     records, per download. */
typedef struct nolzss_rlz_repeat {
    uint64_t position, length, count;
    uint32_t record, palindrome;
} nolzss_rlz_repeat;
typedef struct nolzss_rlz_repeats_result {
    size_t num_repeats;
    nolzss_rlz_repeat *repeats; /* ascending by (position, length) */
    uint64_t *hit_offsets;      /* num_repeats + 1 entries */
    nolzss_rlz_hit *hits;       /* NULL when num_hits == 0 */
    size_t num_hits;
} nolzss_rlz_repeats_result;
int nolzss_rlz_index_repeat_count(const nolzss_rlz_index *h, uint64_t min_length, uint64_t min_count, uint64_t *num_repeats);
int nolzss_rlz_index_repeats(const nolzss_rlz_index *h, uint64_t min_length, uint64_t min_count, uint64_t max_hits,
                             nolzss_rlz_repeats_result *out);
/* NULL is a no-op; the result is zeroed. */
void nolzss_free_rlz_repeats_result(nolzss_rlz_repeats_result *out);
/* Host only (tests): the decision of nolzss_rlz_index_repeats once its counts are known -- NOLZSS_OK, or
 * NOLZSS_ERR_INVALID_ARGUMENT with the message of the call -- and the bit offsets of the 8-bit digits the sort of its
 * records runs for a block of block_length bases (shifts: room for 8). */
int nolzss_debug_rlz_repeats_refusal(uint64_t num_repeats, uint64_t total_hits, uint64_t max_hits, uint64_t min_length);
int nolzss_debug_rlz_repeat_shifts(uint64_t block_length, int *shifts, int *npasses);
/* Maximal match seeds: which stretches of the targets occur in the reference, maximally extended, and where (DESIGN.md
 * 5, "Relative-LZ index: maximal match seeds").  Nothing is added to the handle; the batch goes up as a match lays it
 * out, Tcat = T1 s T2 s .. Tk s, and is searched once.
 *   ms[p], for a target position p, is the length of the longest prefix of the target suffix at p that occurs inside one
 *     reference record -- on either strand when the index has the reverse complement.
 *   A seed is a super-maximal exact match of a target: an interval [start, start + length) of ONE target, length >= 1,
 *     that occurs in the reference, cannot be extended by one base to the left or to the right inside its target and
 *     still occur, and is therefore contained in no other such interval.  Occurrence is closed under taking substrings,
 *     so ms[p + 1] >= ms[p] - 1, and the seeds are exactly the positions with ms[p] >= 1 and (p is the first position of
 *     its target, or ms[p - 1] <= ms[p]), each with length ms[p].  Nothing crosses a target's end or a record's end.
 *   min_length: only seeds with length >= min_length are reported; 0 means 1.  The filter is applied after maximality is
 *     decided: a seed never becomes maximal because a longer neighbour was filtered out.
 *   Occurrences of a seed: exactly those of its bytes as the locate above defines them.  A hit is (position, record,
 *     is_rc) in Rblk coordinates; a reverse-strand hit of a seed of L bases that the mirrored block holds at a lies at
 *     2 B - a - L + 1; a hit lies inside one record; reverse-strand hits come only from an index opened with reverse
 *     complement.  count = the occurrences on both strands together, always >= 1.
 *   max_hits: as in the locate.  A seed with more occurrences than max_hits (0: no cap) reports its count and NO hits, so
 *     which hits come back never depends on how tied suffixes are ordered.
 *   Layout: the seeds ascend by (target, start); target is the 0-based index in this batch, start the position inside the
 *     target.  hit_offsets has num_seeds + 1 entries, seed j owns hits [hit_offsets[j], hit_offsets[j + 1]) (CSR), and
 *     inside a seed the hits ascend by (position, is_rc), forward first; they are sorted on the device.  seeds is NULL
 *     when num_seeds is 0, hits is NULL when num_hits is 0, hit_offsets always holds its num_seeds + 1 entries after a
 *     success.  Free the result with the free function below, whatever the status.
 *   Refusals: everything a match refuses, with the same status and message (a null array, the length rule, "Invalid
 *     nucleotide 'x' found in sequence j"); a null handle or output pointer: NOLZSS_ERR_INVALID_ARGUMENT.  Lower case is
 *     upper-cased.  k == 0, or a batch without a base, succeeds without touching the device.
 *   More than 2^31 - 1 reported seeds in one batch: NOLZSS_ERR_INVALID_ARGUMENT (the sort key of a hit keeps its seed in
 *     31 bits).  It takes a batch of more than 2^31 positions and no test reaches it.
 *   Refusal of the total: when the hits to report number more than the 32-bit pipeline takes, the call returns
 *     NOLZSS_ERR_INVALID_ARGUMENT naming the total and pointing at max_hits and min_length; it is decided once the counts
 *     are known and before anything is expanded.  The seeds, their counts and hit_offsets are still returned; hits is
 *     NULL and num_hits 0.
 *   An arena out-of-memory leaves the handle untouched, as a match does.  Several threads may query one handle; the
 *     calling thread's current device is left as it was.  NOLZSS_RLZ_LOCATE_CHUNK (tests): seed records, and hit
 *     records, per download. */
typedef struct nolzss_rlz_seed {
    uint64_t target, start, length, count;
} nolzss_rlz_seed;
typedef struct nolzss_rlz_seeds_result {
    size_t num_seeds;
    nolzss_rlz_seed *seeds;   /* ascending by (target, start) */
    uint64_t *hit_offsets;    /* num_seeds + 1 entries */
    size_t num_hits;
    nolzss_rlz_hit *hits;     /* NULL when num_hits == 0 */
} nolzss_rlz_seeds_result;
int nolzss_rlz_index_seeds(const nolzss_rlz_index *h, const char *const *targets, const size_t *target_lens, size_t k,
                           uint64_t min_length, uint64_t max_hits, nolzss_rlz_seeds_result *out);
/* NULL is a no-op; the result is zeroed. */
void nolzss_free_rlz_seeds_result(nolzss_rlz_seeds_result *r);
/* Colinear seed chains: where every target lies -- which record, which strand, which interval, how well supported
 * ("Relative-LZ index: colinear seed chains").  The call follows nolzss_rlz_index_seeds up to the sorted
 * hits, which stay on the device, and chains them there; neither seeds nor hits come down.
 *   Parameters: min_length and max_hits are exactly those of nolzss_rlz_index_seeds; a seed with more than max_hits
 *     occurrences contributes no anchor.  max_gap and bandwidth are plain bounds: there is no "0 means unlimited", a value
 *     above any coordinate difference never binds, and the device clamps both to 2^32 - 1.
 *   Anchors: every reported hit (position x, record r, is_rc) of every seed (target t, start s, length L) is an anchor
 *     with q = s and the reference coordinate y = x on the forward strand, y = 2 B - x - L + 1 on the reverse strand: the
 *     coordinate the match has in the mirrored block of the index text X.  On either strand a colinear alignment
 *     therefore runs upward in both q and y.
 *   Groups: the anchors are grouped by (target, is_rc, record) and ordered by (y, q) inside a group; that pair is unique
 *     inside a group.
 *   Recurrence: the look-back is NOLZSS_RLZ_CHAIN_LOOKBACK, a constant of the ABI because it defines the result.  For
 *     anchor i of a group the candidates are the j with 1 <= i - j <= 64 in group order, dq = q_i - q_j >= 1, dy = y_i -
 *     y_j >= 1, max(dq, dy) <= max_gap and |dq - dy| <= bandwidth.  f(i) = max(L_i, max over j of f(j) + min(L_i, dq, dy)
 *     - |dq - dy|); pred(i) is the candidate that attains the maximum if that maximum is strictly greater than L_i, of
 *     equal candidates the nearest (the largest j); otherwise i has no predecessor.  Scores are compared in 64 bits and
 *     fit 32: f(i) <= L(first) + q_i - q(first) < 2^32, since a target of 2^31 bases or more is refused.
 *   The chain of a group: its end e is the smallest index with maximal f; it is reported iff f(e) >= min_score; its
 *     anchors are e, pred(e), .., reported in ascending q.  One chain per (target, strand, record).
 *   Chain record: t_start = q of the first anchor, t_end = q + L of the last (ends ascend with starts: the seeds are
 *     super-maximal); r_start = the MIN of x and r_end = the MAX of x + L over the chain's anchors, in Rblk coordinates
 *     (y + L is not monotone along a chain whose diagonals differ); score = f(e); primary = 1 on the chain of largest
 *     score of its target, on ties the first in output order.
 *   Layout: the chains ascend by (target, is_rc, record).  anchor_offsets has num_chains + 1 entries, chain c owns the
 *     anchors [anchor_offsets[c], anchor_offsets[c + 1]) (CSR); an anchor's position is x as a hit reports it.  chains is
 *     NULL when num_chains is 0, anchors is NULL when num_anchors is 0, anchor_offsets always holds its num_chains + 1
 *     entries after a success.  num_seeds and num_seed_hits are diagnostics: the seeds reported and the hits expanded.
 *   Refusals, all before any device work: everything nolzss_rlz_index_seeds refuses, with the same status and message; a
 *     null params; more than 2^24 targets in one batch (the group sort key keeps target, group and y in 24 + 8 + 32
 *     bits); a target of 2^31 bases or more: NOLZSS_ERR_INVALID_ARGUMENT.  k == 0, or a batch without a base, succeeds
 *     without touching the device.  The refusal of the hit total applies unchanged; it leaves an empty result and the
 *     status.
 *   An arena out-of-memory leaves the handle untouched.  Several threads may query one handle; the calling thread's
 *     current device is left as it was.  NOLZSS_RLZ_LOCATE_CHUNK (tests): chain records, and anchors, per download. */
#define NOLZSS_RLZ_CHAIN_LOOKBACK 64
typedef struct nolzss_rlz_chain_params {
    uint64_t min_length, max_hits, max_gap, bandwidth, min_score;
} nolzss_rlz_chain_params;
typedef struct nolzss_rlz_chain {
    uint64_t target, t_start, t_end, r_start, r_end, score;
    uint32_t record, is_rc, num_anchors, primary;
} nolzss_rlz_chain;
typedef struct nolzss_rlz_chain_anchor {
    uint64_t t_start, position, length;
} nolzss_rlz_chain_anchor;
typedef struct nolzss_rlz_seed_chains_result {
    size_t num_chains;
    nolzss_rlz_chain *chains;         /* ascending by (target, is_rc, record); NULL when num_chains == 0 */
    uint64_t *anchor_offsets;         /* num_chains + 1 entries */
    size_t num_anchors;
    nolzss_rlz_chain_anchor *anchors; /* NULL when num_anchors == 0 */
    size_t num_seeds, num_seed_hits;
} nolzss_rlz_seed_chains_result;
int nolzss_rlz_index_seed_chains(const nolzss_rlz_index *h, const char *const *targets, const size_t *target_lens, size_t k,
                                 const nolzss_rlz_chain_params *params, nolzss_rlz_seed_chains_result *out);
/* NULL is a no-op; the result is zeroed. */
void nolzss_free_rlz_seed_chains_result(nolzss_rlz_seed_chains_result *r);
/* Base-level alignments of the seed chains: which bases match, which differ, where the insertions and deletions are
 * ("Relative-LZ index: base-level alignments").  The call follows nolzss_rlz_index_seed_chains up to its
 * chains, which stay on the device, and aligns every chain there; neither seeds, hits nor anchors come down.
 *   Parameters: min_length, max_hits, max_gap, bandwidth and min_score mean exactly what they mean in
 *     nolzss_rlz_index_seed_chains; the chains aligned are exactly the chains that call reports for them, in the same
 *     order, one alignment per chain.  band: the diagonals allowed on either side.  max_flank: the longest flank aligned.
 *   Coordinates: q inside the target and y in the index text X, as the chain stage uses them: y = x on the forward strand,
 *     y = 2 B - x - L + 1 (the mirrored block's coordinate) on the reverse strand, where the alignment reads forward too.
 *     A record r = [S_r, E_r) of the block spans [S_r, E_r) in y on the forward strand and [2 B + 1 - E_r, 2 B + 1 - S_r)
 *     on the reverse strand.  No job reads X outside its chain's record span.
 *   Anchor trim: for consecutive anchors p, i of a chain, dq = q_i - q_p >= 1, dy = y_i - y_p >= 1, ov = max(0, L_p - dq,
 *     L_p - dy); the earlier anchor keeps L'_p = L_p - ov >= 1 bases, the last anchor of a chain is not trimmed, and an
 *     anchor contributes L' columns of `=`.
 *   Gap job between p and i: the query Q = target[q_p + L'_p, q_i) of gq = dq - L'_p bases against the reference R =
 *     X[y_p + L'_p, y_i) of gy = dy - L'_p bases, delta = gy - gq.  Allowed diagonals d = j - i in [min(0, delta) - band,
 *     max(0, delta) + band], at most NOLZSS_RLZ_ALIGN_LANES of them.  D[0][0] = 0 and D[i][j] is the minimum over the
 *     predecessors that exist inside the rectangle and the band of: the diagonal D[i-1][j-1] + (Q[i-1] != R[j-1]); up,
 *     D[i-1][j] + 1, a query base, op I; left, D[i][j-1] + 1, a reference base, op D.  The job's cost is D[gq][gy].
 *     Traceback from (gq, gy): at every cell the FIRST of diagonal, up, left that attains D is taken; a diagonal step is
 *     `=` or X.  gq == 0 or gy == 0 needs no recurrence: gy times D, or gq times I.
 *   Right flank: fq = target_len - (q_e + L_e) query bases behind the last anchor e, A = the bases of the record span
 *     behind y_e + L_e.  fq == 0: nothing.  fq > max_flank: the flank is clipped.  Otherwise W = min(A, fq + band),
 *     diagonals [-band, band], the same recurrence on (fq + 1) x (W + 1) anchored at (0, 0); the end cell is free on the
 *     reference side: the j in [max(0, fq - band), min(W, fq + band)] with the least D[fq][j], ties to the least |j - fq|,
 *     then to the smaller j.  If that range is empty the flank is clipped.  Traceback by the same rule.
 *   Left flank: the same job on the reversed strings -- the query runs q_0 - 1, q_0 - 2, .., 0, X is read downward from
 *     y_0 - 1 to the start of the record span -- and the job's ops are then reversed.
 *   A clipped flank contributes no column; t_start / t_end show the clip.
 *   Alignment record, one per chain: target, record, is_rc, score and primary are the chain's.  [t_start, t_end) is the
 *     aligned part of the target, [r_start, r_end) the aligned part of the block in Rblk coordinates -- [y_begin, y_end)
 *     on the forward strand, [2 B + 1 - y_end, 2 B + 1 - y_begin) on the reverse strand.  edit_distance is the sum of the
 *     job costs, columns the number of alignment columns.
 *   Ops: CSR -- op_offsets has num_alignments + 1 entries, alignment c owns ops [op_offsets[c], op_offsets[c + 1]), and
 *     an op is (length << 4) | code with BAM's codes: I = 1 (a target base, no block base), D = 2 (a block base, no target
 *     base), `=` = 7, X = 8.  The ops ascend in q: left flank, then anchors and gaps alternating, then the right flank;
 *     adjacent ops of equal code are merged, so no two neighbours share a code.  On the reverse strand the ops still
 *     ascend in q: they consume the block from r_end DOWNWARD, complemented -- the target stretch equals the reverse
 *     complement of Rblk[r_start, r_end) edited by the ops read back to front.
 *   Refusals, all before any device work: everything nolzss_rlz_index_seed_chains refuses, with the same status and
 *     message; bandwidth + 2 band + 1 > NOLZSS_RLZ_ALIGN_LANES (a job's diagonals are the lanes of one wavefront, and the
 *     constant defines the result); a target of 2^28 bases or more (an op keeps its length in 28 bits):
 *     NOLZSS_ERR_INVALID_ARGUMENT.  k == 0, or a batch without a base, succeeds without touching the device.  The
 *     refusal of the hit total applies unchanged; DP rows, column slots or columns beyond 2^32 - 1 in one batch are
 *     refused with the same status.  Either leaves an empty result.
 *   Layout: alignments, op_offsets, ops; alignments and ops are NULL at zero counts, op_offsets always holds its
 *     num_alignments + 1 entries after a success.
 *   An arena out-of-memory leaves the handle untouched.  Several threads may query one handle; the calling thread's
 *     current device is left as it was.  NOLZSS_RLZ_LOCATE_CHUNK (tests): records, offsets and ops per download. */
#define NOLZSS_RLZ_ALIGN_LANES 64
typedef struct nolzss_rlz_align_params {
    uint64_t min_length, max_hits, max_gap, bandwidth, min_score, band, max_flank;
} nolzss_rlz_align_params;
typedef struct nolzss_rlz_alignment {
    uint64_t target, t_start, t_end, r_start, r_end, score, edit_distance, columns;
    uint32_t record, is_rc, num_ops, primary;
} nolzss_rlz_alignment;
typedef struct nolzss_rlz_align_result {
    size_t num_alignments;
    nolzss_rlz_alignment *alignments; /* in the order of the chains; NULL when num_alignments == 0 */
    uint64_t *op_offsets;             /* num_alignments + 1 entries */
    size_t num_ops;
    uint32_t *ops;                    /* (length << 4) | code; NULL when num_ops == 0 */
    size_t num_jobs, num_rows;        /* diagnostics: the jobs planned and the DP rows run */
} nolzss_rlz_align_result;
int nolzss_rlz_index_align(const nolzss_rlz_index *h, const char *const *targets, const size_t *target_lens, size_t k,
                           const nolzss_rlz_align_params *params, nolzss_rlz_align_result *out);
/* NULL is a no-op; the result is zeroed. */
void nolzss_free_rlz_align_result(nolzss_rlz_align_result *r);
/* Host only (tests): the bit offsets of the 8-bit digits the sort of a locate's hits runs for a block of block_length
 * bases and q patterns, least significant first; shifts: 8 entries, the caller's. */
int nolzss_debug_rlz_locate_shifts(uint64_t block_length, uint64_t q, int *shifts, int *npasses);
/* NULL is a no-op. */
int nolzss_rlz_index_close(nolzss_rlz_index *h);

/* ---- relative-LZ index: pileup counts and variant sites of read batches ---------------------------- */
/* Extension.  What the sample says at every position of the reference: how deep the coverage is, which base was
 * observed, on which strand, and where the sample differs ("Relative-LZ index: pileup").  A pileup lives in
 * device memory next to its index; batch after batch goes through the align path of the index and is reduced there:
 * neither alignment records nor ops come down, only the table does, when it is asked for.
 *   A pileup belongs to ONE index handle, which must outlive it, and to ONE nolzss_rlz_align_params, given at open.  It
 *     holds NOLZSS_RLZ_PILEUP_CHANNELS = 8 uint32 counters for every position p of the block Rblk, 0 <= p < B, all zero
 *     after open; the counters of a separator position stay zero.
 *       channel 0..3  A, C, G, T: the base observed, written in the block's forward orientation
 *       channel 4     DEL: deletion columns
 *       channel 5     INS: insertion ops anchored here
 *       channel 6     REV: columns of reverse-strand alignments that consume this base (`=`, X or D)
 *       channel 7     BREAK: alignment ends with a clipped target remainder
 *     Depth at p is A + C + G + T + DEL.
 *   add: the batch is aligned exactly as nolzss_rlz_index_align aligns it with the pileup's parameters: the same
 *     alignments in the same order.  With primary_only, alignments whose `primary` is 0 are skipped.  Every alignment kept
 *     is walked in forward-block orientation: on the forward strand its ops are read first to last and the target bases
 *     are taken as they are; on the reverse strand its ops are read last to first and the target bases are complemented
 *     (the rule of nolzss_rlz_index_align: the target stretch equals the reverse complement of Rblk[r_start, r_end)
 *     edited by the ops read back to front).  The walk starts at r = r_start and r only ascends:
 *       `=` of n: for each of the n positions the channel of the BLOCK's base is incremented; r += n.
 *       X of n: for each of the n positions the channel of the oriented TARGET base is incremented; r += n.
 *       D of n: DEL is incremented at each of the n positions; r += n.
 *       I of n: INS at clamp(r - 1, r_start, r_end - 1) is incremented ONCE per op, whatever n is; r stays.
 *       On the reverse strand REV is also incremented at every position that `=`, X or D consume.
 *       BREAK takes +1 at r_start if the target has bases in front of the aligned part in this orientation (forward
 *       strand: t_start > 0; reverse strand: t_end < target length) and +1 at r_end - 1 in the mirror case.
 *     Counters are exact.  To keep them below 2^32 an add is refused before any device work when the targets added so far
 *     plus k would exceed 2^31 - 1 (a target has at most one chain per strand and record, so at most two alignments over
 *     any position): NOLZSS_ERR_INVALID_ARGUMENT.  Everything nolzss_rlz_index_align refuses is refused with the same
 *     status and message: the parameters by open, the batch by add; the refusals of a total learnt on the device (hits,
 *     DP rows, column slots, columns) are decided before any counter is written.  A refused or failed add leaves the
 *     counters as they were.  k == 0, or a batch without a base, succeeds without touching the device.  *info: the
 *     alignments kept of this batch, their ops and their columns, and the targets added so far.
 *   counts: out[(p - start) * 8 + channel] for start <= p < end, (end - start) * 8 words, the caller's.  end > B or start >
 *     end: NOLZSS_ERR_INVALID_ARGUMENT.
 *   variants(min_count, num, den): for every non-separator position p with block base b one record for every allele a
 *     among the three other bases and DEL with count_a >= min_count and count_a * den >= num * depth, and one for INS
 *     under the same rule against the same depth; the products are taken in 64 bits.  allele is 0..3 for a base, 4 for
 *     DEL, 5 for INS; ref_base is b (0..3 = A, C, G, T); count the allele's counter, depth and rev the position's depth
 *     and REV; record / record_offset the reference record of p and p's place inside it.  The records ascend by
 *     (position, allele).  den == 0, num > den, min_count == 0 or den beyond 32 bits: NOLZSS_ERR_INVALID_ARGUMENT.  Free
 *     the result with the free function below, whatever the status.
 *   The inserted sequence: INS counts the ops, not their bases; the bases are kept in the insertion log and reported by
 *     nolzss_rlz_pileup_insertions, and nolzss_rlz_pileup_consensus applies them (both below).  Not reported: no genotype
 *     is called and no quality is given -- a record says that an allele passed the caller's threshold, nothing about
 *     zygosity; reads are not realigned; an indel is normalised only on request (nolzss_rlz_pileup_open_flags), never
 *     across an X or a second gap, and by at most NOLZSS_RLZ_PILEUP_MAX_SHIFT positions; an inserted allele beyond
 *     NOLZSS_RLZ_PILEUP_INS_BASES bases is reported truncated and never applied.
 *   Memory: 44 bytes of device memory per block base, one allocation of the handle's own: 36 of counters (two difference
 *     arrays -- `=` depth and REV are kept as +1 / -1 entries at the ends of a run and scanned on the first read after an
 *     add --, four X counters, DEL, INS, BREAK) and 8 of resolved depths.  An out-of-memory at open or in an add leaves
 *     the pileup (at open: none) and the index untouched.
 *   Threads: the calls on one pileup are serialised by a mutex in the handle, so several threads may add to and read one
 *     pileup; a reader sees every add that returned before it started.  The calling thread's current device is left as
 *     it was.  NOLZSS_RLZ_LOCATE_CHUNK (tests): positions of counts, and variant records, per download. */
#define NOLZSS_RLZ_PILEUP_CHANNELS 8
typedef struct nolzss_rlz_pileup nolzss_rlz_pileup;
typedef struct nolzss_rlz_pileup_add_info {
    uint64_t alignments, ops, columns; /* of this batch: the alignments kept, their ops, their columns */
    uint64_t targets;                  /* added to the pileup so far, this batch included */
} nolzss_rlz_pileup_add_info;
typedef struct nolzss_rlz_pileup_summary {
    uint64_t block_length, device_bytes;
    uint64_t targets, alignments, ops, columns, adds; /* running totals; adds: the batches that reached the device */
    int32_t device, dirty;                            /* dirty: an add since the last read */
    nolzss_rlz_align_params params;
} nolzss_rlz_pileup_summary;
typedef struct nolzss_rlz_variant {
    uint64_t position, record_offset;
    uint32_t record, ref_base, allele, count, depth, rev;
} nolzss_rlz_variant;
typedef struct nolzss_rlz_variants_result {
    size_t num_variants;
    nolzss_rlz_variant *variants; /* ascending by (position, allele); NULL when num_variants == 0 */
} nolzss_rlz_variants_result;
int nolzss_rlz_pileup_open(const nolzss_rlz_index *index, const nolzss_rlz_align_params *params, nolzss_rlz_pileup **out);
int nolzss_rlz_pileup_add(nolzss_rlz_pileup *p, const char *const *targets, const size_t *target_lens, size_t k,
                          int primary_only, nolzss_rlz_pileup_add_info *info);
int nolzss_rlz_pileup_counts(nolzss_rlz_pileup *p, uint64_t start, uint64_t end, uint32_t *out);
int nolzss_rlz_pileup_variants(nolzss_rlz_pileup *p, uint32_t min_count, uint64_t num, uint64_t den,
                               nolzss_rlz_variants_result *out);
/* NULL is a no-op; the result is zeroed. */
void nolzss_free_rlz_variants_result(nolzss_rlz_variants_result *r);
int nolzss_rlz_pileup_info(nolzss_rlz_pileup *p, nolzss_rlz_pileup_summary *info);
/* NULL is a no-op. */
int nolzss_rlz_pileup_close(nolzss_rlz_pileup *p);
/* Extension.  Left-normalised indels, the insertion alleles and a consensus ("Relative-LZ index:
 * consensus").  nolzss_rlz_pileup_open is nolzss_rlz_pileup_open_flags with flags 0; an unknown flag bit is refused with
 * NOLZSS_ERR_INVALID_ARGUMENT before any device work.
 *   NOLZSS_RLZ_PILEUP_NORMALIZE.  The aligner's traceback takes the first of diagonal, up, left, and a reverse-strand read
 *     is aligned on the mirrored block: an indel inside a repeat lands at one end of it for forward reads and at the other
 *     for reverse reads.  With the flag every indel is counted at its leftmost block position on both strands.  Stated on
 *     the walk of add: the oriented ops of a kept alignment are o_0 .. o_{m-1} (read first to last on the forward strand,
 *     last to first on the reverse strand), S is its oriented target stretch, r ascends from r_start and q from 0; op k
 *     has length n and the values r_k, q_k in front of it.  Its shift s_k is 0 unless the flag is set, o_k is D or I, k > 0
 *     and o_{k-1} is `=` of length m; then, with L = min(m, NOLZSS_RLZ_PILEUP_MAX_SHIFT),
 *       D: s_k = the largest s <= L with Rblk[r_k - j] == Rblk[r_k + n - j] for all 1 <= j <= s;
 *       I, W = S[q_k, q_k + n): s_k = the largest s <= L with Rblk[r_k - j] == W[(n - j) mod n] for all 1 <= j <= s (the
 *         mod is non-negative: each step rotates the inserted string by one).
 *     A shift reads the block and the op's own target bases only.  The counters, where they differ from add's rules:
 *       `=` op k in front of a D op: the block's base is counted at [r_k, r_k + n - s_{k+1}), possibly nowhere;
 *       D op: DEL at [r_k - s, r_k - s + n), and the block's own base at [r_k - s + n, r_k + n) -- the `=` columns that moved
 *         behind the gap;
 *       I op: INS at clamp(r_k - s - 1, r_start, r_end - 1); its allele is W' with W'[i] = W[(i - s) mod n].
 *     X, REV and BREAK are unchanged: every kept alignment still adds exactly one depth to every position of [r_start,
 *     r_end), and no separator is touched.  With flags 0 no shift is computed and the counters are what add states.
 *   The insertion log: every I op of a kept alignment appends one event of 24 bytes to a device buffer of the handle, with
 *     and without the flag: the position where INS was counted, n, and the first min(n, NOLZSS_RLZ_PILEUP_INS_BASES)
 *     bases of W' (flags 0: W' = W) as two words of big-endian 2-bit codes (A, C, G, T = 0 .. 3), zero behind them.  Two
 *     events are the same allele iff position, n and both words are equal; an allele with n > NOLZSS_RLZ_PILEUP_INS_BASES
 *     is truncated.  (An I run of nolzss_rlz_index_align crosses n + 1 of a job's at most NOLZSS_RLZ_ALIGN_LANES diagonals:
 *     it stays below 64 bases.)  The buffer grows geometrically -- a new allocation, a device copy, a free --; the events
 *     of a batch are counted on the device and their room is secured before the first counter of that add is written, so
 *     an add that is refused or runs out of memory leaves counters and log as they were.  An add that would take the log
 *     beyond 2^32 - 1 events is refused: NOLZSS_ERR_INVALID_ARGUMENT.  NOLZSS_RLZ_PILEUP_LOG_EVENTS (tests): the first
 *     capacity.  log_info: the flags, the events logged and the bytes of the log's allocation (device_bytes of
 *     nolzss_rlz_pileup_info keeps meaning the counters).
 *   insertions(min_count, num, den): the allele table -- the distinct events with their multiplicities, built on the
 *     device on the first read after an add and kept until the next add -- filtered: one record per allele with count >=
 *     min_count and count * den >= num * depth (64-bit products), depth = the position's A + C + G + T + DEL, ins_total
 *     its INS counter (the sum of the counts of all alleles there), truncated = 1 for n > NOLZSS_RLZ_PILEUP_INS_BASES;
 *     bases as in the log.  The records ascend by (position, length, bases[0], bases[1]).  Refusals: those of variants.
 *   consensus(params, want_map): for a non-separator position p with block base b, depth d and M the largest of its A, C,
 *     G, T and DEL counters: p is LOW if d < min_depth or M * den < num * d; it then emits b's letter (low == 0) or N
 *     (low == 1) and no insertion.  Otherwise the call is b if b's counter equals M, else the smallest channel that
 *     attains M; a base emits its letter, DEL emits nothing.  Then the modal insertion allele at p -- the largest count,
 *     ties to the first in table order -- is emitted behind the call (also behind a DEL call) if count * den >= num * d,
 *     unless it is truncated: then it is skipped and counted in truncated_skipped.  A separator emits one 0x01.  text:
 *     `length` bytes, the records' consensus joined by one 0x01 each, as the block is; record r is text[record_offsets[r],
 *     record_offsets[r + 1] - 1), record_offsets has num_records + 1 entries.  starts (want_map): starts[p] = the offset
 *     in text where p's output begins, block_length + 1 entries, starts[block_length] = length; else NULL.  called: the
 *     positions not low; substitutions / deleted: calls of another base / of DEL; insertions / inserted_bases: alleles
 *     emitted and their bases.  An insertion in front of an alignment's first block base is anchored by the clamp at
 *     r_start, so it is emitted one base late (a quirk of INS's anchor, kept).  Refusals, before any device work: a null
 *     pointer, min_depth == 0, low > 1, den == 0, num > den, den beyond 32 bits: NOLZSS_ERR_INVALID_ARGUMENT; a text of
 *     2^32 bytes or more is refused with the same status.  Free either result with its free function, whatever the status.
 *   NOLZSS_RLZ_LOCATE_CHUNK (tests): insertion records, text bytes, and map entries, per download. */
#define NOLZSS_RLZ_PILEUP_NORMALIZE 1u
#define NOLZSS_RLZ_PILEUP_MAX_SHIFT 1024 /* a constant of the ABI: it defines the result */
#define NOLZSS_RLZ_PILEUP_INS_BASES 64
typedef struct nolzss_rlz_insertion {
    uint64_t position, record_offset;
    uint32_t record, length, count, depth, ins_total, truncated;
    uint64_t bases[2];
} nolzss_rlz_insertion; /* 56 bytes */
typedef struct nolzss_rlz_insertions_result {
    size_t num_insertions;
    nolzss_rlz_insertion *insertions; /* NULL when num_insertions == 0 */
} nolzss_rlz_insertions_result;
typedef struct nolzss_rlz_consensus_params {
    uint32_t min_depth, low;
    uint64_t num, den;
} nolzss_rlz_consensus_params;
typedef struct nolzss_rlz_consensus_result {
    size_t length;
    char *text;
    size_t num_records;
    uint64_t *record_offsets; /* num_records + 1 */
    uint64_t *starts;         /* want_map: block_length + 1 entries, else NULL */
    uint64_t called, low_positions, substitutions, deleted, insertions, inserted_bases, truncated_skipped;
} nolzss_rlz_consensus_result;
int nolzss_rlz_pileup_open_flags(const nolzss_rlz_index *index, const nolzss_rlz_align_params *params, uint32_t flags,
                                 nolzss_rlz_pileup **out);
int nolzss_rlz_pileup_log_info(nolzss_rlz_pileup *p, uint32_t *flags, uint64_t *events, uint64_t *log_bytes);
int nolzss_rlz_pileup_insertions(nolzss_rlz_pileup *p, uint32_t min_count, uint64_t num, uint64_t den,
                                 nolzss_rlz_insertions_result *out);
/* NULL is a no-op; the result is zeroed. */
void nolzss_free_rlz_insertions_result(nolzss_rlz_insertions_result *r);
int nolzss_rlz_pileup_consensus(nolzss_rlz_pileup *p, const nolzss_rlz_consensus_params *params, int want_map,
                                nolzss_rlz_consensus_result *out);
/* NULL is a no-op; the result is zeroed. */
void nolzss_free_rlz_consensus_result(nolzss_rlz_consensus_result *r);
/* Extension.  A cohort of samples over the block of one index: the base calls of many pileups kept on the device at 3 bits
 * per base, their pairwise SNP distances and the sites that vary among them ("Relative-LZ index: cohort").
 * A cohort belongs to the index it was opened over, which must outlive it, and lives on that index's device.  Align,
 * the pileup, the consensus and their records are what they were.
 *   Planes.  With B the block length and W = ceil(B / 64), sample s is three bit planes of W 64-bit words, ok, lo and hi;
 *     bit p & 63 of word p >> 6 belongs to block position p.  ok: the sample has a base call at p; lo | hi << 1: the
 *     base's code (A, C, G, T = 0 .. 3, as the packed texts have it).  Two invariants hold, and every read-out relies on
 *     them: lo and hi are 0 wherever ok is 0, and every bit at or beyond B is 0.
 *   add_pileup(cohort, pileup, params): the pileup must be open over the same index (the pointer and the serial number
 *     the index got at its open are compared), else NOLZSS_ERR_INVALID_ARGUMENT.  params are refused in the words of
 *     nolzss_rlz_pileup_consensus; `low` is checked but plays no part.  The pileup is resolved if it is dirty, as any
 *     read of it does; its counters are not changed.  Per non-separator position with depth d and M the largest of its
 *     A, C, G, T and DEL counters: the position is LOW exactly when the consensus says so (d < min_depth or M * den <
 *     num * d, 64-bit products); else the call is the block's base if its counter equals M, else the smallest channel
 *     that attains M -- the consensus' own rule, one function in the library.  ok is set iff the position is not LOW and
 *     the call is a base: a DEL call, a LOW position and a separator are "no call".  Insertion alleles play no part:
 *     neither the log nor the allele table is read, and an inserted base has no position in the block.  *info: the
 *     sample's index and four counts -- called (the ok bits), low, deleted (DEL calls), differs (ok and the call is not
 *     the block's base).  For the same rule on the same pileup, by construction: called == consensus.called -
 *     consensus.deleted, deleted == consensus.deleted, differs == consensus.substitutions, low == consensus.low_positions.
 *   add_calls(cohort, calls, n): a sample given as one byte per block position, a consensus computed elsewhere for one;
 *     n must equal B.  A, C, G, T in either case are calls, any other byte is no call, and a separator position is no
 *     call whatever its byte says.  The counts: deleted = 0, low = the non-separator positions without a call.
 *   distances(cohort): two N x N uint32 matrices, row-major.  differences[i][j] = the positions where both samples are
 *     ok and their codes differ; compared[i][j] = the positions where both are ok.  Both are symmetric; differences[i][i]
 *     = 0 and compared[i][i] = called of sample i.  The counts are exact (each at most B < 2^32) and do not depend on
 *     how the work was split.  No sample: num_samples 0 and NULL matrices.
 *   sites(cohort, min_present, with_reference): per non-separator position, present = the samples with ok there and
 *     counts[4] = those of every base.  With with_reference the block's base counts as one more allele in the test
 *     that follows and nowhere else (not in present, not in counts).  A position is reported iff at least two distinct
 *     bases occur and present >= min_present; the records ascend by position; reference: the block's base code.
 *     min_present above N gives no record.
 *   columns(cohort, positions, S, out): out[s * S + k] = the letter of sample s at positions[k], `N` for no call (also
 *     at a separator), N x S bytes.  The positions may come in any order and repeat.  calls(cohort, sample, start, end,
 *     out): the same letters of one sample over [start, end).
 *   info: samples, capacity (samples the allocation holds), block length, device bytes.  samples(out, capacity, count):
 *     *count = N, and the infos of the first min(N, capacity) samples go to out.
 *   Refusals, each NOLZSS_ERR_INVALID_ARGUMENT and before any device work: a null pointer; a pileup of another index; n
 *     != B; a sample index or a range out of bounds; a position at or beyond B; a sample beyond
 *     NOLZSS_RLZ_COHORT_MAX_SAMPLES (a constant of the ABI: both matrices of a full cohort, 2 x N^2 cells of 4 bytes,
 *     stay below 2^32 bytes).
 *   Memory: the planes lie sample-major in ONE device allocation of the handle, 24 W bytes per sample -- 3 bits per
 *     base.  Its capacity in samples grows geometrically -- a new allocation, a device copy, a free --, and the room is
 *     secured before the first word of a new sample is written.  NOLZSS_RLZ_COHORT_SAMPLES (tests): the first capacity,
 *     read at open; else as many samples as 256 MiB hold, at least 1 and at most 64.  Matrices, flags, scans and staging
 *     buffers are arena memory.  An out-of-memory condition in any call leaves the cohort, the pileup and the index as
 *     they were.
 *   Threads: the calls on one cohort are serialised by a mutex in the handle; add_pileup takes the cohort's mutex, then
 *     the pileup's.  The calling thread's current device is left as it was.  NOLZSS_RLZ_COHORT_SLICE (tests): the words
 *     of a plane one workgroup of the pair kernel covers, read on every call; NOLZSS_RLZ_LOCATE_CHUNK (tests): matrix
 *     cells, site records and letters per download.
 *   Not done: insertions and indel alleles in the distances, DEL as a fifth state, genotypes or qualities, trees,
 *     removing a sample, save / load, more than one GPU. */
#define NOLZSS_RLZ_COHORT_MAX_SAMPLES 16384
typedef struct nolzss_rlz_cohort nolzss_rlz_cohort;
typedef struct nolzss_rlz_cohort_sample_info {
    uint64_t sample;                         /* the sample's index in the cohort */
    uint64_t called, low, deleted, differs;
} nolzss_rlz_cohort_sample_info;
typedef struct nolzss_rlz_cohort_summary {
    uint64_t samples, capacity, block_length, device_bytes;
    int32_t device, reserved;
} nolzss_rlz_cohort_summary;
typedef struct nolzss_rlz_cohort_distances_result {
    size_t num_samples;
    uint32_t *differences, *compared; /* num_samples x num_samples each, row-major; NULL when num_samples == 0 */
} nolzss_rlz_cohort_distances_result;
typedef struct nolzss_rlz_cohort_site {
    uint64_t position, record_offset;
    uint32_t record, present, counts[4], reference, reserved;
} nolzss_rlz_cohort_site; /* 48 bytes */
typedef struct nolzss_rlz_cohort_sites_result {
    size_t num_sites;
    nolzss_rlz_cohort_site *sites; /* ascending by position; NULL when num_sites == 0 */
} nolzss_rlz_cohort_sites_result;
int nolzss_rlz_cohort_open(const nolzss_rlz_index *index, nolzss_rlz_cohort **out);
int nolzss_rlz_cohort_add_pileup(nolzss_rlz_cohort *c, nolzss_rlz_pileup *p, const nolzss_rlz_consensus_params *params,
                                 nolzss_rlz_cohort_sample_info *info);
int nolzss_rlz_cohort_add_calls(nolzss_rlz_cohort *c, const char *calls, size_t n, nolzss_rlz_cohort_sample_info *info);
int nolzss_rlz_cohort_info(nolzss_rlz_cohort *c, nolzss_rlz_cohort_summary *info);
int nolzss_rlz_cohort_samples(nolzss_rlz_cohort *c, nolzss_rlz_cohort_sample_info *out, size_t capacity, size_t *count);
int nolzss_rlz_cohort_distances(nolzss_rlz_cohort *c, nolzss_rlz_cohort_distances_result *out);
/* NULL is a no-op; the result is zeroed. */
void nolzss_free_rlz_cohort_distances_result(nolzss_rlz_cohort_distances_result *r);
int nolzss_rlz_cohort_sites(nolzss_rlz_cohort *c, uint64_t min_present, int with_reference, nolzss_rlz_cohort_sites_result *out);
/* NULL is a no-op; the result is zeroed. */
void nolzss_free_rlz_cohort_sites_result(nolzss_rlz_cohort_sites_result *r);
int nolzss_rlz_cohort_columns(nolzss_rlz_cohort *c, const uint64_t *positions, size_t S, char *out);
int nolzss_rlz_cohort_calls(nolzss_rlz_cohort *c, uint64_t sample, uint64_t start, uint64_t end, char *out);
/* NULL is a no-op. */
int nolzss_rlz_cohort_close(nolzss_rlz_cohort *c);

/* ---- relative-LZ archive: batches appended from the index ---------------------------------------- */
/* Extension.  The index and the archive meet on the device: a batch is matched against the index as
 * nolzss_rlz_index_factorize matches it, and its records go from the match kernels straight into the archive's resident
 * form -- no record crosses PCIe, and an archive grows batch by batch without a limit on the number of targets (DESIGN.md
 * 5, "Relative-LZ archive: batches appended from the index").
 *   open_index: an empty archive (z = 0, no targets) over the reference block of `ix`, on the index's device and bound
 *     to that index.  The block is Rblk, the reference records upper-cased and joined by one 0x01 each -- byte for byte
 *     the block of nolzss_amd.genomics.rlz.absolute_records --, unpacked on the device from the packed index text into
 *     an allocation of the archive's own.  Every index handle carries a serial number, a process-wide counter taken at
 *     its open; the archive remembers it.  The archive may outlive the index; only an append needs it.
 *   append_index: the k targets become targets num_targets .. num_targets + k - 1 of the archive, in order.  With the
 *     batch laid out as Tcat = T1 s .. Tk s, the record of factor start i at batch position p, with j separators below
 *     p, becomes resident record z_old + i - j with start = decoded_old + p - j; a separator's own literal is dropped,
 *     so a batch adds exactly (factor starts of the batch) - k records.  The position sample is extended over the new
 *     positions.  When the record or sample array is too small it is replaced by one of max(needed, 2 x current)
 *     entries, the old contents copied device to device; device_bytes counts capacity.
 *   All or nothing: the handle changes only after the device work of the call has finished without error.  Any refusal
 *     or failure, an arena or device out-of-memory included, leaves the archive exactly as it was and usable.
 *   Refusals of append: NOLZSS_ERR_INVALID_ARGUMENT before any device work for a null handle or index, an archive not
 *     opened by open_index, an index whose serial number or device is not the one the archive is bound to;
 *     NOLZSS_ERR_INVALID_ARGUMENT naming the quantity for decoded_old + sum(len) beyond the 32-bit pipeline (decided
 *     by the lengths alone) and for z reaching 2^32; and everything nolzss_rlz_index_factorize refuses, with its status
 *     and message ("sequence j" is m + the target's index in this batch).  k == 0 succeeds without touching the device.
 *   export: the host form of ANY archive, exactly what nolzss_rlz_archive_open_records takes: the block, z records with
 *     absolute start = block_len + decoded start, ref carrying NOLZSS_RC_MASK or equal to start for a literal, and the
 *     literal symbols in record order.  Each of the three comes down once; malloc'ed, nolzss_free.
 *   An append must not overlap any other call on that archive; the index may serve other threads' matches meanwhile.
 *   The calling thread's current device is left as it was. */
typedef struct nolzss_rlz_archive_append_info {
    uint64_t targets_added, records_added, literals_added, bases_added;
    uint64_t num_targets, z, total_length;  /* of the archive after the call */
    uint64_t capacity_records;              /* records the handle's allocation can hold */
    uint64_t device_bytes;                  /* as in the summary: what the handle holds now */
    int32_t reallocated;                    /* 1 if the record or sample array moved in this call */
} nolzss_rlz_archive_append_info;
int nolzss_rlz_archive_open_index(const nolzss_rlz_index *ix, nolzss_rlz_archive **h);
/* info may be NULL. */
int nolzss_rlz_archive_append_index(nolzss_rlz_archive *h, const nolzss_rlz_index *ix, const char *const *targets,
                                    const size_t *target_lens, size_t k, nolzss_rlz_archive_append_info *info);
int nolzss_rlz_archive_export(const nolzss_rlz_archive *h, uint8_t **block, size_t *block_len, nolzss_factor **records,
                              size_t *z, uint8_t **literals, size_t *n_literals);

/* ---- relative-LZ archive: the compact container --------------------------------------------------- */
/* Extension.  A compact, canonical, byte-exact form of an archive, packed on the device from the resident records and
 * expanded on the device into them: only the compact streams cross PCIe and the file system, the 24-byte records of
 * export / open_records do not appear ("Relative-LZ archive: the compact container").
 *   The format.  All integers little-endian, all arithmetic unsigned 32-bit with wrap-around.  Record i, in archive
 *     order, has a decoded start p (relative to the end of the block), a length L >= 1, a kind (literal, forward copy,
 *     reverse-complement copy) and, a copy, the forward-strand source start x with x + L <= B, B = block_length.  For a
 *     copy r = 1 (reverse complement) or 0, y = x (forward) or 2 B + 1 - x - L (the mirrored coordinate, in which a
 *     reverse-complement match reads forward), g = y - p.  With c the last copy before i in the whole archive (none:
 *     g_c = r_c = 0): e = int32(g - g_c), s = r ^ r_c, v = (zigzag32(e) << 1) | s, 33 bits, zigzag32(e) = (e << 1) ^
 *     (e >> 31).  A copy that continues colinearly behind any number of literals, on either strand, has v = 0.
 *   control: one nibble per record, record 2 j in the low and 2 j + 1 in the high nibble of byte j, (z + 1) / 2 bytes,
 *     the spare nibble of an odd z is 0.  nibble = a | b << 2; a: 0 a literal (L = 1, b = 0), 1 / 2 / 3: L in 1 / 2 / 4
 *     bytes; b: 0: v = 0, 1 / 2 / 3: v in 1 / 3 / 5 bytes.  The packer uses the smallest code that holds the value, so
 *     the sections are a function of the archive; open_packed takes any well-formed code.
 *   data: per record, in order, the bytes of L, then those of v; a literal has none.
 *   literals: the symbols of the literal records in order; literal_mode 1: every one is A, C, G or T (also: there is
 *     none) and they lie four to a byte at 2 bits (A, C, G, T = 0 .. 3), the first in the low bits, unused bits 0;
 *     literal_mode 0: one byte each.
 *   block: block_mode 1: every byte is A, C, G, T or 0x01 (always so over an index): (B + 3) / 4 bytes of bases at 2
 *     bits as above, 0x01 stored as base 0, then num_separators ascending 32-bit positions of the 0x01 bytes (at no
 *     particular alignment); block_mode 0: the B bytes raw, num_separators = 0.
 *   The file (written and read by nolzss_amd.genomics.rlz.write_packed_archive / read_packed_archive, host only): a
 *     112-byte header -- the magic "noLZRLZ1", uint32 version = 1, uint32 flags (bit 0 block_mode, bit 1 literal_mode,
 *     bit 2 has_ids, the rest 0), then uint64 B, k, z, n_literals, decoded, num_separators and the byte sizes of the
 *     six sections -- and the sections, each padded with zeros to 8 bytes: target lengths (k uint64), ids (k + 1 uint64
 *     offsets and the UTF-8 bytes; empty without ids), block, control, data, literals.  Nothing follows.
 *   pack: any archive handle -> the four device-made sections as malloc'ed buffers, the modes and the counts; free
 *     with nolzss_free_rlz_archive_packed (NULL and an all-zero struct are no-ops; the struct is zeroed).  z == 0 (and
 *     k == 0) is valid and launches no kernel.  A data section of 2^32 bytes or more is refused with
 *     NOLZSS_ERR_INVALID_ARGUMENT before anything is written.  The handle is not changed; a pack may run beside
 *     extracts of the same handle, not beside an append or a close.
 *   open_packed: the sections are UNTRUSTED.  The byte size of every section is first checked on the host against the
 *     counts (block, control, literals; NOLZSS_ERR_INVALID_ARGUMENT naming the section), and every device read is
 *     bounded by these sizes and never by what a section says.  The rules, all checked on the device: the spare nibble
 *     is 0; a literal nibble has b == 0; the data bytes the nibbles ask for are exactly data_bytes (compared before a
 *     data byte is read); L >= 1; v has 33 bits; x + L <= B for a copy, which covers a recovered y outside its strand's
 *     range; no record straddles the end of a target or lies behind the last one; the literal records are n_literals;
 *     sum L == decoded == sum(target_lengths); the separator list ascends and stays below B.  B, decoded, their sum,
 *     z and k beyond the 32-bit pipeline are refused as nolzss_rlz_archive_open_records refuses them.  A violation
 *     returns NOLZSS_ERR_INVALID_ARGUMENT; the message names the smallest offending record index and the rule, whatever
 *     the schedule (a count that falls short names record z, "behind the last"; the separator list is judged first and
 *     names the smallest offending list index).  Nothing is opened then, and an arena or device out-of-memory leaves
 *     nothing open either.
 *   The handle of open_packed behaves exactly as one of nolzss_rlz_archive_open_records: info, extract, extract_device,
 *     export, pack and close serve it, append_index and finder_open refuse it as they refuse every archive not opened
 *     over an index; device_bytes counts the block, 16 bytes per record and the position sample.
 *   The calling thread's current device is left as it was. */
typedef struct nolzss_rlz_archive_packed {
    uint32_t block_mode, literal_mode;
    uint64_t block_length;                      /* B */
    uint64_t z, n_literals;
    uint64_t decoded;                           /* sum of the lengths of the records = sum of the target lengths */
    uint64_t num_separators;                    /* entries of the separator list of a block of mode 1 */
    uint8_t *block, *control, *data, *literals; /* malloc'ed by pack (never NULL after a success); the caller's for open_packed */
    uint64_t block_bytes, control_bytes, data_bytes, literal_bytes;
} nolzss_rlz_archive_packed;
int nolzss_rlz_archive_pack(const nolzss_rlz_archive *h, nolzss_rlz_archive_packed *out);
void nolzss_free_rlz_archive_packed(nolzss_rlz_archive_packed *p);
int nolzss_rlz_archive_open_packed(const nolzss_rlz_archive_packed *in, const uint64_t *target_lengths, size_t k, int device,
                                   nolzss_rlz_archive **h);

/* ---- relative-LZ archive: locate patterns inside the targets, through the parse ------------------- */
/* Extension.  In which targets of an archive, and where, does a pattern occur?  Answered on the device without decoding
 * the targets ("Relative-LZ archive: locate through the parse"; a hybrid index after Ferrada, Gagie,
 * Hirvola and Puglisi 2014).
 *   Occurrences: pattern P of m bases, 1 <= m <= M, occurs in target t at `position` when target_t[position .. position +
 *     m) equals P (is_rc = 0) or, with an index opened with reverse complement, rc(P) (is_rc = 1).  An occurrence lies
 *     inside one target.  A pattern that is its own reverse complement is reported on both strands, forward first; an
 *     index without reverse complement reports no is_rc hits; an empty pattern has count 0.
 *   primary: the records tile the decoded targets.  An occurrence that lies inside ONE copy record is secondary
 *     (primary = 0); one that crosses a record start or lies in a literal record is primary (primary = 1).
 *   open: `archive` must have been opened by nolzss_rlz_archive_open_index over `index`.  M = max_pattern_length, 1 ..
 *     4096, is fixed here; prefix_syms (0: chosen, else 1 .. 12) is the key length of the prefix table of the index over
 *     the kernel text.  The finder is a SNAPSHOT of the archive: it holds, in device memory of its own, the records
 *     ordered by their source interval in the block with a max pyramid over the interval ends, the kernel text K -- the
 *     bytes within max(M - 1, 1) positions of every record start, clipped to the record's target, overlapping or
 *     touching windows merged, back to back -- with its interval tables, and an index over K built as
 *     nolzss_rlz_index_open builds one, with the strand setting of `index`.  Archive and index must outlive the finder.
 *     An archive without records gives a valid finder whose every count is 0; its queries do no device work.
 *   Refusals of open, before any device work, NOLZSS_ERR_INVALID_ARGUMENT: a null pointer; an archive not opened by
 *     open_index; an index whose serial number or device is not the one the archive is bound to; M outside 1 .. 4096;
 *     prefix_syms > 12; a kernel text whose index text could exceed the 32-bit pipeline -- decided by the bound
 *     min(total_length, 2 max(M - 1, 1) z) on |K|, the message names z, M and that length.
 *   count / locate: a batch of q patterns, packed and validated exactly as for nolzss_rlz_index_locate, with its
 *     statuses and messages (a null handle, array or output pointer; 2^31 or more patterns in a locate; the length rule
 *     before "Invalid nucleotide 'x' found in pattern j", NOLZSS_ERR_RUNTIME).  Further refusals before any device work,
 *     NOLZSS_ERR_INVALID_ARGUMENT: a pattern longer than M (the first such pattern and M are named); an archive that has
 *     grown since the open (z or the number of targets differ: open a new finder).  counts[j] = the occurrences of
 *     pattern j on both strands, exact in 64 bits.  locate: every occurrence of a pattern with counts[j] <= max_hits (0:
 *     no cap) comes back as (target, position inside the target, is_rc, primary); a pattern above the cap reports its
 *     count and NO hits.  Layout as in nolzss_rlz_index_locate: hit_offsets has q + 1 entries, inside a pattern the hits
 *     ascend by (target, position, is_rc); *hits is malloc'ed (nolzss_free), NULL when *num_hits = hit_offsets[q] is 0.
 *   Refusals of the totals, NOLZSS_ERR_INVALID_ARGUMENT once the counts are known: more occurrences of the batch in the
 *     block or in K than the 32-bit pipeline takes (decided before anything is expanded; the counts are not known
 *     then), or more hits to report (counts and hit_offsets are then filled, *hits is NULL).
 *   An arena out-of-memory leaves finder, archive and index untouched.  Several threads may query one finder; a close,
 *     or an append to the archive, must not overlap a query.  The calling thread's current device is left as it was.
 *     NOLZSS_RLZ_LOCATE_CHUNK (tests): hit records per download.
 *   kernel (test hook): K and its interval tables as malloc'ed host arrays (nolzss_free): interval i holds the decoded
 *     positions [dstart[i], dstart[i] + kstart[i + 1] - kstart[i]) at K[kstart[i] ..); intervals + 1 entries each,
 *     kstart[intervals] = |K|, dstart[intervals] = total_length.  A finder without records returns empty K and one entry. */
typedef struct nolzss_rlz_finder nolzss_rlz_finder;
typedef struct nolzss_rlz_finder_summary {
    uint64_t num_targets, z, total_length;  /* of the archive when the finder was opened */
    uint64_t max_pattern_length;            /* M */
    uint64_t kernel_length, intervals;      /* |K| and the number of its intervals */
    int32_t with_rc;
    int32_t device;
    uint64_t device_bytes;                  /* what the finder itself holds */
} nolzss_rlz_finder_summary;
typedef struct nolzss_rlz_target_hit {
    uint64_t target;
    uint64_t position;
    uint32_t is_rc;
    uint32_t primary;
} nolzss_rlz_target_hit;
int nolzss_rlz_finder_open(const nolzss_rlz_archive *archive, const nolzss_rlz_index *index, uint64_t max_pattern_length,
                           uint32_t prefix_syms, nolzss_rlz_finder **h);
int nolzss_rlz_finder_info(const nolzss_rlz_finder *h, nolzss_rlz_finder_summary *info);
int nolzss_rlz_finder_count(const nolzss_rlz_finder *h, const char *const *patterns, const size_t *pattern_lens, size_t q,
                            uint64_t *counts);
int nolzss_rlz_finder_locate(const nolzss_rlz_finder *h, const char *const *patterns, const size_t *pattern_lens,
                             size_t q, uint64_t max_hits, uint64_t *counts, uint64_t *hit_offsets,
                             nolzss_rlz_target_hit **hits, size_t *num_hits);
int nolzss_rlz_finder_kernel(const nolzss_rlz_finder *h, uint8_t **kernel, size_t *kernel_len, uint64_t **kstart,
                             uint64_t **dstart, size_t *intervals);
/* NULL is a no-op; the calling thread's current device is left as it was. */
int nolzss_rlz_finder_close(nolzss_rlz_finder *h);

/* ---- measurement hooks -------------------------------------------------------------------- */
/* HIP-event timing of every pipeline stage on the context's stream (off by default). */
int nolzss_profile_enable(int device, int on);
int nolzss_profile_reset(int device);
/* Writes lines "name count total_ms algorithmic_bytes\n" into buf (NUL-terminated, truncated
 * to cap).  Nested scopes are reported separately (a stage and the kernels inside it). */
int nolzss_profile_report(int device, char *buf, size_t cap);

/* ---- introspection used by the parity tests of the intermediate arrays -------------------- */
/* Any output pointer may be NULL.  sa/isa/lstar: n entries; lcp: n + 1 entries. */
int nolzss_debug_arrays(const uint8_t *text, size_t n, int device, uint32_t *sa, uint32_t *isa,
                        uint32_t *lcp, uint32_t *lstar);
/* The factor record (start, length, ref) of EVERY position of the text in plain mode -- what nolzss_factorize would
 * emit for a factor starting there (a literal has ref = start): n records in out. */
int nolzss_debug_position_factors(const uint8_t *text, size_t n, int device, nolzss_factor *out);
/* The reverse-complement pipeline over a prepared string S (nolzss_prepare_multiple_dna_w_rc; same guards as
 * nolzss_factorize_multiple_dna_w_rc), N = S_len / 2 - 1.  Any output pointer may be NULL.  sa: S_len entries; lcp:
 * S_len + 1; isa, code, plain, records: N.  code = factor length of the position in bits 0..30, bit 31 set for a
 * reverse-complement factor, 0 for a literal.  want_plain != 0 runs the form that also computes the plain-mode length
 * of every position (0 = literal) as a by-product, as nolzss_count_factors_batch_both does.  records: the factor a
 * cursor at each position would emit.  counters (5 entries): ranks finished from global memory, ranks queued for the
 * exact forward search by the tile kernel, the same after the far ranks, compact tile output used (0 / 1), tile kernel
 * relaunched after an undecided LCP entry (0 / 1). */
int nolzss_debug_rc_arrays(const uint8_t *S, size_t S_len, int device, int want_plain, uint32_t *sa, uint32_t *isa,
                           uint32_t *lcp, uint32_t *code, uint32_t *plain, nolzss_factor *records,
                           uint32_t *counters);
/* Sorts n (key, value) pairs in place on the device by all 64 key bits (stable). */
int nolzss_debug_sort_pairs(uint64_t *keys, uint32_t *vals, size_t n, int device);
/* mode 0: exclusive add-scan, mode 1: inclusive max-scan, in place. */
int nolzss_debug_scan(uint32_t *data, size_t n, int mode, int device);
/* The 16-ary min (is_max: max) pyramid over base[0 .. len) and its three queries, run by the device functions of
 * pyramid.hpp with kMax = is_max.  The base array is uploaded into arena memory with 16 spare entries behind it; those,
 * the rest of its allocation and the arena span of the upper levels are filled with the byte `poison` (0x00 or 0xFF)
 * before anything is built, so that what a query or a build reads beyond a level's length is known and adverse.
 *   mode 0: build_pyramid; with flag_min != 0 (min pyramid, len >= 2: level 1 sets it) *flag = 1 if some base entry is >= flag_min, else 0.
 *   mode 1 (len >= 2): alloc_pyramid, level1[0 .. first_entry) uploaded into level 1 as the caller's own work,
 *     fill_pyramid_tail(first_entry) for the rest of level 1, fill_pyramid from level 2; first_entry <= len of level 1.
 *   queries: nq triples (op, a, b); results: one u32 each.  NOLZSS_PYR_NEAREST_LEFT (r, x), r < len: the largest
 *     q <= r with base[q] < x (max: > x), 0xffffffff if none.  NOLZSS_PYR_NEAREST_RIGHT (r, x), any r: the smallest
 *     q >= r, len if none.  NOLZSS_PYR_RANGE (a, b), a <= b < len: min (max) of base[a .. b].
 *   Out: *nlev, level_lens[0 .. *nlev) (room for 9), the levels back to back from level 0 in `levels` (NULL: not
 *     wanted; levels_cap entries, at least the sum of the level lengths), *flag (may be NULL when flag_min == 0).
 * NOLZSS_ERR_INVALID_ARGUMENT before any device work for null pointers, len == 0, len >= 2^32, a query outside the
 * ranges above, an unknown op, mode or poison. */
enum { NOLZSS_PYR_NEAREST_LEFT = 0, NOLZSS_PYR_NEAREST_RIGHT = 1, NOLZSS_PYR_RANGE = 2 };
int nolzss_debug_pyramid(const uint32_t *base, size_t len, int is_max, int mode, const uint32_t *level1,
                         size_t first_entry, uint32_t flag_min, int poison, const uint32_t *queries, size_t nq,
                         int device, int *nlev, uint32_t *level_lens, uint32_t *levels, size_t levels_cap,
                         uint32_t *flag, uint32_t *results);
/* The searches of nearest.hpp over sa[0 .. n) and lcp[0 .. n] (lcp[0] == lcp[n] == 0 is required), on the min and max
 * pyramids over sa and the min pyramid over lcp from build_pyramid, padding poisoned as above.  sa need not be a
 * permutation nor lcp a true LCP array.  queries: nq quintuples (op, r, a, b, c), r < n; results: two u32 each.
 *   NEAR_UP / NEAR_DOWN / FAR_UP / FAR_DOWN, _LESS or _GREATER (the latter on the max pyramid): (r, x, floor) -> (len, pos)
 *   LCP_INTERVAL (r, d), d >= 1 -> (lo, hi);  LPNF_LEFTMOST (r, d), d >= 1 -> (min SA[I(d)], 0)
 *   LPNF_SEARCH (r, i, lo, cap), i < n -> (the length, 0); meaningful where P(lo) holds or lo == 0, on a true SA / LCP */
enum {
    NOLZSS_NEAR_UP_LESS = 0, NOLZSS_NEAR_UP_GREATER = 1, NOLZSS_NEAR_DOWN_LESS = 2, NOLZSS_NEAR_DOWN_GREATER = 3,
    NOLZSS_NEAR_FAR_UP_LESS = 4, NOLZSS_NEAR_FAR_UP_GREATER = 5, NOLZSS_NEAR_FAR_DOWN_LESS = 6,
    NOLZSS_NEAR_FAR_DOWN_GREATER = 7, NOLZSS_NEAR_LCP_INTERVAL = 8, NOLZSS_NEAR_LPNF_LEFTMOST = 9,
    NOLZSS_NEAR_LPNF_SEARCH = 10
};
int nolzss_debug_nearest(const uint32_t *sa, const uint32_t *lcp, size_t n, int poison, const uint32_t *queries,
                         size_t nq, int device, uint32_t *results);
/* The LDS tile searches of nearest_lds.hpp over sa[0 .. n) (distinct values) and lcp[0 .. n] (lcp[0] == lcp[n] == 0 is
 * required; neither need come from a text), padding poisoned as above: stage_tile -> build_block_tables ->
 * lds_search_wave_blocks, one workgroup per 1024 ranks.
 *   form NOLZSS_LDS_PLAIN: the template arguments of the plain candidate kernel -- two searches per rank (0: smaller
 *     suffix start towards smaller ranks, 1: towards larger ranks); strand is ignored.
 *   form NOLZSS_LDS_RC: those of the reverse-complement kernel -- only ranks with sa[r] < strand search, four searches
 *     (0, 1 as above; 2, 3: suffix start greater than 2 * strand - sa[r], towards smaller / larger ranks), work lists of
 *     128 entries (a search that finds its list full: NOLZSS_LDS_OVERFLOW).  The other ranks return 0 / no position.
 *   len: searches * n words, len[k * n + r] for search k of rank r: the length (0: nothing), or with bit 31 set "left the
 *     reach" with the bound in bits 0..30, or NOLZSS_LDS_OVERFLOW.  pos: 2 * n words for searches 0 and 1, the suffix
 *     start of the match or 0xffffffff.
 * NOLZSS_ERR_INVALID_ARGUMENT before any device work for null pointers, n == 0, n > 2^31 - 2048, an unknown form or
 * poison, lcp[0] or lcp[n] != 0. */
enum { NOLZSS_LDS_PLAIN = 0, NOLZSS_LDS_RC = 1 };
#define NOLZSS_LDS_OVERFLOW 0xffffffffu
int nolzss_debug_lds_search(const uint32_t *sa, const uint32_t *lcp, size_t n, int form, uint32_t strand, int poison,
                            int device, uint32_t *len, uint32_t *pos);
/* The LDS sub-bucket sort (local_sort_kernel and the host function around it, local_sort_sub_buckets) on the caller's
 * pairs: n pairs (stored word, value) that lie in nb buckets [starts[k], starts[k + 1]) (nb + 1 starts, from 0 up to n).
 * Runs what the key sorts run behind their most-significant-digit pass: the bucketed view of the starts, one segmented
 * pass by the digit at bit 24 (256 sub-buckets per bucket), then every sub-bucket by npass digits from shift0 up --
 * in LDS where it fits a workgroup (18 432 pairs), by segmented passes otherwise.  The forms of the product:
 *   16-base key: shift0 8, npass 2;  35-bit key: key35, shift0 5, npass 2 (digits of 10 and 9 bits);  records: shift0 0,
 *   npass 3, any nb.  The bits below shift0 take no part in the order; the sort is stable.
 * want_regroup (the two key layouts; nb * 256 a multiple of 1024; tags at most 16 / 17): the form with the regroup of
 * round 0 on the way is asked for, whatever n is.  Where it completes (NOLZSS_LOCAL_SORT_FUSED in *status) the sorted
 * WORDS ARE NOT WRITTEN -- words_out is left alone -- and lcp[n] (0xffffffff: not a group head), new_slot / new_grp
 * (room for n; *survivors entries: the tied elements in slot order, each with the slot of its group's head) are filled;
 * otherwise the plain kernel has run and only words_out / values_out are.
 * *status: NOLZSS_LOCAL_SORT_FUSED | NOLZSS_LOCAL_SORT_LOOKBACK_GAVE_UP (the fused form ran and fell back) |
 * NOLZSS_LOCAL_SORT_LANE_ORDER (a lane-order check of the kernel failed: everything was redone by segmented passes) |
 * (sub-buckets sent to the list of those beyond a workgroup << NOLZSS_LOCAL_SORT_LISTED_SHIFT).  A failed lane-order
 * check is reported here only: the process-wide switch it throws is put back, later calls run what they would have run.
 * NOLZSS_ERR_INVALID_ARGUMENT before any device work for null pointers, n == 0, n >= 2^31, nb == 0 or > 65535, starts
 * that do not ascend from 0 to n, npass outside 2 .. 3, digits that reach beyond bit 24, key35 with another shift0 or
 * npass, want_regroup with another form or with nb * 256 not a multiple of 1024. */
enum { NOLZSS_LOCAL_SORT_FUSED = 1, NOLZSS_LOCAL_SORT_LOOKBACK_GAVE_UP = 2, NOLZSS_LOCAL_SORT_LANE_ORDER = 4,
       NOLZSS_LOCAL_SORT_LISTED_SHIFT = 8 };
int nolzss_debug_local_sort(const uint32_t *words, const uint32_t *values, size_t n, const uint32_t *starts, size_t nb,
                            int shift0, int npass, int key35, int want_regroup, int device, uint32_t *words_out,
                            uint32_t *values_out, uint32_t *lcp, uint32_t *new_slot, uint32_t *new_grp, uint32_t *survivors,
                            uint32_t *status);
/* The permutation into text order (text_order.hpp: bucketed_scatter, permute_packed) on the caller's pairs.  idx[count] and
 * val[count] (NOLZSS_TEXT_ORDER_PERMUTE_PACKED: packed[count], 64-bit words, instead of val) are uploaded; out, out2 and
 * the 16-bit array are filled with `fill` (its low half for the 16-bit array) before the call, so that what no pair names
 * is known afterwards.  flags: KEEP_INPUT, KEEP_VAL, SHORT_CODES as the arguments of bucketed_scatter; OUT2: the second
 * target (rank + 1) is wanted; NARROW (with OUT2): the codes leave as uint16_t saturated at code_max, with a wide-code
 * list of list_cap entries; PERMUTE_PACKED: permute_packed(idx, packed) instead.  rec_ends (optional): n_recs ascending
 * record ends, the last = count = n_out, handed to record_scatter_plan (report word 9: a plan was made and passed on;
 * refused, the call runs without one).
 * Out: out[n_out], out2[n_out] (may be NULL unless OUT2 / PERMUTE_PACKED), narrow[n_out] and list_items[min(listed,
 * list_cap)] (NARROW), idx_after[count] / val_after[count]: the buffers idx[0] / val[0] as the call left them (not with
 * PERMUTE_PACKED), report[NOLZSS_TEXT_ORDER_REPORT_WORDS]: 0 the form that ran (NOLZSS_TEXT_ORDER_FORM_*), 1 the packed
 * form was tried, 2 the codes it escaped, 3 its exception list overflowed, 4 a look-back gave up, 5 index bits of n_out,
 * 6 window bits, 7 partition passes in front of the plain scatter, 8 the boolean result, 9 plan made, 10 entries
 * appended to the wide-code list (may exceed list_cap).
 * NOLZSS_ERR_INVALID_ARGUMENT before any device work for null pointers, n_out == 0 or >= 2^32, count >= 2^32, an unknown
 * flag, NARROW without OUT2 or with code_max outside 1 .. 0xffff, record ends that do not ascend to count = n_out, and
 * for an idx that is not a permutation of [0, count) where the form relies on one: PERMUTE_PACKED, record ends, or
 * count == n_out > 2^22.  Elsewhere idx must not name a target below n_out twice (the result would depend on a race;
 * nothing is stored out of bounds).  A separator suffix that is not the first of its record: NOLZSS_ERR_DEVICE with
 * bucketed_scatter's message. */
enum { NOLZSS_TEXT_ORDER_KEEP_INPUT = 1, NOLZSS_TEXT_ORDER_KEEP_VAL = 2, NOLZSS_TEXT_ORDER_SHORT_CODES = 4,
       NOLZSS_TEXT_ORDER_OUT2 = 8, NOLZSS_TEXT_ORDER_NARROW = 16, NOLZSS_TEXT_ORDER_PERMUTE_PACKED = 32 };
enum { NOLZSS_TEXT_ORDER_FORM_NONE = 0, NOLZSS_TEXT_ORDER_FORM_PLAIN = 1, NOLZSS_TEXT_ORDER_FORM_PARTIAL_THEN_PLAIN = 2,
       NOLZSS_TEXT_ORDER_FORM_WINDOW_PERM = 3, NOLZSS_TEXT_ORDER_FORM_TWO_VALUE_HIST = 4, NOLZSS_TEXT_ORDER_FORM_PACKED = 5,
       NOLZSS_TEXT_ORDER_FORM_RECORD_PLAN = 6, NOLZSS_TEXT_ORDER_FORM_RECORD_PLAN2 = 7,
       NOLZSS_TEXT_ORDER_FORM_PERMUTE_PLAIN = 8, NOLZSS_TEXT_ORDER_FORM_PERMUTE_WINDOWS = 9 };
#define NOLZSS_TEXT_ORDER_REPORT_WORDS 12
int nolzss_debug_text_order(const uint32_t *idx, const uint32_t *val, const uint64_t *packed, size_t count, size_t n_out,
                            uint32_t flags, uint32_t fill, size_t list_cap, uint32_t code_max, const uint32_t *rec_ends,
                            size_t n_recs, int device, uint32_t *out, uint32_t *out2, uint16_t *narrow, uint64_t *list_items,
                            uint32_t *idx_after, uint32_t *val_after, uint32_t *report);
/* The rounds of one group-sort pass of the suffix-array construction (group_sort.hpp: group_dir_kernel and the tiled,
 * 128-, 256- and 1024-member forms of group_sort_kernel, as window rounds or as pivot rounds) on the caller's groups,
 * without the regroup behind them -- the launch function of the construction itself (group_sort_rounds).
 * text[n] is packed as every text is (pack_text: 2, 4 or 8 bits per symbol by its alphabet; nucleotides plus at most 250
 * byte values that occur once are packed segmented, the once-only bytes becoming terminators).  sa[n]: only the slots of
 * the listed groups are read and written.  slot[m] / grp[m]: the active list, in ascending slot order, grp = the head slot
 * of the entry's group; the members of a group hold consecutive list positions and the slots grp .. grp + size - 1, and
 * every listed group has at least two members.  h0: the symbols the members of every group agree on, in front of their
 * terminators (NOT CHECKED: the caller's business; nothing is read out of bounds if it does not hold).  pivot: pivot rounds,
 * depth_cap symbols deep at the most; else window rounds (depth_cap is not read).  max_rounds <= 24.  lcp_mark (optional,
 * n entries): the equalising round's filter, only groups with lcp_mark[grp + 1] == 0xffffffff are taken.
 * Out: sa, out_lo[m] (strictly smaller members of the entry's group), lcp_list[m] (0 at the head of a taken group, the
 * LCP of a boundary that appeared, else 0xffffffff), *min_depth (symbols every class that stays tied agrees on at least;
 * 0xffffffff: nothing reported), info (optional, 3 words): bits per symbol, entries of the terminator table, segmented.
 * NOLZSS_ERR_INVALID_ARGUMENT before any device work for null pointers, n == 0, m > n, max_rounds > 24, a list entry
 * with grp > slot or slot >= n, a listed slot whose sa entry is >= n, slots that do not ascend, a group that does not hold
 * consecutive list positions and the slots from its head slot on, a listed group of one member; behind the packing and
 * in front of the rounds for more than 65536 terminators. */
int nolzss_debug_group_sort(const uint8_t *text, size_t n, uint32_t *sa, const uint32_t *slot, const uint32_t *grp, size_t m,
                            uint32_t h0, int pivot, uint32_t max_rounds, uint32_t depth_cap, const uint32_t *lcp_mark,
                            int device, uint32_t *out_lo, uint32_t *lcp_list, uint32_t *min_depth, uint32_t *info);
/* The first direct round of the suffix-array construction (sa_direct.hip: group_refine_kernel and the compaction of what it
 * leaves tied) on the caller's groups -- the launch function of the construction itself (direct_round_launch), which holds
 * the only launch site of the kernel.
 * text[n], sa[n], slot[m] / grp[m]: as for nolzss_debug_group_sort, but a group may have ANY number of members >= 2 (more
 * than 64: the round leaves it as it is).  h0: the symbols the members of every group agree on, in front of their
 * terminators; cap: the depth at which the round gives up (the construction: h0 + NOLZSS_REFINE_WORDS words, 4 by default).
 * Checked of h0: every listed suffix has h0 symbols in the text (sa[slot] + h0 <= n).  NOT CHECKED, the caller's business:
 * that the members agree on them and that no terminator lies among them.  If that does not hold the results mean nothing
 * (the distance to the terminator minus the depth wraps around), but nothing is written outside the slots of the listed
 * groups and the outputs, and nothing is read out of bounds: a member then fetches windows that start up to cap - h0
 * symbols behind the end of the text, and the hook keeps 32 + 5 words of its own behind the packed text for them (the
 * straggler rounds do not fetch behind the end at all).
 * flags: NO_STRAGGLERS (the A/B switch NOLZSS_NO_STRAGGLERS), TIMED (the instantiation with the phase clocks, as under
 * NOLZSS_REFINE_PHASES: one line on stderr, the same results), WITH_RANKS (rank_by_slot is handed to the kernel; else it
 * gets none, as when the construction defers the ranks).  lcp_in[n]: what lcp holds before the call; fill: what
 * rank_by_slot holds before the call -- so every entry the round must not touch is known afterwards.
 * Out: sa[n]; lcp[n] (the LCP of every boundary that appeared, 0xfffffffe at a boundary inside a compared class that stays
 * tied, the head entry of every group as it was); rank_by_slot[n] (head slot of the member's class + 1 for every listed
 * member); new_slot / new_grp (room for m) and *new_m: the members still tied, in slot order, with the head slot of their
 * class; min_depth[3]: [0] the least depth of the compared classes left tied, [1] h0 if a group was not touched (both
 * 0xffffffff: none), [2] the members of untouched groups as every 64th workgroup counted them -- the raw counter, not
 * multiplied by 64; info (optional, 3 words): bits per symbol, entries of the terminator table, segmented.
 * NOLZSS_ERR_INVALID_ARGUMENT before any device work for null pointers, n == 0, m > n, an unknown flag, cap <= h0,
 * cap - h0 > 1024, a list entry with grp > slot or slot >= n, a listed slot whose sa entry + h0 is > n, slots that do not
 * ascend, a group that does not hold consecutive list positions and the slots from its head slot on, a listed group of
 * one member; behind the packing and in front of the round for cap - h0 beyond 32 words of the width the text has (512
 * symbols at 4 bits, 256 at 8).  (The hook also repeats the guard of suffix_array.hip against more than 65536
 * terminators; pack_text makes at most 251 table entries of a text handed in this way, so no call can meet it.) */
enum { NOLZSS_DIRECT_ROUND_NO_STRAGGLERS = 1, NOLZSS_DIRECT_ROUND_TIMED = 2, NOLZSS_DIRECT_ROUND_WITH_RANKS = 4 };
int nolzss_debug_direct_round(const uint8_t *text, size_t n, uint32_t *sa, const uint32_t *slot, const uint32_t *grp, size_t m,
                              uint32_t h0, uint32_t cap, uint32_t flags, const uint32_t *lcp_in, uint32_t fill, int device,
                              uint32_t *lcp, uint32_t *rank_by_slot, uint32_t *new_slot, uint32_t *new_grp, uint32_t *new_m,
                              uint32_t *min_depth, uint32_t *info);
/* The two arithmetic passes of the suffix-array construction over repetitive texts (sa_repeats.hip: the pair-run pass and
 * the periodic pass, with the regroup behind the latter) and the counts in front of them, on the caller's partial state --
 * periodic_pass and pair_run_pass of the construction themselves, behind the driver's own set-up (set_up_late_rounds:
 * work arrays of n entries, count_large_groups, the LCP pyramid, the radix shifts; the pair-run arrays are forced on,
 * whatever NOLZSS_PAIR_RUNS_MIN says).
 * text[n]: packed as every text is (pack_text; bytes only: no mirrored text, no merged batch).  The state as it stands
 * behind write_all_ranks: sa[n]; lcp[n + 1], a decided value (< 0xffffffbf) at the first slot of every group and a pending
 * code (>= 0xffffffbf: 0xffffffff, or 0xfffffffe inside a class the direct round compared) at every other slot of it;
 * rank[n] by position, head slot of the suffix's group + 1; slot[m] / grp[m]: the active list as for
 * nolzss_debug_group_sort, EXACTLY the slots of the groups of two and more members.  lcp[n] goes to the device as the
 * caller gives it: the driver has memory there that nothing has written yet (it clears the entry when the construction is
 * over), and no range minimum of the passes reaches it.  h: the symbols every group agrees on.  NOT CHECKED, the caller's
 * business: that the state is a true partial order of the text (each group a range of the true suffix array whose members
 * agree on h symbols, every decided LCP the true one).
 * which: NOLZSS_REPEAT_PASS_COUNTS (arg 0), _PERIODIC (arg = per_attempts on entry, 0 .. 3: 0 the first call with its
 * gate, 1 a later call, 3 "never again"), _PAIR_RUNS (arg = passes, 1 .. 10; they stop when nothing is tied any more --
 * the NOLZSS_PAIR_RUNS_* knobs play no part).  NOLZSS_NO_PERIODIC is honoured as the construction honours it.
 * Out: sa, lcp (n + 1), rank over all entries; new_slot / new_grp (room for m) and *new_m: the next active list;
 * counts[4]: what count_large_groups returns for the limit 16 (members beyond the first 16 of their group, groups of more
 * than 16, groups, members next to a member of their group at most 4096 symbols away; zero for m == 0); info (optional,
 * 3 words): bits per symbol, entries of the terminator table, segmented; periodic[3]: the return value of periodic_pass
 * (0 for the other two), per_hint and per_attempts afterwards.
 * NOLZSS_ERR_INVALID_ARGUMENT before any device work for null pointers, n == 0, n >= 2^31, m > n, another `which`, an
 * `arg` outside its range, a list entry with grp > slot or slot >= n, slots that do not ascend, a group that does not hold
 * consecutive list positions and the slots from its head slot on, a listed group of one member, an sa that is no
 * permutation, a pending lcp[0], a rank that is not the head slot (by lcp) + 1, a slot inside a group (by lcp) that is not
 * listed, a listed group without a decided entry at its head or with a decided entry inside it. */
enum { NOLZSS_REPEAT_PASS_COUNTS = 0, NOLZSS_REPEAT_PASS_PERIODIC = 1, NOLZSS_REPEAT_PASS_PAIR_RUNS = 2 };
int nolzss_debug_repeat_pass(const uint8_t *text, size_t n, uint32_t *sa, uint32_t *lcp, uint32_t *rank, const uint32_t *slot,
                             const uint32_t *grp, size_t m, uint32_t h, int which, int arg, int device, uint32_t *new_slot,
                             uint32_t *new_grp, uint32_t *new_m, uint32_t *counts, uint32_t *info, uint32_t *periodic);
/* The greedy cursor (chain.hip: mark_chain, chain_starts, chain_lengths) and the widening of 16-bit codes (lpnf.hip:
 * widened_lstar) on the caller's codes -- the production functions, which read the codes and nothing else.  codes[n]: one
 * u32 per position, length in bits 0..30 (0 = literal), bit 31 the strand.  The cursor runs p -> p + max(1, length) from
 * start_pos (start_pos >= n: *z = 0, nothing is launched; n == 0 returns at once).
 *   width 32: the codes as they are.
 *   width 16, list_max == 0: the codes narrowed into a uint16_t array allocated and padded as the pipeline's own (n + 8
 *     entries), the padding filled with the half-word `poison`; every code must be below 0xffff.  The cursor kernels read
 *     two bytes per position.  lengths / hist asked of this form: NOLZSS_ERR_DEVICE (the length kernels read 32-bit codes).
 *   width 16, list_max 1 .. 0xffff: the narrow array as above (codes <= list_max) and list[list_len], entries
 *     (position | code << 32), of which the first `listed` are applied by widened_lstar: of two entries for one position
 *     the larger counts, an entry with position >= n is ignored.  The widened array (widened[n], optional) is what the
 *     cursor then runs on, as 32-bit codes.
 * with_strand: hist holds 2 x 2048 bins, those of the codes with bit 31 behind the others (else 2048 bins; bit 31 is
 * masked out of the length either way).  bounds (optional): 2k ascending u32, counts[j] = starts inside [bounds[2j],
 * bounds[2j + 1]) (rlz_count_per_target over the emitted starts).
 * Out, each but z optional: *z, starts[z] (room for n), lengths[z] in factor order (room for n: max(1, code & 0x7fffffff)
 * of every start), hist (bin strand * 2048 + L for L < 2048) with tail[*tail_count] (room for n / 2048 + 1: L | strand <<
 * 32 for L >= 2048, in no particular order), widened[n], counts[k].  For z == 0 hist, *tail_count and counts are zero.
 * NOLZSS_ERR_INVALID_ARGUMENT before any device work for null pointers, another width, n > 2^32 - 2^19 - 1, a poison
 * above 0xffff, a 16-bit code >= 0xffff (with a list: > list_max), hist without tail and tail_count, bounds that do not
 * ascend, listed > list_len, a list or `widened` without list_max, list_max with width 32 or above 0xffff. */
int nolzss_debug_chain(const uint32_t *codes, size_t n, size_t start_pos, int width, uint32_t poison, const uint64_t *list,
                       size_t list_len, size_t listed, uint32_t list_max, int with_strand, const uint32_t *bounds, size_t k,
                       int device, uint32_t *z, uint32_t *starts, uint32_t *lengths, uint32_t *hist, uint64_t *tail,
                       uint32_t *tail_count, uint32_t *widened, uint32_t *counts);
/* What the last run of the cursor (mark_chain) on the device's context did: info[0] = 0 nothing ran (start_pos >= n),
 * 1 the speculative walk delivered the mark, 2 it raised its flag and the exact stages ran behind it, 3 the exact stages
 * alone (NOLZSS_NO_SPEC_CURSOR); info[1] = the tiles whose walk from the entry did not meet the speculative walk (with
 * NOLZSS_TEST_SPEC_CURSOR_FAILS one more). */
int nolzss_debug_cursor(int device, uint32_t *info);
/* The seed-chain stages from the group heads to the chain records (rlz_seed_chain.hip: rlz_seed_chain_run, the
 * production function) on the caller's anchors, by the rules of nolzss_rlz_index_seed_chains.  target, group, y, q,
 * length: n entries each, already ordered by (target, group, y, q); group = is_rc * m + record, and x is derived from y
 * with B and m (x = y below group m, else 2 B - y - length + 1).  Of params, max_gap, bandwidth and min_score are read.
 * Every device array is followed by padding filled with 0xff bytes.
 * Out: f[n] and pred[n] per anchor, group-local (pred 0xffffffff: none); *res as the query returns it (num_seeds and
 * num_seed_hits are 0), freed with nolzss_free_rlz_seed_chains_result.  n == 0 succeeds without a launch.
 * NOLZSS_ERR_INVALID_ARGUMENT before any launch for null pointers, n >= 2^31, m == 0 or m > 128, a target >= 2^24, a
 * group >= 2 m, length == 0, q + length >= 2^31, a reverse-strand anchor with y + length > 2 B + 1, entries out of order,
 * or a (y, q) pair that occurs twice in a group. */
int nolzss_debug_rlz_seed_chain(const uint32_t *target, const uint32_t *group, const uint32_t *y, const uint32_t *q,
                                const uint32_t *length, size_t n, const nolzss_rlz_chain_params *params, uint64_t B,
                                uint32_t m, int device, uint32_t *f, uint32_t *pred, nolzss_rlz_seed_chains_result *res);
/* The alignment stages from the job offsets to the traceback (rlz_align.hip: rlz_align_sizes, rlz_align_layout,
 * rlz_align_dp, rlz_align_traceback, the production functions) on the caller's jobs, by the rules of
 * nolzss_rlz_index_align.  query / reference: plain ACGT bytes (case-insensitive), packed as a target batch is.
 * Job j of n: kind[j] 0 = gap, 1 = right flank, 2 = left flank; a gap reads nq[j] query bases from q0[j] and ny[j]
 * reference bases from y0[j]; a right flank reads nq[j] = fq query bases from q0[j] with ny[j] = A reference bases
 * available from y0[j]; a left flank reads fq query bases downward from q0[j] - 1 with A reference bases available below
 * y0[j].  max_flank does not apply.  The job array is followed by 64 entries filled with 0xff bytes.
 * Out: cost[n], end_col[n] (a gap: ny; a flank: the end cell's j; a clipped flank: 0 with cost 0 and no column),
 * col_offsets[n + 1] and *cols: one code byte (1, 2, 7, 8) per alignment column of every job, in ascending q, malloc'ed
 * (nolzss_free; NULL without a column).  n == 0 succeeds without a launch.
 * NOLZSS_ERR_INVALID_ARGUMENT before any launch for null pointers, n >= 2^24, an invalid base, a kind above 2, a job
 * that leaves either text, 2 band + 1 > 64, or a gap with |ny - nq| + 2 band + 1 > 64. */
int nolzss_debug_rlz_align_jobs(const char *query, size_t query_len, const char *reference, size_t reference_len,
                                const uint32_t *kind, const uint32_t *q0, const uint32_t *nq, const uint32_t *y0,
                                const uint32_t *ny, size_t n, uint32_t band, int device, uint32_t *cost, uint32_t *end_col,
                                uint64_t *col_offsets, uint8_t **cols);
/* The pileup stages (rlz_pileup.hip: rlz_pileup_accumulate, rlz_pileup_resolve, rlz_pileup_compose, the production
 * functions) on the caller's alignments, by the rules of nolzss_rlz_pileup_add.  block: B bytes, ACGT (case-insensitive)
 * and any other byte for a separator between two records; targets: k plain ACGT strings, packed as a batch is; the
 * alignment records, op_offsets (num_alignments + 1 entries) and ops as nolzss_rlz_index_align returns them.
 * Out: counts[B x 8], the caller's.  No alignment, or B == 0, succeeds without a launch (the counts are zeroed).
 * NOLZSS_ERR_INVALID_ARGUMENT before any launch for null pointers, B or the batch beyond 2^28 positions, an invalid target
 * base, offsets that do not start at 0, ascend and end at num_ops, an alignment without ops, an op of length 0 or a code
 * other than 1, 2, 7, 8, a target index >= k, an alignment whose ops do not consume exactly [t_start, t_end) and
 * [r_start, r_end), whose stretches are empty on the block side, leave the target or the block, or cover a separator. */
int nolzss_debug_rlz_pileup(const char *block, size_t B, const char *const *targets, const size_t *target_lens, size_t k,
                            const nolzss_rlz_alignment *alignments, const uint64_t *op_offsets, size_t num_alignments,
                            const uint32_t *ops, size_t num_ops, int primary_only, int device, uint32_t *counts);
/* The same with the insertion log, the allele table and the consensus (the log holds one slot per op, so no
 * event is counted first; rlz_pileup_accumulate under `flags`, rlz_pileup_resolve, rlz_pileup_compose, rlz_pileup_alleles and the read-outs of
 * nolzss_rlz_pileup_insertions and nolzss_rlz_pileup_consensus, the production functions) on the caller's alignments.
 * Out: counts[B x 8]; *insertions: the whole allele table (min_count 1, fraction 0 / 1); *consensus: under *params, with
 * its map; a record is the stretch between two separator bytes of the block.  It refuses everything
 * nolzss_debug_rlz_pileup refuses, and an unknown flag bit, null results and the parameters nolzss_rlz_pileup_consensus
 * refuses.  B == 0 succeeds without a launch; no alignment gives the consensus of empty counters.  Free both results with
 * their free functions, whatever the status. */
int nolzss_debug_rlz_pileup_consensus(const char *block, size_t B, const char *const *targets, const size_t *target_lens, size_t k,
                                      const nolzss_rlz_alignment *alignments, const uint64_t *op_offsets, size_t num_alignments,
                                      const uint32_t *ops, size_t num_ops, int primary_only, uint32_t flags,
                                      const nolzss_rlz_consensus_params *params, int device, uint32_t *counts,
                                      nolzss_rlz_insertions_result *insertions, nolzss_rlz_consensus_result *consensus);
/* Capacity and high-water mark (bytes) of the device arena of `device` (lane 0). */
int nolzss_debug_arena(int device, size_t *capacity, size_t *peak);
/* The device allocations the resident handles of this process hold at the moment (index, archive, finder, pileup,
 * cohort, dotplot): their number and the bytes asked for.  Reads two counters and touches no device. */
int nolzss_debug_device_buffers(size_t *buffers, size_t *bytes);
/* The FASTA reader behind the nolzss_*fasta* entry points (host only, no device needed): records and
 * ids as NUL-terminated strings back to back; sanitize_mode 0 = remove ambiguous, 1 = strict.
 * reference: parse_fasta_sequences_and_ids, fasta_processor.cpp:28-128.  Free both with nolzss_free(). */
int nolzss_debug_parse_fasta(const char *path, int sanitize_mode, char **ids, size_t *ids_bytes,
                             char **sequences, size_t *sequences_bytes, size_t *count);
/* The reader behind nolzss_read_nucleotide_fasta alone (host only): the records after the nucleotide
 * check, or the error the reference's Python reader raises.  reference: genomics/fasta.py:28-76, 110-115. */
int nolzss_debug_parse_nucleotide_fasta(const char *path, char **ids, size_t *ids_bytes, char **sequences,
                                        size_t *sequences_bytes, size_t *count);
/* The shard plan of nolzss_read_nucleotide_fasta: owners[j] = shard of a record of lens[j] bases. */
int nolzss_debug_lpt_plan(const size_t *lens, size_t m, size_t bins, size_t *owners);
/* The static plan of nolzss_factorize_batch / _dna_w_rc for m records on n_dev devices, without touching a device
 * (host logic only): chunk_of[j] = index of the merged run record j shares (-1: none), device_of[j] = slot in the device
 * list of the pipeline run record j takes on its own (-1: none; both -1: an empty record).  The merged runs are taken by
 * n_dev x 2 lanes from ONE work queue (lane w on device w % n_dev), the single records are dealt to the devices
 * longest-processing-time first.  n_chunks (optional) = number of merged runs. */
int nolzss_debug_batch_plan(const size_t *lens, size_t m, size_t n_dev, int with_rc, int32_t *chunk_of, int32_t *device_of,
                            size_t *n_chunks);
/* Gives the device arenas that no call is using back to the driver (they are otherwise kept between
 * calls and only grow; the library does this by itself when a reservation fails). */
int nolzss_debug_trim_arenas(int device, size_t *released_bytes);
/* Records factorized since the library was loaded by merged runs / one pipeline run each. */
void nolzss_debug_batch_counters(uint64_t *merged_records, uint64_t *single_records);

#ifdef __cplusplus
}
#endif
#endif /* NOLZSS_HIP_H */
