"""Loader for libnolzss_hip.so, the gfx950 library behind this package.

There is deliberately no fallback: if the shared library is missing or cannot be loaded the
import fails loudly, and if no MI355X is visible every compute call raises (the library
returns NOLZSS_ERR_DEVICE).  Nothing in this package computes factors on the CPU.
"""
import ctypes as C
import os
from pathlib import Path

_PKG = Path(__file__).resolve().parent
# NOLZSS_LIB: another build of the same library (A/B measurements of compile-time variants, tools/ab_variant.sh)
LIB_PATH = Path(os.environ["NOLZSS_LIB"]).resolve() if os.environ.get("NOLZSS_LIB") else _PKG / "libnolzss_hip.so"

OK, ERR_INVALID_ARGUMENT, ERR_RUNTIME, ERR_NOMEM, ERR_DEVICE, ERR_IO, ERR_UNSUPPORTED = range(7)


class FastaResult(C.Structure):
    """Mirror of nolzss_fasta_result (include/nolzss_hip.h)."""
    _fields_ = [("factors", C.c_void_p), ("num_factors", C.c_size_t),
                ("sentinel_factor_indices", C.c_void_p), ("num_sentinels", C.c_size_t),
                ("sequence_ids", C.c_void_p), ("sequence_ids_bytes", C.c_size_t),
                ("num_sequences", C.c_size_t)]


class FastaPerSequenceResult(C.Structure):
    """Mirror of nolzss_fasta_per_sequence_result (include/nolzss_hip.h)."""
    _fields_ = [("factors", C.POINTER(C.c_void_p)), ("counts", C.POINTER(C.c_size_t)),
                ("sequence_ids", C.c_void_p), ("sequence_ids_bytes", C.c_size_t), ("num_sequences", C.c_size_t)]


class NucleotideFasta(C.Structure):
    """Mirror of nolzss_nucleotide_fasta (include/nolzss_hip.h)."""
    _fields_ = [("sequence_ids", C.c_void_p), ("sequence_ids_bytes", C.c_size_t), ("num_sequences", C.c_size_t),
                ("lengths", C.POINTER(C.c_size_t)), ("counts", C.POINTER(C.c_size_t)),
                ("owners", C.POINTER(C.c_size_t)), ("factors", C.POINTER(C.c_void_p)), ("keep", C.c_void_p)]


class LengthHist(C.Structure):
    """Mirror of nolzss_length_hist (include/nolzss_hip.h)."""
    _fields_ = [("threshold", C.c_uint32), ("fwd", C.POINTER(C.c_uint64)), ("rc", C.POINTER(C.c_uint64)),
                ("tail_lengths", C.POINTER(C.c_uint64)), ("tail_rc", C.POINTER(C.c_uint8)), ("tail_count", C.c_size_t),
                ("z", C.c_size_t), ("lengths", C.POINTER(C.c_uint32)), ("lengths_count", C.c_size_t)]


class FactorMapRequest(C.Structure):
    """Mirror of nolzss_factor_map_request (include/nolzss_hip.h)."""
    _fields_ = [("x_bins", C.c_uint32), ("y_bins", C.c_uint32), ("total_length", C.c_uint64),
                ("min_factor_length", C.c_uint64), ("length_edges", C.POINTER(C.c_double)),
                ("n_length_edges", C.c_size_t), ("position_edges", C.POINTER(C.c_double)),
                ("n_position_edges", C.c_size_t), ("position_min_bins", C.c_uint32), ("position_bin_bp", C.c_uint64)]


class FactorMaps(C.Structure):
    """Mirror of nolzss_factor_maps (include/nolzss_hip.h)."""
    _fields_ = [("z", C.c_uint64), ("z_used", C.c_uint64), ("x_max", C.c_uint64), ("y_max", C.c_uint64),
                ("unit", C.c_uint64), ("x_bins", C.c_uint32), ("y_bins", C.c_uint32),
                ("forward_units", C.POINTER(C.c_uint64)), ("rc_units", C.POINTER(C.c_uint64)),
                ("n_length_bins", C.c_size_t), ("n_position_bins", C.c_size_t),
                ("hist_forward", C.POINTER(C.c_uint64)), ("hist_rc", C.POINTER(C.c_uint64)),
                ("position_edges", C.POINTER(C.c_double)), ("kept_forward", C.c_uint64), ("kept_rc", C.c_uint64),
                ("min_length", C.c_uint64), ("max_length", C.c_uint64), ("max_start", C.c_uint64)]


class DotPlotSummary(C.Structure):
    """Mirror of nolzss_dotplot_summary (include/nolzss_hip.h)."""
    _fields_ = [("z", C.c_uint64), ("x_max", C.c_uint64), ("y_max", C.c_uint64), ("min_length", C.c_uint64),
                ("max_length", C.c_uint64), ("kept_forward", C.c_uint64), ("kept_rc", C.c_uint64),
                ("device", C.c_int32), ("sentinel_starts", C.POINTER(C.c_uint64)), ("n_sentinel_starts", C.c_size_t)]


class DotPlotView(C.Structure):
    """Mirror of nolzss_dotplot_view (include/nolzss_hip.h)."""
    _fields_ = [("x_lo", C.c_uint64), ("x_hi", C.c_uint64), ("y_lo", C.c_uint64), ("y_hi", C.c_uint64),
                ("width", C.c_uint32), ("height", C.c_uint32), ("min_factor_length", C.c_uint64),
                ("len_lo", C.c_uint64), ("len_hi", C.c_uint64), ("want_counts", C.c_int32),
                ("hover_bins", C.c_uint32)]


class DotPlotRaster(C.Structure):
    """Mirror of nolzss_dotplot_raster (include/nolzss_hip.h)."""
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("hover_bins", C.c_uint32),
                ("max_forward", C.POINTER(C.c_uint32)), ("max_rc", C.POINTER(C.c_uint32)),
                ("count_forward", C.POINTER(C.c_uint32)), ("count_rc", C.POINTER(C.c_uint32)),
                ("visible_forward", C.c_uint64), ("visible_rc", C.c_uint64),
                ("hover_start", C.POINTER(C.c_uint64)), ("hover_length", C.POINTER(C.c_uint64)),
                ("hover_ref", C.POINTER(C.c_uint64))]


class RlzResult(C.Structure):
    """Mirror of nolzss_rlz_result (include/nolzss_hip.h)."""
    _fields_ = [("num_targets", C.c_size_t), ("block_length", C.c_uint64),
                ("target_offsets", C.POINTER(C.c_uint64)), ("target_lengths", C.POINTER(C.c_uint64)),
                ("counts", C.POINTER(C.c_size_t)), ("factors", C.POINTER(C.c_void_p)), ("block", C.c_void_p),
                ("reference_ids", C.c_void_p), ("reference_ids_bytes", C.c_size_t), ("num_references", C.c_size_t),
                ("target_ids", C.c_void_p), ("target_ids_bytes", C.c_size_t)]


class DecodeInfo(C.Structure):
    """Mirror of nolzss_decode_info (include/nolzss_hip.h)."""
    _fields_ = [("n", C.c_uint64), ("z", C.c_uint64), ("n_literals", C.c_uint64), ("resolved_at_expand", C.c_uint64),
                ("rounds", C.c_uint64), ("max_active", C.c_uint64)]


class RlzRange(C.Structure):
    """Mirror of nolzss_rlz_range (include/nolzss_hip.h)."""
    _fields_ = [("target", C.c_uint64), ("lo", C.c_uint64), ("hi", C.c_uint64)]


class RlzArchiveSummary(C.Structure):
    """Mirror of nolzss_rlz_archive_summary (include/nolzss_hip.h)."""
    _fields_ = [("num_targets", C.c_uint64), ("block_length", C.c_uint64), ("z", C.c_uint64), ("n_literals", C.c_uint64),
                ("total_length", C.c_uint64), ("target_lengths", C.POINTER(C.c_uint64)), ("device", C.c_int32),
                ("device_bytes", C.c_uint64)]


class RlzArchiveAppendInfo(C.Structure):
    """Mirror of nolzss_rlz_archive_append_info (include/nolzss_hip.h)."""
    _fields_ = [("targets_added", C.c_uint64), ("records_added", C.c_uint64), ("literals_added", C.c_uint64),
                ("bases_added", C.c_uint64), ("num_targets", C.c_uint64), ("z", C.c_uint64), ("total_length", C.c_uint64),
                ("capacity_records", C.c_uint64), ("device_bytes", C.c_uint64), ("reallocated", C.c_int32)]


class RlzArchivePacked(C.Structure):
    """Mirror of nolzss_rlz_archive_packed (include/nolzss_hip.h)."""
    _fields_ = [("block_mode", C.c_uint32), ("literal_mode", C.c_uint32), ("block_length", C.c_uint64), ("z", C.c_uint64),
                ("n_literals", C.c_uint64), ("decoded", C.c_uint64), ("num_separators", C.c_uint64),
                ("block", C.c_void_p), ("control", C.c_void_p), ("data", C.c_void_p), ("literals", C.c_void_p),
                ("block_bytes", C.c_uint64), ("control_bytes", C.c_uint64), ("data_bytes", C.c_uint64),
                ("literal_bytes", C.c_uint64)]


class PackedFactors(C.Structure):
    """Mirror of nolzss_packed_factors (include/nolzss_hip.h)."""
    _fields_ = [("literal_mode", C.c_uint32), ("reserved", C.c_uint32), ("first_start", C.c_uint64), ("z", C.c_uint64),
                ("n_literals", C.c_uint64), ("decoded", C.c_uint64),
                ("control", C.c_void_p), ("data", C.c_void_p), ("literals", C.c_void_p),
                ("control_bytes", C.c_uint64), ("data_bytes", C.c_uint64), ("literal_bytes", C.c_uint64)]


class RlzFinderSummary(C.Structure):
    """Mirror of nolzss_rlz_finder_summary (include/nolzss_hip.h)."""
    _fields_ = [("num_targets", C.c_uint64), ("z", C.c_uint64), ("total_length", C.c_uint64),
                ("max_pattern_length", C.c_uint64), ("kernel_length", C.c_uint64), ("intervals", C.c_uint64),
                ("with_rc", C.c_int32), ("device", C.c_int32), ("device_bytes", C.c_uint64)]


class RlzIndexSummary(C.Structure):
    """Mirror of nolzss_rlz_index_summary (include/nolzss_hip.h)."""
    _fields_ = [("num_references", C.c_uint64), ("block_length", C.c_uint64), ("index_length", C.c_uint64),
                ("with_rc", C.c_int32), ("device", C.c_int32), ("prefix_syms", C.c_uint32), ("device_bytes", C.c_uint64)]


class RlzSeedsResult(C.Structure):
    """Mirror of nolzss_rlz_seeds_result (include/nolzss_hip.h)."""
    _fields_ = [("num_seeds", C.c_size_t), ("seeds", C.c_void_p), ("hit_offsets", C.c_void_p), ("num_hits", C.c_size_t),
                ("hits", C.c_void_p)]


class RlzRepeatsResult(C.Structure):
    """Mirror of nolzss_rlz_repeats_result (include/nolzss_hip.h)."""
    _fields_ = [("num_repeats", C.c_size_t), ("repeats", C.c_void_p), ("hit_offsets", C.c_void_p), ("hits", C.c_void_p),
                ("num_hits", C.c_size_t)]


class RlzChainParams(C.Structure):
    """Mirror of nolzss_rlz_chain_params (include/nolzss_hip.h)."""
    _fields_ = [("min_length", C.c_uint64), ("max_hits", C.c_uint64), ("max_gap", C.c_uint64), ("bandwidth", C.c_uint64),
                ("min_score", C.c_uint64)]


class RlzSeedChainsResult(C.Structure):
    """Mirror of nolzss_rlz_seed_chains_result (include/nolzss_hip.h)."""
    _fields_ = [("num_chains", C.c_size_t), ("chains", C.c_void_p), ("anchor_offsets", C.c_void_p),
                ("num_anchors", C.c_size_t), ("anchors", C.c_void_p), ("num_seeds", C.c_size_t),
                ("num_seed_hits", C.c_size_t)]


class RlzAlignParams(C.Structure):
    """Mirror of nolzss_rlz_align_params (include/nolzss_hip.h)."""
    _fields_ = [("min_length", C.c_uint64), ("max_hits", C.c_uint64), ("max_gap", C.c_uint64), ("bandwidth", C.c_uint64),
                ("min_score", C.c_uint64), ("band", C.c_uint64), ("max_flank", C.c_uint64)]


class RlzAlignResult(C.Structure):
    """Mirror of nolzss_rlz_align_result (include/nolzss_hip.h)."""
    _fields_ = [("num_alignments", C.c_size_t), ("alignments", C.c_void_p), ("op_offsets", C.c_void_p),
                ("num_ops", C.c_size_t), ("ops", C.c_void_p), ("num_jobs", C.c_size_t), ("num_rows", C.c_size_t)]


class RlzPileupAddInfo(C.Structure):
    """Mirror of nolzss_rlz_pileup_add_info (include/nolzss_hip.h)."""
    _fields_ = [("alignments", C.c_uint64), ("ops", C.c_uint64), ("columns", C.c_uint64), ("targets", C.c_uint64)]


class RlzPileupSummary(C.Structure):
    """Mirror of nolzss_rlz_pileup_summary (include/nolzss_hip.h)."""
    _fields_ = [("block_length", C.c_uint64), ("device_bytes", C.c_uint64), ("targets", C.c_uint64),
                ("alignments", C.c_uint64), ("ops", C.c_uint64), ("columns", C.c_uint64), ("adds", C.c_uint64),
                ("device", C.c_int32), ("dirty", C.c_int32), ("params", RlzAlignParams)]


class RlzVariant(C.Structure):
    """Mirror of nolzss_rlz_variant (include/nolzss_hip.h)."""
    _fields_ = [("position", C.c_uint64), ("record_offset", C.c_uint64), ("record", C.c_uint32), ("ref_base", C.c_uint32),
                ("allele", C.c_uint32), ("count", C.c_uint32), ("depth", C.c_uint32), ("rev", C.c_uint32)]


class RlzVariantsResult(C.Structure):
    """Mirror of nolzss_rlz_variants_result (include/nolzss_hip.h)."""
    _fields_ = [("num_variants", C.c_size_t), ("variants", C.c_void_p)]


class RlzInsertion(C.Structure):
    """Mirror of nolzss_rlz_insertion (include/nolzss_hip.h)."""
    _fields_ = [("position", C.c_uint64), ("record_offset", C.c_uint64), ("record", C.c_uint32), ("length", C.c_uint32),
                ("count", C.c_uint32), ("depth", C.c_uint32), ("ins_total", C.c_uint32), ("truncated", C.c_uint32),
                ("bases", C.c_uint64 * 2)]


class RlzInsertionsResult(C.Structure):
    """Mirror of nolzss_rlz_insertions_result (include/nolzss_hip.h)."""
    _fields_ = [("num_insertions", C.c_size_t), ("insertions", C.c_void_p)]


class RlzConsensusParams(C.Structure):
    """Mirror of nolzss_rlz_consensus_params (include/nolzss_hip.h)."""
    _fields_ = [("min_depth", C.c_uint32), ("low", C.c_uint32), ("num", C.c_uint64), ("den", C.c_uint64)]


class RlzConsensusResult(C.Structure):
    """Mirror of nolzss_rlz_consensus_result (include/nolzss_hip.h)."""
    _fields_ = [("length", C.c_size_t), ("text", C.c_void_p), ("num_records", C.c_size_t), ("record_offsets", C.c_void_p),
                ("starts", C.c_void_p), ("called", C.c_uint64), ("low_positions", C.c_uint64), ("substitutions", C.c_uint64),
                ("deleted", C.c_uint64), ("insertions", C.c_uint64), ("inserted_bases", C.c_uint64),
                ("truncated_skipped", C.c_uint64)]


class RlzCohortSampleInfo(C.Structure):
    """Mirror of nolzss_rlz_cohort_sample_info (include/nolzss_hip.h)."""
    _fields_ = [("sample", C.c_uint64), ("called", C.c_uint64), ("low", C.c_uint64), ("deleted", C.c_uint64),
                ("differs", C.c_uint64)]


class RlzCohortSummary(C.Structure):
    """Mirror of nolzss_rlz_cohort_summary (include/nolzss_hip.h)."""
    _fields_ = [("samples", C.c_uint64), ("capacity", C.c_uint64), ("block_length", C.c_uint64), ("device_bytes", C.c_uint64),
                ("device", C.c_int32), ("reserved", C.c_int32)]


class RlzCohortDistancesResult(C.Structure):
    """Mirror of nolzss_rlz_cohort_distances_result (include/nolzss_hip.h)."""
    _fields_ = [("num_samples", C.c_size_t), ("differences", C.c_void_p), ("compared", C.c_void_p)]


class RlzCohortSitesResult(C.Structure):
    """Mirror of nolzss_rlz_cohort_sites_result (include/nolzss_hip.h)."""
    _fields_ = [("num_sites", C.c_size_t), ("sites", C.c_void_p)]


class Factor(C.Structure):
    """Mirror of nolzss_factor / the reference's struct Factor (factorizer.hpp:147-151)."""
    _fields_ = [("start", C.c_uint64), ("length", C.c_uint64), ("ref", C.c_uint64)]


def _share_hip_runtime_with_torch():
    """PyTorch-ROCm wheels bundle their own libamdhip64; a process that initialises the system's HIP runtime
    first (through this library) and torch's afterwards ends up with two runtimes, and torch then reports no
    GPU.  When torch is installed, its runtime is loaded first so that libnolzss_hip.so binds to the same one
    (the loader resolves the SONAME to the copy already in the process) -- whatever the import order.
    NOLZSS_SYSTEM_HIP=1 keeps the system runtime."""
    import importlib.util
    import os
    if os.environ.get("NOLZSS_SYSTEM_HIP"):
        return
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        return
    if spec is None or not spec.origin:
        return
    cand = Path(spec.origin).resolve().parent / "lib" / "libamdhip64.so"
    if cand.exists():
        try:
            C.CDLL(str(cand), mode=C.RTLD_GLOBAL)
        except OSError:
            pass


def _load():
    if not LIB_PATH.exists():
        raise ImportError(
            f"{LIB_PATH} not found: build the HIP extension first "
            "(python -c 'import __graft_entry__ as g; g.build()' or make -C nolzss_amd/csrc). "
            "nolzss_amd has no CPU fallback.")
    _share_hip_runtime_with_torch()
    lib = C.CDLL(str(LIB_PATH))
    vp, sz = C.c_void_p, C.c_size_t
    szp, vpp = C.POINTER(C.c_size_t), C.POINTER(C.c_void_p)
    lib.nolzss_last_error.restype = C.c_char_p
    lib.nolzss_version.restype = C.c_char_p
    lib.nolzss_free.argtypes = [vp]
    lib.nolzss_free.restype = None
    lib.nolzss_device_count.argtypes = [C.POINTER(C.c_int)]
    lib.nolzss_factorize.argtypes = [vp, sz, sz, C.c_int, vpp, szp]
    lib.nolzss_count_factors.argtypes = [vp, sz, sz, C.c_int, szp]
    lib.nolzss_factorize_file.argtypes = [C.c_char_p, sz, C.c_int, vpp, szp]
    lib.nolzss_count_factors_file.argtypes = [C.c_char_p, sz, C.c_int, szp]
    lib.nolzss_factorize_device.argtypes = [vp, sz, sz, C.c_int, vp, C.c_int, vpp, szp]
    lib.nolzss_prepare_multiple_dna_w_rc.argtypes = [
        C.POINTER(C.c_char_p), C.POINTER(C.c_size_t), sz, vpp, szp, szp, vpp, szp]
    lib.nolzss_factorize_multiple_dna_w_rc.argtypes = [vp, sz, sz, C.c_int, vpp, szp]
    lib.nolzss_count_factors_multiple_dna_w_rc.argtypes = [vp, sz, sz, C.c_int, szp]
    lib.nolzss_factorize_dna_w_rc.argtypes = [vp, sz, C.c_int, vpp, szp]
    lib.nolzss_count_factors_dna_w_rc.argtypes = [vp, sz, C.c_int, szp]
    lib.nolzss_factorize_dna_w_rc_device.argtypes = [vp, sz, C.c_int, vp, C.c_int, vpp, szp]
    lib.nolzss_factorize_w_reference.argtypes = [vp, sz, vp, sz, C.c_int, vpp, szp]
    lib.nolzss_factorize_dna_w_reference_seq.argtypes = [C.c_char_p, sz, C.c_char_p, sz, C.c_int, vpp, szp]
    lib.nolzss_write_factors_binary_file.argtypes = [C.c_char_p, C.c_char_p, C.c_int, szp]
    lib.nolzss_write_factors_binary_file_dna_w_rc.argtypes = [C.c_char_p, C.c_char_p, C.c_int, szp]
    lib.nolzss_factorize_w_reference_file.argtypes = [vp, sz, vp, sz, C.c_char_p, C.c_int, szp]
    lib.nolzss_factorize_dna_w_reference_seq_file.argtypes = [C.c_char_p, sz, C.c_char_p, sz, C.c_char_p,
                                                              C.c_int, szp]
    lib.nolzss_write_factor_file.argtypes = [C.c_char_p, vp, sz, C.c_uint64, C.c_uint64, C.c_uint64, vp, sz]
    lib.nolzss_prepare_multiple_dna_no_rc.argtypes = [
        C.POINTER(C.c_char_p), C.POINTER(C.c_size_t), sz, vpp, szp, szp, vpp, szp]
    lib.nolzss_factorize_fasta_multiple_dna.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_int,
                                                        C.POINTER(FastaResult)]
    lib.nolzss_free_fasta_result.argtypes = [C.POINTER(FastaResult)]
    lib.nolzss_free_fasta_result.restype = None
    lib.nolzss_write_factors_binary_file_fasta_multiple_dna.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.c_int,
                                                                        C.c_int, szp]
    lib.nolzss_factorize_dna_rc_w_ref_fasta_files.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.c_int,
                                                              C.POINTER(FastaResult)]
    lib.nolzss_write_factors_dna_w_reference_fasta_files_to_binary.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p,
                                                                               C.c_int, C.c_int, szp]
    lib.nolzss_factorize_fasta_per_sequence.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_char_p, C.c_int,
                                                        C.POINTER(FastaPerSequenceResult)]
    lib.nolzss_free_fasta_per_sequence_result.argtypes = [C.POINTER(FastaPerSequenceResult)]
    lib.nolzss_free_fasta_per_sequence_result.restype = None
    lib.nolzss_factorize_batch.argtypes = [
        C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), sz, C.POINTER(C.c_int), sz,
        C.POINTER(C.POINTER(C.c_void_p)), C.POINTER(C.POINTER(C.c_size_t))]
    lib.nolzss_factorize_batch_dna_w_rc.argtypes = lib.nolzss_factorize_batch.argtypes
    lib.nolzss_factorize_batch_device.argtypes = [C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), sz, C.c_int, C.c_int,
                                                  C.POINTER(C.c_size_t)]
    lib.nolzss_count_factors_batch_both.argtypes = [C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), sz, C.POINTER(C.c_int),
                                                    sz, szp, szp]
    lib.nolzss_free_batch.argtypes = [C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), sz]
    lib.nolzss_free_batch.restype = None
    lib.nolzss_read_nucleotide_fasta.argtypes = [C.c_char_p, C.POINTER(C.c_int), sz, C.c_int, sz, sz,
                                                 C.POINTER(NucleotideFasta)]
    lib.nolzss_free_nucleotide_fasta.argtypes = [C.POINTER(NucleotideFasta)]
    lib.nolzss_free_nucleotide_fasta.restype = None
    lib.nolzss_debug_parse_nucleotide_fasta.argtypes = [C.c_char_p, C.POINTER(C.c_void_p), szp, C.POINTER(C.c_void_p),
                                                        szp, szp]
    lib.nolzss_debug_lpt_plan.argtypes = [szp, sz, sz, szp]
    lib.nolzss_debug_batch_plan.argtypes = [szp, sz, sz, C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_int32), szp]
    lib.nolzss_free_length_hist.argtypes = [C.POINTER(LengthHist)]
    lib.nolzss_free_length_hist.restype = None
    lib.nolzss_factor_length_histogram.argtypes = [vp, sz, C.c_int, C.c_int, C.c_uint64, C.c_int, C.POINTER(LengthHist)]
    lib.nolzss_factor_length_histogram_with_lengths.argtypes = [vp, sz, C.c_int, C.c_int, C.POINTER(LengthHist)]
    lib.nolzss_fasta_factor_length_histogram.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_uint64, C.c_int,
                                                         C.POINTER(LengthHist)]
    lib.nolzss_fasta_factor_length_histogram_with_lengths.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_int,
                                                                      C.POINTER(LengthHist)]
    lib.nolzss_fasta_shuffled_text.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_uint64, C.c_int, vpp, szp]
    lib.nolzss_factor_lengths.argtypes = [vp, sz, C.c_int, C.c_int, vpp, szp]
    lib.nolzss_shuffle_dna.argtypes = [vp, sz, C.c_uint64, C.c_int, vpp]
    rqp, fmp = C.POINTER(FactorMapRequest), C.POINTER(FactorMaps)
    lib.nolzss_free_factor_maps.argtypes = [fmp]
    lib.nolzss_free_factor_maps.restype = None
    lib.nolzss_factor_maps_text.argtypes = [vp, sz, C.c_int, C.c_int, rqp, fmp]
    lib.nolzss_factor_maps_fasta.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_int, rqp, fmp]
    lib.nolzss_factor_maps_records.argtypes = [vp, sz, vp, sz, C.c_int, rqp, fmp]
    lib.nolzss_dotplot_open_text.argtypes = [vp, sz, C.c_int, C.c_int, vpp]
    lib.nolzss_dotplot_open_fasta.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_int, vpp]
    lib.nolzss_dotplot_open_records.argtypes = [vp, sz, vp, sz, C.c_int, vpp]
    lib.nolzss_dotplot_info.argtypes = [vp, C.POINTER(DotPlotSummary)]
    lib.nolzss_dotplot_render.argtypes = [vp, C.POINTER(DotPlotView), C.POINTER(DotPlotRaster)]
    lib.nolzss_free_dotplot_raster.argtypes = [C.POINTER(DotPlotRaster)]
    lib.nolzss_free_dotplot_raster.restype = None
    lib.nolzss_dotplot_close.argtypes = [vp]
    lib.nolzss_debug_position_edges.argtypes = [C.c_uint64, C.c_uint32, C.c_uint64, vpp, szp]
    seqs = [C.POINTER(C.c_char_p), szp, sz, C.POINTER(C.c_char_p), szp, sz]  # references, then targets
    lib.nolzss_rlz_prepare.argtypes = seqs + [C.c_int, vpp, szp, vpp, szp, szp, szp]
    lib.nolzss_rlz_factorize.argtypes = seqs + [C.c_int, C.c_int, C.c_int, C.POINTER(RlzResult)]
    lib.nolzss_rlz_factorize_fasta.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_int,
                                               C.POINTER(RlzResult)]
    lib.nolzss_free_rlz_result.argtypes = [C.POINTER(RlzResult)]
    lib.nolzss_free_rlz_result.restype = None
    lib.nolzss_debug_rlz_codes.argtypes = seqs + [C.c_int, C.c_int, vp]
    u64p, dip = C.POINTER(C.c_uint64), C.POINTER(DecodeInfo)
    lib.nolzss_literal_symbols.argtypes = [vp, sz, vp, sz, vpp, szp]
    lib.nolzss_decode.argtypes = [vp, sz, vp, sz, vp, sz, C.c_int, vpp, szp, dip]
    lib.nolzss_roundtrip.argtypes = [vp, sz, C.c_int, C.c_int, szp, u64p, u64p, dip]
    lib.nolzss_roundtrip_device.argtypes = [vp, sz, C.c_int, C.c_int, vp, szp, u64p, u64p, dip]
    lib.nolzss_debug_count_mismatches.argtypes = [vp, vp, sz, C.c_int, u64p, u64p]
    if hasattr(lib, "nolzss_factors_pack"):  # (NOLZSS_LIB: a variant built from an older commit has none)
        pfp = C.POINTER(PackedFactors)
        lib.nolzss_factors_pack.argtypes = [vp, sz, vp, sz, C.c_int, C.c_int, pfp]
        lib.nolzss_factorize_packed.argtypes = [vp, sz, C.c_int, C.c_int, C.c_int, pfp]
        lib.nolzss_factorize_packed_device.argtypes = [vp, sz, C.c_int, C.c_int, C.c_int, vp, pfp]
        lib.nolzss_free_packed_factors.argtypes = [pfp]
        lib.nolzss_free_packed_factors.restype = None
        lib.nolzss_factors_unpack.argtypes = [pfp, C.c_int, vpp, szp, vpp, szp]
        lib.nolzss_decode_packed.argtypes = [pfp, vp, sz, C.c_int, vpp, szp, dip]
    lib.nolzss_rlz_archive_open_records.argtypes = [vp, sz, vp, sz, vp, sz, vp, sz, C.c_int, vpp]
    lib.nolzss_rlz_archive_info.argtypes = [vp, C.POINTER(RlzArchiveSummary)]
    lib.nolzss_rlz_archive_extract.argtypes = [vp, vp, sz, vpp, vpp, u64p]
    lib.nolzss_rlz_archive_extract_device.argtypes = [vp, vp, sz, vp, sz, vp, u64p]
    lib.nolzss_rlz_archive_close.argtypes = [vp]
    lib.nolzss_rlz_index_open.argtypes = seqs[:3] + [C.c_int, C.c_uint32, C.c_int, vpp]
    lib.nolzss_rlz_index_open_fasta.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_uint32, C.c_int, vpp]
    lib.nolzss_rlz_index_info.argtypes = [vp, C.POINTER(RlzIndexSummary)]
    lib.nolzss_rlz_index_factorize.argtypes = [vp] + seqs[3:] + [C.c_int, C.POINTER(RlzResult)]
    lib.nolzss_rlz_index_codes.argtypes = [vp] + seqs[3:] + [vp]
    lib.nolzss_rlz_index_close.argtypes = [vp]
    lib.nolzss_rlz_index_count.argtypes = [vp] + seqs[3:] + [vp]
    lib.nolzss_rlz_index_locate.argtypes = [vp] + seqs[3:] + [C.c_uint64, vp, vp, vpp, szp]
    lib.nolzss_rlz_index_seeds.argtypes = [vp] + seqs[3:] + [C.c_uint64, C.c_uint64, C.POINTER(RlzSeedsResult)]
    lib.nolzss_free_rlz_seeds_result.argtypes = [C.POINTER(RlzSeedsResult)]
    lib.nolzss_free_rlz_seeds_result.restype = None
    if hasattr(lib, "nolzss_rlz_index_repeats"):  # (NOLZSS_LIB: a variant built from an older commit has none)
        lib.nolzss_rlz_index_repeat_count.argtypes = [vp, C.c_uint64, C.c_uint64, u64p]
        lib.nolzss_rlz_index_repeats.argtypes = [vp, C.c_uint64, C.c_uint64, C.c_uint64, C.POINTER(RlzRepeatsResult)]
        lib.nolzss_free_rlz_repeats_result.argtypes = [C.POINTER(RlzRepeatsResult)]
        lib.nolzss_free_rlz_repeats_result.restype = None
        lib.nolzss_debug_rlz_repeats_refusal.argtypes = [C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64]
        lib.nolzss_debug_rlz_repeat_shifts.argtypes = [C.c_uint64, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    lib.nolzss_rlz_index_seed_chains.argtypes = [vp] + seqs[3:] + [C.POINTER(RlzChainParams), C.POINTER(RlzSeedChainsResult)]
    lib.nolzss_free_rlz_seed_chains_result.argtypes = [C.POINTER(RlzSeedChainsResult)]
    lib.nolzss_free_rlz_seed_chains_result.restype = None
    lib.nolzss_debug_rlz_seed_chain.argtypes = [vp, vp, vp, vp, vp, sz, C.POINTER(RlzChainParams), C.c_uint64, C.c_uint32,
                                                C.c_int, vp, vp, C.POINTER(RlzSeedChainsResult)]
    lib.nolzss_rlz_index_align.argtypes = [vp] + seqs[3:] + [C.POINTER(RlzAlignParams), C.POINTER(RlzAlignResult)]
    lib.nolzss_free_rlz_align_result.argtypes = [C.POINTER(RlzAlignResult)]
    lib.nolzss_free_rlz_align_result.restype = None
    lib.nolzss_debug_rlz_align_jobs.argtypes = [C.c_char_p, sz, C.c_char_p, sz, vp, vp, vp, vp, vp, sz, C.c_uint32, C.c_int,
                                                vp, vp, vp, vpp]
    lib.nolzss_rlz_pileup_open.argtypes = [vp, C.POINTER(RlzAlignParams), vpp]
    lib.nolzss_rlz_pileup_add.argtypes = [vp] + seqs[3:] + [C.c_int, C.POINTER(RlzPileupAddInfo)]
    lib.nolzss_rlz_pileup_counts.argtypes = [vp, C.c_uint64, C.c_uint64, vp]
    lib.nolzss_rlz_pileup_variants.argtypes = [vp, C.c_uint32, C.c_uint64, C.c_uint64, C.POINTER(RlzVariantsResult)]
    lib.nolzss_free_rlz_variants_result.argtypes = [C.POINTER(RlzVariantsResult)]
    lib.nolzss_free_rlz_variants_result.restype = None
    lib.nolzss_rlz_pileup_info.argtypes = [vp, C.POINTER(RlzPileupSummary)]
    lib.nolzss_rlz_pileup_close.argtypes = [vp]
    lib.nolzss_debug_rlz_pileup.argtypes = [vp, sz] + seqs[3:] + [vp, vp, sz, vp, sz, C.c_int, C.c_int, vp]
    lib.nolzss_rlz_pileup_open_flags.argtypes = [vp, C.POINTER(RlzAlignParams), C.c_uint32, vpp]
    lib.nolzss_rlz_pileup_log_info.argtypes = [vp, C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    lib.nolzss_rlz_pileup_insertions.argtypes = [vp, C.c_uint32, C.c_uint64, C.c_uint64, C.POINTER(RlzInsertionsResult)]
    lib.nolzss_free_rlz_insertions_result.argtypes = [C.POINTER(RlzInsertionsResult)]
    lib.nolzss_free_rlz_insertions_result.restype = None
    lib.nolzss_rlz_pileup_consensus.argtypes = [vp, C.POINTER(RlzConsensusParams), C.c_int, C.POINTER(RlzConsensusResult)]
    lib.nolzss_free_rlz_consensus_result.argtypes = [C.POINTER(RlzConsensusResult)]
    lib.nolzss_free_rlz_consensus_result.restype = None
    lib.nolzss_debug_rlz_pileup_consensus.argtypes = [vp, sz] + seqs[3:] + [vp, vp, sz, vp, sz, C.c_int, C.c_uint32,
                                                      C.POINTER(RlzConsensusParams), C.c_int, vp,
                                                      C.POINTER(RlzInsertionsResult), C.POINTER(RlzConsensusResult)]
    if hasattr(lib, "nolzss_rlz_cohort_open"):  # (NOLZSS_LIB: a variant built from an older commit has none)
        lib.nolzss_rlz_cohort_open.argtypes = [vp, vpp]
        lib.nolzss_rlz_cohort_add_pileup.argtypes = [vp, vp, C.POINTER(RlzConsensusParams), C.POINTER(RlzCohortSampleInfo)]
        lib.nolzss_rlz_cohort_add_calls.argtypes = [vp, vp, sz, C.POINTER(RlzCohortSampleInfo)]
        lib.nolzss_rlz_cohort_info.argtypes = [vp, C.POINTER(RlzCohortSummary)]
        lib.nolzss_rlz_cohort_samples.argtypes = [vp, vp, sz, szp]
        lib.nolzss_rlz_cohort_distances.argtypes = [vp, C.POINTER(RlzCohortDistancesResult)]
        lib.nolzss_free_rlz_cohort_distances_result.argtypes = [C.POINTER(RlzCohortDistancesResult)]
        lib.nolzss_free_rlz_cohort_distances_result.restype = None
        lib.nolzss_rlz_cohort_sites.argtypes = [vp, C.c_uint64, C.c_int, C.POINTER(RlzCohortSitesResult)]
        lib.nolzss_free_rlz_cohort_sites_result.argtypes = [C.POINTER(RlzCohortSitesResult)]
        lib.nolzss_free_rlz_cohort_sites_result.restype = None
        lib.nolzss_rlz_cohort_columns.argtypes = [vp, vp, sz, vp]
        lib.nolzss_rlz_cohort_calls.argtypes = [vp, C.c_uint64, C.c_uint64, C.c_uint64, vp]
        lib.nolzss_rlz_cohort_close.argtypes = [vp]
    lib.nolzss_debug_rlz_locate_shifts.argtypes = [C.c_uint64, C.c_uint64, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    lib.nolzss_rlz_archive_open_index.argtypes = [vp, vpp]
    lib.nolzss_rlz_archive_append_index.argtypes = [vp, vp] + seqs[3:] + [C.POINTER(RlzArchiveAppendInfo)]
    lib.nolzss_rlz_archive_export.argtypes = [vp, vpp, szp, vpp, szp, vpp, szp]
    lib.nolzss_rlz_archive_pack.argtypes = [vp, C.POINTER(RlzArchivePacked)]
    lib.nolzss_free_rlz_archive_packed.argtypes = [C.POINTER(RlzArchivePacked)]
    lib.nolzss_free_rlz_archive_packed.restype = None
    lib.nolzss_rlz_archive_open_packed.argtypes = [C.POINTER(RlzArchivePacked), vp, sz, C.c_int, vpp]
    lib.nolzss_rlz_finder_open.argtypes = [vp, vp, C.c_uint64, C.c_uint32, vpp]
    lib.nolzss_rlz_finder_info.argtypes = [vp, C.POINTER(RlzFinderSummary)]
    lib.nolzss_rlz_finder_count.argtypes = [vp] + seqs[3:] + [vp]
    lib.nolzss_rlz_finder_locate.argtypes = [vp] + seqs[3:] + [C.c_uint64, vp, vp, vpp, szp]
    lib.nolzss_rlz_finder_kernel.argtypes = [vp, vpp, szp, vpp, vpp, szp]
    lib.nolzss_rlz_finder_close.argtypes = [vp]
    lib.nolzss_profile_enable.argtypes = [C.c_int, C.c_int]
    lib.nolzss_profile_reset.argtypes = [C.c_int]
    lib.nolzss_profile_report.argtypes = [C.c_int, C.c_char_p, sz]
    lib.nolzss_debug_arrays.argtypes = [vp, sz, C.c_int, vp, vp, vp, vp]
    lib.nolzss_debug_position_factors.argtypes = [vp, sz, C.c_int, vp]
    lib.nolzss_debug_rc_arrays.argtypes = [vp, sz, C.c_int, C.c_int, vp, vp, vp, vp, vp, vp, vp]
    lib.nolzss_debug_sort_pairs.argtypes = [vp, vp, sz, C.c_int]
    lib.nolzss_debug_scan.argtypes = [vp, sz, C.c_int, C.c_int]
    lib.nolzss_debug_pyramid.argtypes = [vp, sz, C.c_int, C.c_int, vp, sz, C.c_uint32, C.c_int, vp, sz, C.c_int,
                                         C.POINTER(C.c_int), vp, vp, sz, vp, vp]
    lib.nolzss_debug_nearest.argtypes = [vp, vp, sz, C.c_int, vp, sz, C.c_int, vp]
    lib.nolzss_debug_lds_search.argtypes = [vp, vp, sz, C.c_int, C.c_uint32, C.c_int, C.c_int, vp, vp]
    lib.nolzss_debug_local_sort.argtypes = [vp, vp, sz, vp, sz, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, vp,
                                            vp, vp, vp, vp]
    lib.nolzss_debug_text_order.argtypes = [vp, vp, vp, sz, sz, C.c_uint32, C.c_uint32, sz, C.c_uint32, vp, sz, C.c_int,
                                            vp, vp, vp, vp, vp, vp, vp]
    lib.nolzss_debug_group_sort.argtypes = [vp, sz, vp, vp, vp, sz, C.c_uint32, C.c_int, C.c_uint32, C.c_uint32, vp, C.c_int,
                                            vp, vp, vp, vp]
    lib.nolzss_debug_direct_round.argtypes = [vp, sz, vp, vp, vp, sz, C.c_uint32, C.c_uint32, C.c_uint32, vp, C.c_uint32,
                                              C.c_int, vp, vp, vp, vp, vp, vp, vp]
    if hasattr(lib, "nolzss_debug_repeat_pass"):  # (NOLZSS_LIB: a variant built from an older commit has none)
        lib.nolzss_debug_repeat_pass.argtypes = [vp, sz, vp, vp, vp, vp, vp, sz, C.c_uint32, C.c_int, C.c_int, C.c_int, vp,
                                                 vp, vp, vp, vp, vp]
    lib.nolzss_debug_chain.argtypes = [vp, sz, sz, C.c_int, C.c_uint32, vp, sz, sz, C.c_uint32, C.c_int, vp, sz, C.c_int,
                                       vp, vp, vp, vp, vp, vp, vp, vp]
    if hasattr(lib, "nolzss_debug_cursor"):  # (NOLZSS_LIB: a variant built from an older commit has none)
        lib.nolzss_debug_cursor.argtypes = [C.c_int, vp]
    lib.nolzss_debug_arena.argtypes = [C.c_int, szp, szp]
    if hasattr(lib, "nolzss_debug_device_buffers"):  # (NOLZSS_LIB: a variant built from an older commit has none)
        lib.nolzss_debug_device_buffers.argtypes = [szp, szp]
    lib.nolzss_debug_trim_arenas.argtypes = [C.c_int, szp]
    lib.nolzss_debug_parse_fasta.argtypes = [C.c_char_p, C.c_int, C.POINTER(C.c_void_p), szp, C.POINTER(C.c_void_p),
                                             szp, szp]
    lib.nolzss_debug_batch_counters.argtypes = [C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    lib.nolzss_debug_batch_counters.restype = None
    return lib


lib = _load()

EXPORTED_SYMBOLS = [
    "nolzss_last_error", "nolzss_version", "nolzss_free", "nolzss_device_count",
    "nolzss_factorize", "nolzss_count_factors", "nolzss_factorize_file", "nolzss_count_factors_file",
    "nolzss_factorize_device", "nolzss_prepare_multiple_dna_w_rc",
    "nolzss_factorize_multiple_dna_w_rc", "nolzss_count_factors_multiple_dna_w_rc",
    "nolzss_factorize_dna_w_rc", "nolzss_count_factors_dna_w_rc", "nolzss_factorize_batch",
    "nolzss_factorize_w_reference", "nolzss_factorize_dna_w_reference_seq",
    "nolzss_write_factors_binary_file", "nolzss_write_factors_binary_file_dna_w_rc",
    "nolzss_factorize_w_reference_file", "nolzss_factorize_dna_w_reference_seq_file",
    "nolzss_write_factor_file", "nolzss_prepare_multiple_dna_no_rc", "nolzss_factorize_fasta_multiple_dna",
    "nolzss_free_fasta_result", "nolzss_write_factors_binary_file_fasta_multiple_dna",
    "nolzss_factorize_fasta_per_sequence", "nolzss_free_fasta_per_sequence_result",
    "nolzss_factorize_dna_rc_w_ref_fasta_files", "nolzss_write_factors_dna_w_reference_fasta_files_to_binary",
    "nolzss_free_batch", "nolzss_profile_enable", "nolzss_profile_reset", "nolzss_profile_report",
    "nolzss_debug_arrays", "nolzss_debug_sort_pairs", "nolzss_debug_scan", "nolzss_debug_arena",
    "nolzss_debug_device_buffers",
    "nolzss_debug_batch_counters", "nolzss_factorize_batch_dna_w_rc",
    "nolzss_debug_trim_arenas", "nolzss_debug_parse_fasta",
    "nolzss_read_nucleotide_fasta", "nolzss_free_nucleotide_fasta", "nolzss_debug_parse_nucleotide_fasta", "nolzss_debug_lpt_plan", "nolzss_debug_batch_plan", "nolzss_factorize_batch_device",
    "nolzss_factorize_dna_w_rc_device", "nolzss_count_factors_batch_both",
    "nolzss_free_length_hist", "nolzss_factor_length_histogram", "nolzss_factor_length_histogram_with_lengths",
    "nolzss_fasta_factor_length_histogram", "nolzss_fasta_factor_length_histogram_with_lengths",
    "nolzss_fasta_shuffled_text", "nolzss_factor_lengths", "nolzss_shuffle_dna",
    "nolzss_free_factor_maps", "nolzss_factor_maps_text", "nolzss_factor_maps_fasta", "nolzss_factor_maps_records",
    "nolzss_debug_position_edges",
    "nolzss_dotplot_open_text", "nolzss_dotplot_open_fasta", "nolzss_dotplot_open_records", "nolzss_dotplot_info",
    "nolzss_dotplot_render", "nolzss_free_dotplot_raster", "nolzss_dotplot_close",
    "nolzss_debug_position_factors", "nolzss_debug_rc_arrays",
    "nolzss_rlz_prepare", "nolzss_rlz_factorize", "nolzss_rlz_factorize_fasta", "nolzss_free_rlz_result",
    "nolzss_debug_rlz_codes",
    "nolzss_literal_symbols", "nolzss_decode", "nolzss_roundtrip", "nolzss_roundtrip_device",
    "nolzss_debug_count_mismatches",
    "nolzss_factors_pack", "nolzss_factorize_packed", "nolzss_factorize_packed_device", "nolzss_free_packed_factors",
    "nolzss_factors_unpack", "nolzss_decode_packed",
    "nolzss_rlz_archive_open_records", "nolzss_rlz_archive_info", "nolzss_rlz_archive_extract",
    "nolzss_rlz_archive_extract_device", "nolzss_rlz_archive_close",
    "nolzss_rlz_index_open", "nolzss_rlz_index_open_fasta", "nolzss_rlz_index_info", "nolzss_rlz_index_factorize",
    "nolzss_rlz_index_codes", "nolzss_rlz_index_close", "nolzss_rlz_index_count", "nolzss_rlz_index_locate",
    "nolzss_debug_rlz_locate_shifts", "nolzss_rlz_index_seeds", "nolzss_free_rlz_seeds_result",
    "nolzss_rlz_index_repeat_count", "nolzss_rlz_index_repeats", "nolzss_free_rlz_repeats_result",
    "nolzss_debug_rlz_repeats_refusal", "nolzss_debug_rlz_repeat_shifts",
    "nolzss_rlz_archive_open_index", "nolzss_rlz_archive_append_index", "nolzss_rlz_archive_export",
    "nolzss_rlz_archive_pack", "nolzss_free_rlz_archive_packed", "nolzss_rlz_archive_open_packed",
    "nolzss_rlz_finder_open", "nolzss_rlz_finder_info", "nolzss_rlz_finder_count", "nolzss_rlz_finder_locate",
    "nolzss_rlz_finder_kernel", "nolzss_rlz_finder_close",
    "nolzss_debug_pyramid", "nolzss_debug_nearest", "nolzss_debug_lds_search",
    "nolzss_debug_local_sort", "nolzss_debug_text_order", "nolzss_debug_group_sort",
    "nolzss_debug_direct_round", "nolzss_debug_repeat_pass",
    "nolzss_debug_chain", "nolzss_debug_cursor",
    "nolzss_rlz_index_seed_chains", "nolzss_free_rlz_seed_chains_result", "nolzss_debug_rlz_seed_chain",
    "nolzss_rlz_index_align", "nolzss_free_rlz_align_result", "nolzss_debug_rlz_align_jobs",
    "nolzss_rlz_pileup_open", "nolzss_rlz_pileup_add", "nolzss_rlz_pileup_counts", "nolzss_rlz_pileup_variants",
    "nolzss_free_rlz_variants_result", "nolzss_rlz_pileup_info", "nolzss_rlz_pileup_close", "nolzss_debug_rlz_pileup",
    "nolzss_rlz_pileup_open_flags", "nolzss_rlz_pileup_log_info", "nolzss_rlz_pileup_insertions",
    "nolzss_free_rlz_insertions_result", "nolzss_rlz_pileup_consensus", "nolzss_free_rlz_consensus_result",
    "nolzss_debug_rlz_pileup_consensus",
    "nolzss_rlz_cohort_open", "nolzss_rlz_cohort_add_pileup", "nolzss_rlz_cohort_add_calls", "nolzss_rlz_cohort_info",
    "nolzss_rlz_cohort_samples", "nolzss_rlz_cohort_distances", "nolzss_free_rlz_cohort_distances_result",
    "nolzss_rlz_cohort_sites", "nolzss_free_rlz_cohort_sites_result", "nolzss_rlz_cohort_columns",
    "nolzss_rlz_cohort_calls", "nolzss_rlz_cohort_close",
]


def check(rc):
    """Map a status code to the exception the reference's pybind11 module would raise
    (std::invalid_argument -> ValueError, std::runtime_error -> RuntimeError;
    reference: src/cpp/bindings.cpp default exception translation)."""
    if rc == OK:
        return
    msg = lib.nolzss_last_error().decode("utf-8", "replace")
    if rc == ERR_INVALID_ARGUMENT:
        raise ValueError(msg)
    if rc == ERR_NOMEM:
        raise MemoryError(msg)
    raise RuntimeError(msg)
