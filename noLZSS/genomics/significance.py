"""noLZSS.genomics.significance (reference: src/noLZSS/genomics/significance.py): factor-length significance
against a shuffled control; the GPU extensions take both factorizations from the device.  The data layer of the
reference's plots is noLZSS.genomics.plots; drawing is not provided."""
from nolzss_amd.genomics.significance import (calculate_factor_length_threshold,  # noqa: F401
                                              clopper_pearson_upper, extract_factor_lengths,
                                              fasta_shuffled_control_significance, factor_length_histogram,
                                              infer_length_significance, shuffle_dna,
                                              shuffled_control_significance)

__all__ = ["clopper_pearson_upper", "extract_factor_lengths", "infer_length_significance",
           "calculate_factor_length_threshold", "shuffled_control_significance",
           "fasta_shuffled_control_significance", "factor_length_histogram", "shuffle_dna"]
