"""Genomics entry points on the hot path (mirror of noLZSS.genomics,
reference: src/noLZSS/genomics/__init__.py:8-25)."""
from .._noLZSS import (
    factorize_dna_w_rc,
    count_factors_dna_w_rc,
    factorize_multiple_dna_w_rc,
    count_factors_multiple_dna_w_rc,
    prepare_multiple_dna_sequences_w_rc,
)
from .fasta import FASTAError, read_nucleotide_fasta, shard_nucleotide_fasta
from .sequences import is_dna_sequence, factorize_dna_w_reference_seq, factorize_dna_w_reference_seq_file
from .significance import (calculate_factor_length_threshold, infer_length_significance, extract_factor_lengths,
                           clopper_pearson_upper)

__all__ = [
    "factorize_dna_w_rc", "count_factors_dna_w_rc", "factorize_multiple_dna_w_rc",
    "count_factors_multiple_dna_w_rc", "prepare_multiple_dna_sequences_w_rc",
    "FASTAError", "read_nucleotide_fasta", "shard_nucleotide_fasta",
    "is_dna_sequence", "factorize_dna_w_reference_seq", "factorize_dna_w_reference_seq_file",
    "calculate_factor_length_threshold", "infer_length_significance", "extract_factor_lengths",
    "clopper_pearson_upper",
]
