"""noLZSS.genomics.rlz (extension, no counterpart in the reference package): relative Lempel-Ziv of many targets
against one reference block from one suffix sort on the GPU."""
from nolzss_amd.genomics.rlz import (ALIGN_DTYPE, PILEUP_CHANNELS, VARIANT_DTYPE, INSERTION_DTYPE, insertion_bases, RlzPileup, COHORT_SITE_DTYPE, RlzCohort, CHAIN_ANCHOR_DTYPE, CHAIN_DTYPE, HIT_DTYPE, RLZ_DTYPE, SEED_DTYPE, REPEAT_DTYPE, TARGET_HIT_DTYPE, RlzArchive, RlzArchiveFinder, RlzIndex, plan_index_batches, rebase, rlz_count_factors, rlz_decode, rlz_factorize,  # noqa: F401
                                     rlz_factorize_fasta, rlz_literals, rlz_summary, split_and_rebase, cigar_string,
                                     write_packed_archive, read_packed_archive)

__all__ = ["RLZ_DTYPE", "HIT_DTYPE", "SEED_DTYPE", "REPEAT_DTYPE", "CHAIN_DTYPE", "CHAIN_ANCHOR_DTYPE", "ALIGN_DTYPE", "VARIANT_DTYPE", "INSERTION_DTYPE", "insertion_bases", "PILEUP_CHANNELS", "RlzPileup", "COHORT_SITE_DTYPE", "RlzCohort", "cigar_string", "TARGET_HIT_DTYPE", "RlzArchiveFinder", "split_and_rebase", "rebase", "rlz_factorize", "rlz_count_factors", "rlz_factorize_fasta",
           "rlz_summary", "rlz_literals", "rlz_decode", "RlzArchive", "RlzIndex", "plan_index_batches", "write_packed_archive", "read_packed_archive"]
