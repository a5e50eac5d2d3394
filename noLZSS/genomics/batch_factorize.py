"""noLZSS.genomics.batch_factorize (reference: src/noLZSS/genomics/batch_factorize.py:370-461): the per-sequence
complexity table, both counts of every record from one GPU pipeline run."""
from nolzss_amd.genomics.batch_factorize import (compute_sequence_complexity_table,  # noqa: F401
                                                 write_sequence_complexity_tsv)

__all__ = ["compute_sequence_complexity_table", "write_sequence_complexity_tsv"]
