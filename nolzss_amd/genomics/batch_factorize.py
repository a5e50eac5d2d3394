"""Per-sequence complexity table (reference: src/noLZSS/genomics/batch_factorize.py:370-461).

For every FASTA record: (id, full header, length, count_factors_dna_w_rc(seq), count_factors(seq)).  The reference
runs two complete factorizations per record in a CPU process pool; here both counts of every record come from ONE
GPU pipeline run per batch of records (_noLZSS.count_factors_batch_both: the plain-mode L* is a by-product of the
reverse-complement run over the same suffix array, DESIGN.md "Both counts from one suffix sort").

Only the two table functions are mirrored; downloads, gzip, shuffling, the CLI and the LSF driver are not.
"""
from pathlib import Path
from typing import Callable, Dict, List, Optional, Sequence, Tuple, Union

from .. import _noLZSS
from .fasta import _parse_fasta_content

Row = Tuple[str, str, int, int, int]
# counts(records) -> (counts_w_rc, counts_no_rc), one entry per record bytes object
CountsFn = Callable[[Sequence[bytes]], Tuple[Sequence[int], Sequence[int]]]

TSV_HEADER = "sequence_id\theader\tlength\tcomplexity_w_rc\tcomplexity_no_rc\n"


def _header_map(content: str) -> Dict[str, str]:
    """{id: full header} the reference's way (:407-414): lines split on '\\n', a '>' in column 0, the last header
    line of an id wins."""
    headers = {}
    for line in content.split("\n"):
        if line.startswith(">"):
            full_header = line[1:].strip()
            seq_id = full_header.split()[0] if full_header else full_header
            headers[seq_id] = full_header
    return headers


def _complexity_rows(sequences: Dict[str, str], headers: Dict[str, str], counts: CountsFn) -> List[Row]:
    """The table rows for parsed records ({id: sequence} in first-appearance order of the ids).  Errors as in the
    reference, whose pool raises the first failing record in file order (:376-381): a record with non-ASCII text
    fails as seq.encode('ascii') does, one with another letter as count_factors_dna_w_rc does on it."""
    ids = list(sequences)
    records: List[bytes] = []
    encode_error = None
    for seq_id in ids:
        try:
            records.append(sequences[seq_id].encode("ascii"))
        except UnicodeEncodeError as e:
            encode_error = e
            break
    # (the records in front of a non-ASCII one are counted first: an invalid letter there comes first in file order)
    w_rc, no_rc = counts(records) if records else ([], [])
    if encode_error is not None:
        raise encode_error
    return [(seq_id, headers.get(seq_id, seq_id), len(sequences[seq_id]), int(a), int(b))
            for seq_id, a, b in zip(ids, w_rc, no_rc)]


def _table_from_content(content: str, counts: CountsFn) -> List[Row]:
    sequences = _parse_fasta_content(content)  # (parse errors before any count)
    return _complexity_rows(sequences, _header_map(content), counts)


def _write_tsv(rows: Sequence[Row], output_path: Union[str, Path]) -> int:
    output_path = Path(output_path)
    output_path.parent.mkdir(parents=True, exist_ok=True)
    with open(output_path, "w", encoding="utf-8") as f:
        f.write(TSV_HEADER)
        for seq_id, full_header, length, count_w_rc, count_no_rc in rows:
            f.write(f"{seq_id}\t{full_header}\t{length}\t{count_w_rc}\t{count_no_rc}\n")
    return len(rows)


def _device_counts(devices: Optional[Sequence[int]]) -> CountsFn:
    return lambda records: _noLZSS.count_factors_batch_both(records, devices=devices)


def compute_sequence_complexity_table(fasta_path: Union[str, Path], num_processes: Optional[int] = None,
                                      devices: Optional[Sequence[int]] = None) -> List[Row]:
    """reference: batch_factorize.py:391-429 -> [(sequence_id, full_header, length, complexity_w_rc,
    complexity_no_rc)].  num_processes is accepted and ignored (the records are dealt over `devices`, default: the
    current device)."""
    del num_processes
    with open(Path(fasta_path), "r", encoding="utf-8") as f:
        content = f.read()
    return _table_from_content(content, _device_counts(devices))


def write_sequence_complexity_tsv(fasta_path: Union[str, Path], output_path: Union[str, Path],
                                  num_processes: Optional[int] = None,
                                  devices: Optional[Sequence[int]] = None) -> int:
    """reference: batch_factorize.py:432-461: the table as TSV (parent directories created); returns the row
    count."""
    output_path = Path(output_path)
    output_path.parent.mkdir(parents=True, exist_ok=True)
    return _write_tsv(compute_sequence_complexity_table(fasta_path, num_processes, devices=devices), output_path)


__all__ = ["compute_sequence_complexity_table", "write_sequence_complexity_tsv"]
