"""CPU: the per-sequence complexity table (nolzss_amd.genomics.batch_factorize) against what the reference's own
Python code produced on the same FASTA texts (tests/golden/python_ref_complexity.json, written by
tests/golden/make_complexity_fixtures.py).  The counts come from the oracle through the row builder's counts
callable, so rows, errors and TSV bytes are checked without a GPU."""
import json
from pathlib import Path

import pytest

import oracle_lib as oracle

FIXTURES = json.loads((Path(__file__).resolve().parent / "golden" / "python_ref_complexity.json").read_text())
CASES = {c["name"]: c for c in FIXTURES["cases"]}


class RcCountMarker(Exception):
    """the RC count met a byte other than A/C/G/T (args: the record's bytes, hex), as the fixture's stub raised"""


def oracle_rc_count(record: bytes) -> int:
    if not record:
        return 0
    S, _, _ = oracle.prepare_multiple_dna_w_rc([record])
    return oracle.count_factors_multiple_dna_w_rc(S)


def oracle_counts(records):
    """the counts callable: record by record as the reference's pool does (RC count first)"""
    w_rc, no_rc = [], []
    for r in records:
        r = bytes(r)
        if any(c not in b"ACGT" for c in r):
            raise RcCountMarker(r.hex())
        w_rc.append(oracle_rc_count(r))
        no_rc.append(oracle.count_factors(r))
    return w_rc, no_rc


def _write_fasta(tmp_path, case):
    path = tmp_path / (case["name"] + ".fa")
    path.write_bytes(bytes.fromhex(case["fasta_hex"]))
    return path


def _table(path):
    from nolzss_amd.genomics import batch_factorize as bf
    with open(path, "r", encoding="utf-8") as f:
        content = f.read()
    return bf._table_from_content(content, oracle_counts)


@pytest.mark.parametrize("name", sorted(CASES))
def test_rows_match_reference(name, tmp_path):
    case = CASES[name]
    path = _write_fasta(tmp_path, case)
    exp = case["rows"]
    if "ok" in exp:
        assert [list(r) for r in _table(path)] == exp["ok"]
        return
    if exp["exc"] == FIXTURES["marker"]:
        # the error comes from the RC count, of the record the reference's pool failed on first
        with pytest.raises(RcCountMarker) as ei:
            _table(path)
        assert ei.value.args[0] == exp["msg"]
        return
    with pytest.raises(Exception) as ei:
        _table(path)
    assert type(ei.value).__name__ == exp["exc"]
    assert str(ei.value) == exp["msg"]


@pytest.mark.parametrize("name", sorted(CASES))
def test_tsv_bytes_match_reference(name, tmp_path, monkeypatch):
    from nolzss_amd.genomics import batch_factorize as bf
    case = CASES[name]
    path = _write_fasta(tmp_path, case)
    out = tmp_path / "new" / "dir" / (name + ".tsv")
    # the public writer with the oracle in place of the device counts
    monkeypatch.setattr(bf, "_device_counts", lambda devices: oracle_counts)
    exp = case["tsv_written"]
    if "ok" in exp:
        assert bf.write_sequence_complexity_tsv(path, out, num_processes=3) == exp["ok"]
        assert out.read_bytes() == bytes.fromhex(case["tsv_hex"])
        return
    with pytest.raises(RcCountMarker if exp["exc"] == FIXTURES["marker"] else Exception) as ei:
        bf.write_sequence_complexity_tsv(path, out)
    if exp["exc"] != FIXTURES["marker"]:
        assert type(ei.value).__name__ == exp["exc"] and str(ei.value) == exp["msg"]
    assert not out.exists() and case["tsv_hex"] is None


def test_fixture_table_covers_the_issue_inputs():
    assert {"duplicate_ids", "header_with_leading_blanks", "crlf", "empty_record", "lower_case", "n_in_second_of_three",
            "empty_header", "data_before_first_header", "headers_only", "descriptions_with_tabs"} <= set(CASES)


def test_reference_import_path_reexports_the_table():
    import noLZSS.genomics.batch_factorize as ref_path
    from nolzss_amd.genomics import batch_factorize as bf
    assert ref_path.compute_sequence_complexity_table is bf.compute_sequence_complexity_table
    assert ref_path.write_sequence_complexity_tsv is bf.write_sequence_complexity_tsv


def test_batch_both_entry_point_is_declared():
    from nolzss_amd import _lib, _noLZSS
    assert "nolzss_count_factors_batch_both" in _lib.EXPORTED_SYMBOLS
    assert _noLZSS.count_factors_batch_both([]) == ([], [])  # (no record: no device touched)
