#!/usr/bin/env python3
"""Pins the per-sequence complexity table to what the reference's own Python code produces.

Build container only (never on the GPU box, which has no /root/reference): the reference's `noLZSS` package is
loaded by path under a private name with a stub compiled module `_noLZSS` -- `count_factors` and
`count_factors_dna_w_rc` come from the oracle (tests/oracle_lib.py), the stub's `count_factors_dna_w_rc` raises
RcCountMarker on a byte other than A/C/G/T, every other imported name is a no-op -- and its
`compute_sequence_complexity_table(path, num_processes=1)` and `write_sequence_complexity_tsv` run on a table of
FASTA texts.  tests/golden/python_ref_complexity.json records each input and then the rows or the exception class
and message, and the TSV bytes.  Inputs and observed outputs only: nothing of the reference's text is copied.

tests/test_complexity_host.py (CPU suite) replays the entries through nolzss_amd.genomics.batch_factorize with the
oracle as the counts callable.

    python tests/golden/make_complexity_fixtures.py      (rewrites tests/golden/python_ref_complexity.json)
"""
import importlib.util
import json
import sys
import tempfile
import types
from pathlib import Path

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT / "tests"))
import oracle_lib as oracle  # noqa: E402

REF_PKG = Path("/root/reference/src/noLZSS")
OUT = Path(__file__).resolve().parent / "python_ref_complexity.json"
PRIVATE = "_reference_noLZSS"

CASES = [
    ("duplicate_ids", ">a first\nACGTACGT\n>b\nTTTT\n>a second copy\nGGGACGTCCC\n"),
    ("header_with_leading_blanks", "  >lead desc\nACGTTGCA\n>c\nAAAAAAAA\n>  spaced id here\nGATTACA\n"),
    ("crlf", ">x one\r\nACGTAC\r\nGTACGT\r\n>y two\r\nCCCCGGGG\r\n"),
    ("empty_record", ">e\n>f desc\nACGTTTACG\n"),
    ("lower_case", ">l\nacgtacgtAC\nggcc\n"),
    ("n_in_second_of_three", ">r1\nACGTACGT\n>r2\nACGNACGT\n>r3\nTTTTGGGG\n"),
    ("empty_header", ">\nACGT\n"),
    ("data_before_first_header", "ACGT\n>a\nACGT\n"),
    ("headers_only", ">h1 one\n>h2 two\n"),
    ("descriptions_with_tabs", ">t1\tdesc\twith tabs\nATGCAT\n>t2 x\ty\nGATTACAGATTACA\n"),
    ("non_ascii_in_second", ">u\nACGTAA\n>v\nAC\u00e9T\n>w\nACGN\n"),
    ("n_before_non_ascii", ">u\nACGTAA\n>v\nACNT\n>w\nAC\u00e9T\n"),
]


class RcCountMarker(Exception):
    """the stub's count_factors_dna_w_rc met a byte other than A/C/G/T (message: the record's bytes, hex)"""


def _count_factors(data):
    return oracle.count_factors(bytes(data))


def _count_factors_dna_w_rc(data):
    data = bytes(data)
    if any(c not in b"ACGT" for c in data):
        raise RcCountMarker(data.hex())
    if not data:
        return 0
    S, _, _ = oracle.prepare_multiple_dna_w_rc([data])
    return oracle.count_factors_multiple_dna_w_rc(S)


def _noop(*args, **kwargs):
    return None


def load_reference_package():
    stub = types.ModuleType(PRIVATE + "._noLZSS")
    stub.__version__ = "0.0.0-stub"
    stub.count_factors = _count_factors
    stub.count_factors_dna_w_rc = _count_factors_dna_w_rc
    stub.RcCountMarker = RcCountMarker
    stub.__getattr__ = lambda name: _noop  # every other name the package imports
    sys.modules[PRIVATE + "._noLZSS"] = stub
    spec = importlib.util.spec_from_file_location(PRIVATE, REF_PKG / "__init__.py",
                                                  submodule_search_locations=[str(REF_PKG)])
    pkg = importlib.util.module_from_spec(spec)
    sys.modules[PRIVATE] = pkg
    spec.loader.exec_module(pkg)
    return importlib.import_module(PRIVATE + ".genomics.batch_factorize")


def outcome(fn):
    try:
        return {"ok": fn()}
    except Exception as e:  # noqa: BLE001  (the class is what is recorded)
        return {"exc": type(e).__name__, "msg": str(e)}


def main():
    # (the stub's marker class must be the one the pool's workers raise: registered under the stub's name)
    RcCountMarker.__module__ = PRIVATE + "._noLZSS"
    bf = load_reference_package()
    fx = {"_how": "tests/golden/make_complexity_fixtures.py: the reference's noLZSS package loaded by path with a "
                  "stub compiled module whose counts come from the oracle; inputs and observed outputs only",
          "marker": "RcCountMarker", "cases": []}
    with tempfile.TemporaryDirectory() as td:
        for name, text in CASES:
            path = Path(td) / (name + ".fa")
            path.write_bytes(text.encode("utf-8"))  # (\r\n kept as written)
            rows = outcome(lambda: [list(r) for r in bf.compute_sequence_complexity_table(path, num_processes=1)])
            tsv_path = Path(td) / "out" / "sub" / (name + ".tsv")
            written = outcome(lambda: bf.write_sequence_complexity_tsv(path, tsv_path, num_processes=1))
            entry = {"name": name, "fasta_hex": text.encode("utf-8").hex(), "rows": rows, "tsv_written": written,
                     "tsv_hex": tsv_path.read_bytes().hex() if tsv_path.exists() else None}
            fx["cases"].append(entry)
            print(name, rows, written)
    OUT.write_text(json.dumps(fx, indent=1, ensure_ascii=True) + "\n")
    print(f"wrote {OUT}: {len(fx['cases'])} cases")


if __name__ == "__main__":
    sys.exit(main())
