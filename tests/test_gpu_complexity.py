"""GPU: both factor counts of every record from one suffix sort (nolzss_count_factors_batch_both) and the
per-sequence complexity table built on it (nolzss_amd.genomics.batch_factorize).  Every count is compared with the
oracle, not with the GPU alone."""
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import gen
import genomes
import oracle_lib as oracle

pytestmark = pytest.mark.gpu

KATS = json.loads((Path(__file__).resolve().parent / "golden" / "kats.json").read_text())
_CACHE = {}


@pytest.fixture(scope="module")
def native():
    from nolzss_amd import _noLZSS
    assert _noLZSS.device_count() >= 1, "no MI355X visible"
    return _noLZSS


def oracle_pair(record: bytes):
    """(count_factors_dna_w_rc, count_factors) of one record on the CPU oracle, cached per record"""
    key = (len(record), hash(record))
    if key not in _CACHE:
        if not record:
            _CACHE[key] = (0, 0)
        else:
            S, _, _ = oracle.prepare_multiple_dna_w_rc([record])
            _CACHE[key] = (oracle.count_factors_multiple_dna_w_rc(S), oracle.count_factors(record))
    return _CACHE[key]


def _expect(records):
    pairs = [oracle_pair(r) for r in records]
    return [p[0] for p in pairs], [p[1] for p in pairs]


def _kat_inputs():
    out = []
    for group in ("plain", "dna_w_rc", "dna_w_rc_partial"):
        for k in KATS[group]:
            if isinstance(k.get("input"), str):
                out.append(k["input"].encode("latin-1"))
    return out


def test_kats_and_atgcat(native):
    kats = _kat_inputs()
    assert len(kats) >= 5
    texts = [t for t in kats if all(c in b"ACGT" for c in t)] + [b"ATGCAT", b"A", b"AC", b"ACGT" * 9]
    # the other KAT inputs: refused as count_factors_dna_w_rc refuses them, lower-case DNA refused on its own
    for t in kats:
        if t in texts:
            continue
        try:
            native.count_factors_dna_w_rc(t)
        except RuntimeError as e:
            with pytest.raises(RuntimeError) as ei:
                native.count_factors_batch_both([b"ACGT", t])
            assert str(ei.value) == str(e)
        else:
            with pytest.raises(ValueError, match="lower-case"):
                native.count_factors_batch_both([t])
    w_rc, no_rc = native.count_factors_batch_both(texts)
    assert (w_rc, no_rc) == _expect(texts)
    i = texts.index(b"ATGCAT")
    assert w_rc[i] != no_rc[i]  # (the RC count differs from the plain one there)
    for t in texts:  # one by one: single-record runs
        assert native.count_factors_batch_both([t]) == ([oracle_pair(t)[0]], [oracle_pair(t)[1]])


_far_copy = gen.far_copy


@pytest.fixture(scope="module")
def mixed_records():
    rng = np.random.default_rng(0xC0DE)
    recs = [b"", b"A", b"GT"]
    for k, n in enumerate([(1 << 21) - 1, 1 << 21, (1 << 21) + 1]):  # around the merge threshold
        recs.append((gen.repeat_dna(n, seed=100 + k) if k % 2 else gen.random_dna(n, 100 + k)).tobytes())
    recs.append(gen.repeat_dna((1 << 23) + 5, seed=7).tobytes())  # compact permutation
    recs.append(gen.repeat_dna(3 << 20, seed=8).tobytes())  # between 2^21 and 2^22 bases: not compact
    recs += [b"A" * 70_000, b"AC" * 40_000, b"A" * 3000, b"ACG" * 5000]  # the exact queue
    recs += [_far_copy(600_000, 9), _far_copy(150_000, 10)]  # the far queue
    while len(recs) < 200:
        n = int(np.exp(rng.uniform(np.log(8), np.log(40_000))))
        s = int(rng.integers(0, 1 << 30))
        recs.append((gen.repeat_dna(n, seed=s, lo=16, hi=4096) if rng.random() < 0.5 else gen.random_dna(n, s)).tobytes())
    order = rng.permutation(len(recs))
    return [recs[j] for j in order]


def test_mixed_batch_matches_oracle(native, mixed_records):
    exp = _expect(mixed_records)
    assert native.count_factors_batch_both(mixed_records) == exp
    # one by one through the two calls the table replaces: equal
    assert [native.count_factors_dna_w_rc(r) for r in mixed_records] == exp[0]
    assert [native.count_factors(r) for r in mixed_records] == exp[1]


def test_mixed_batch_long_records_one_run_each(native, mixed_records, monkeypatch):
    # (long records as single pipeline runs: the 2^23 + 5 record compact, the 3 * 2^20 one not)
    monkeypatch.setenv("NOLZSS_BATCH_MERGE_LONG_BELOW", "0")
    assert native.count_factors_batch_both(mixed_records) == _expect(mixed_records)


def test_mixed_batch_two_device_lanes(native, mixed_records):
    assert native.count_factors_batch_both(mixed_records, devices=[0, 0]) == _expect(mixed_records)


def test_invalid_nucleotide_first_record_in_input_order(native):
    recs = [b"ACGTACGT", b"ACGTNACG", b"ACGT", b"ACGRACGT", b"GATTACA"]
    with pytest.raises(RuntimeError) as single:
        native.count_factors_dna_w_rc(recs[1])
    with pytest.raises(RuntimeError) as both:
        native.count_factors_batch_both(recs)
    assert str(both.value) == str(single.value) and "'N'" in str(both.value)
    big = [gen.random_dna(3 << 20, 1).tobytes(), b"AC" * 10 + b"*" + b"AC", b"ACGTN"]  # a long record in front
    with pytest.raises(RuntimeError, match="Invalid nucleotide '\\*' found in sequence 0"):
        native.count_factors_batch_both(big)


def test_lower_case_refused(native):
    with pytest.raises(ValueError, match="lower-case"):
        native.count_factors_batch_both([b"ACGT", b"acgt"])
    # an invalid letter in a later record still wins: the reverse-complement count refuses it on its own
    with pytest.raises(RuntimeError, match="Invalid nucleotide 'N'"):
        native.count_factors_batch_both([b"acgt", b"ANA"])


def test_one_suffix_sort(native):
    rec = gen.repeat_dna(1 << 23, seed=11).tobytes()
    native.profile_enable(True)
    try:
        native.profile_reset()
        z_rc = native.count_factors_dna_w_rc(rec)
        sorts_rc = native.profile_report()["sa_sort_initial"][0]
        native.profile_reset()
        both = native.count_factors_batch_both([rec])
        rep = native.profile_report()
    finally:
        native.profile_enable(False)
    assert both == ([z_rc], [oracle_pair(rec)[1]]) and z_rc == oracle_pair(rec)[0]
    assert rep["sa_sort_initial"][0] == sorts_rc
    assert "rc_plain_gather" in rep and "plain_chain" in rep


_ARENA_CHILD = """
import sys
import gen
from nolzss_amd import _noLZSS as native
rec = gen.repeat_dna((1 << 23) + 5, seed=7).tobytes()
z = native.count_factors_batch_both([rec]) if sys.argv[1] == "both" else native.count_factors_dna_w_rc(rec)
print(native.debug_arena()[1])
"""


def test_arena_high_water_at_the_largest_rc_size(native):
    # fresh processes: the high-water mark of an arena is kept for its lifetime
    here = Path(__file__).resolve().parent
    peaks = {}
    for mode in ("rc", "both"):
        r = subprocess.run([sys.executable, "-c", _ARENA_CHILD, mode], cwd=here, capture_output=True, text=True,
                           timeout=300, env={**os.environ,
                                             "PYTHONPATH": f"{here.parent}:{here}"})
        assert r.returncode == 0, r.stderr[-2000:]
        peaks[mode] = int(r.stdout.split()[-1])
    n = (1 << 23) + 5
    # the plain by-product adds at most what the reservation adds for it (dna_w_rc_common: 4 n + 32 MiB)
    assert peaks["rc"] <= peaks["both"] <= peaks["rc"] + 4 * n + (32 << 20), peaks


@pytest.mark.parametrize("import_path", ["nolzss_amd.genomics.batch_factorize", "noLZSS.genomics.batch_factorize"])
def test_table_on_golden_genomes(native, import_path, tmp_path):
    import importlib
    bf = importlib.import_module(import_path)
    for name in ["Vibrio_cholerae", "test_bacterial_dna", "test_viral_dna", "T3"]:
        path = genomes.materialize(name, tmp_path)
        rows = bf.compute_sequence_complexity_table(path, num_processes=4)
        recs = genomes.records(name)
        assert [r[0] for r in rows] == [rid for rid, _ in recs]
        for (rid, seq), row in zip(recs, rows):
            assert row[2] == len(seq)
            assert (row[3], row[4]) == oracle_pair(seq), (name, rid)
        out = tmp_path / "tsv" / (name + ".tsv")
        assert bf.write_sequence_complexity_tsv(path, out) == len(rows)
        lines = out.read_text().split("\n")
        assert lines[0] == "sequence_id\theader\tlength\tcomplexity_w_rc\tcomplexity_no_rc" and lines[-1] == ""
        back = [ln.split("\t") for ln in lines[1:-1]]
        assert [(b[0], b[1], int(b[2]), int(b[3]), int(b[4])) for b in back] == [tuple(r) for r in rows]
