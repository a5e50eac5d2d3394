"""GPU: factor-length histograms and lengths straight from the chain, the keyed shuffle, and the shuffled-control
significance built on them (nolzss_amd.genomics.significance).  The yardstick is the CPU oracle's factorization and
the host restatement of the shuffle (tests/shuffle_ref.py), never the GPU alone."""
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
import shuffle_ref

pytestmark = pytest.mark.gpu

KATS = json.loads((Path(__file__).resolve().parent / "golden" / "kats.json").read_text())
T = 2048
RC_MASK = np.uint64(1 << 63)


@pytest.fixture(scope="module")
def native():
    from nolzss_amd import _noLZSS
    assert _noLZSS.device_count() >= 1, "no MI355X visible"
    return _noLZSS


@pytest.fixture(scope="module")
def sig():
    from nolzss_amd.genomics import significance
    return significance


def oracle_lengths(text: bytes, with_rc: bool):
    """(lengths in factor order, reverse-complement flags) of the oracle's factorization of one text"""
    if with_rc:
        S, _, _ = oracle.prepare_multiple_dna_w_rc([text])
        return oracle_S_lengths(S, True)
    return oracle_S_lengths(text, False)


def oracle_S_lengths(S: bytes, with_rc: bool):
    f = oracle.factors_array_multiple_dna_w_rc(S) if with_rc else oracle.factors_array(S)
    return f["length"].astype(np.int64), (f["ref"] & RC_MASK) != 0


def expected_hist(lengths, is_rc):
    fwd = np.bincount(lengths[(lengths < T) & ~is_rc], minlength=T)[:T]
    rc = np.bincount(lengths[(lengths < T) & is_rc], minlength=T)[:T]
    big = lengths >= T
    tail = sorted(zip(is_rc[big].tolist(), lengths[big].tolist()))
    return fwd, rc, tail


def check_hist(h, lengths, is_rc, what=""):
    fwd, rc, tail = expected_hist(lengths, is_rc)
    assert h["threshold"] == T and h["z"] == len(lengths), what
    assert np.array_equal(h["fwd"], fwd), what
    assert np.array_equal(h["rc"], rc), what
    assert list(zip(h["tail_rc"].tolist(), h["tail_lengths"].tolist())) == tail, what
    # the reference's view of the same lengths: np.unique over all of them
    from nolzss_amd.genomics.significance import hist_values_counts
    v, c = hist_values_counts(h)
    u, uc = np.unique(lengths, return_counts=True)
    assert v.tolist() == u.tolist() and c.tolist() == uc.tolist(), what


def tail_text():
    """copies of at least T bases, one block over 2^16 and reverse-complement copies of 3000 and 2T bases: the tail
    path on both strands"""
    rng = np.random.default_rng(3)
    base = gen.random_dna(300_000, seed=21).tobytes()
    parts = [base[:100_000], base[5_000:5_000 + 70_000], base[100_000:150_000], base[20_000:20_000 + 3000],
             base[150_000:200_000], base[40_000:40_000 + T], base[200_000:210_000], base[60_000:60_000 + T - 1],
             genomes.revcomp(base[80_000:83_000]), base[210_000:220_000], genomes.revcomp(base[120_000:120_000 + 2 * T]),
             rng.choice(np.frombuffer(b"ACGT", np.uint8), 5000).astype(np.uint8).tobytes()]
    return b"".join(parts)


def dna_texts():
    kats = [k["input"].encode("latin-1") for g in ("plain", "dna_w_rc", "dna_w_rc_partial") for k in KATS[g]
            if isinstance(k.get("input"), str)]
    kats = [t for t in kats if t and all(c in b"ACGT" for c in t)]
    return [("kat%d" % i, t) for i, t in enumerate(kats)] + [
        ("atgcat", b"ATGCAT"), ("a", b"A"), ("acgt9", b"ACGT" * 9),
        ("random_2^20", gen.random_dna(1 << 20, seed=5).tobytes()),
        ("repeat_2^22", gen.repeat_dna(1 << 22, seed=9).tobytes()),
        ("tail", tail_text()),
    ]


def fasta_records(native, path):
    return [bytes(s) for _, s in native.debug_parse_fasta(path)]


@pytest.mark.parametrize("with_rc", [False, True])
def test_histogram_and_lengths_vs_oracle(native, with_rc):
    for name, text in dna_texts():
        lengths, is_rc = oracle_lengths(text, with_rc)
        h = native.factor_length_histogram(text, with_rc=with_rc)
        check_hist(h, lengths, is_rc, name)
        got = native.factor_lengths(text, with_rc=with_rc)
        assert got.dtype == np.uint32 and np.array_equal(got.astype(np.int64), lengths), name
        hl = native.factor_length_histogram_with_lengths(text, with_rc=with_rc)
        check_hist(hl, lengths, is_rc, name)
        assert np.array_equal(hl["lengths"].astype(np.int64), lengths), name
        if name == "tail":
            assert len(h["tail_lengths"]) >= 2 and h["tail_lengths"].max() > 1 << 16
            # reverse-complement factors of T bases or more: strand bit packed into the tail and unpacked again
            assert h["tail_rc"].sum() == (2 if with_rc else 0) == (is_rc & (lengths >= T)).sum()
            if with_rc:
                assert sorted(h["tail_lengths"][h["tail_rc"]].tolist()) == sorted(lengths[is_rc & (lengths >= T)].tolist())
        if with_rc and name == "repeat_2^22":
            assert is_rc.any() and h["rc"].sum() > 0


def test_histogram_plain_bytes(native):
    rng = np.random.default_rng(8)
    text = rng.integers(1, 256, 200_000, dtype=np.uint8).tobytes() + b"hello world " * 500
    lengths, is_rc = oracle_lengths(text, False)
    check_hist(native.factor_length_histogram(text), lengths, is_rc)
    assert np.array_equal(native.factor_lengths(text).astype(np.int64), lengths)


def test_golden_genomes(native):
    for name in ["test_viral_dna", "T3", "T7", "test_bacterial_dna"]:
        for rid, seq in genomes.records(name)[:2]:
            if not seq or not all(c in b"ACGT" for c in seq):
                continue
            for with_rc in (False, True):
                lengths, is_rc = oracle_lengths(seq, with_rc)
                check_hist(native.factor_length_histogram(seq, with_rc=with_rc), lengths, is_rc, (name, rid))


def test_rc_refusals_match_count(native):
    for bad in (b"ACGTNACGT", b"ACGxT"):
        with pytest.raises(RuntimeError) as e1:
            native.count_factors_dna_w_rc(bad)
        for call in (lambda: native.factor_length_histogram(bad, with_rc=True),
                     lambda: native.factor_length_histogram(bad, with_rc=True, shuffle_seed=3),
                     lambda: native.factor_lengths(bad, with_rc=True)):
            with pytest.raises(RuntimeError) as e2:
                call()
            assert str(e2.value) == str(e1.value)


@pytest.mark.parametrize("n", [1, 2, 1000, (1 << 20) + 7])
def test_shuffle_matches_host(native, n):
    text = gen.random_dna(n, seed=n).tobytes()
    for seed in (0, 12345, 0xFFFFFFFFFFFFFFFF):
        got = native.shuffle_dna(text, seed)
        assert got == shuffle_ref.shuffle_bytes(text, seed)
        assert sorted(got) == sorted(text)
        assert native.shuffle_dna(text, seed) == got


def test_shuffled_histogram_is_histogram_of_shuffle(native):
    text = gen.repeat_dna(1 << 20, seed=4).tobytes()
    for with_rc in (False, True):
        h = native.factor_length_histogram(text, with_rc=with_rc, shuffle_seed=99)
        lengths, is_rc = oracle_lengths(shuffle_ref.shuffle_bytes(text, 99), with_rc)
        check_hist(h, lengths, is_rc, with_rc)


def _write_fasta(tmp_path):
    recs = [("r1", gen.random_dna(30_000, seed=1).tobytes()),
            ("r2 desc", gen.repeat_dna(50_000, seed=2, lo=16, hi=4096).tobytes()),
            ("r3", b"ACGTNNACGTRYACGT" * 200),
            ("r4", b"GATTACA" * 3000)]
    path = tmp_path / "in.fa"
    gen.write_fasta(path, recs)
    return str(path)


@pytest.mark.parametrize("with_rc", [True, False])
def test_fasta_shuffled_text_is_prepare_of_shuffled_records(native, tmp_path, with_rc):
    path = _write_fasta(tmp_path)
    records = fasta_records(native, path)
    seed = 77
    shuffled = shuffle_ref.shuffle_records(records, seed)
    got = native.fasta_shuffled_text(path, seed, with_rc=with_rc)
    if with_rc:
        S, _, _ = oracle.prepare_multiple_dna_w_rc(shuffled)
    else:  # (the oracle has no no-rc prepare: the host-only one)
        S, _, _ = native.prepare_multiple_dna_sequences_no_rc_bytes(shuffled)
    assert got == S
    lengths, is_rc = oracle_S_lengths(S, with_rc)
    check_hist(native.fasta_factor_length_histogram(path, with_rc=with_rc, shuffle_seed=seed), lengths, is_rc)


def _assert_same_result(got, exp):
    for k in ("N_real", "N_shuf", "L_star", "tau_expected_fp", "alpha_cp"):
        assert got[k] == exp[k], k
    for k in ("rarity_scores_real", "uniq_L", "S0", "S0_upper", "expected_fp_upper"):
        assert np.array_equal(got[k], exp[k]), k
    for L in (1, 5, 12.5, 40, 1e6):
        assert got["p_any_ge"](L) == exp["p_any_ge"](L)


@pytest.mark.parametrize("with_rc", [False, True])
def test_shuffled_control_significance_end_to_end(native, sig, with_rc):
    text = gen.repeat_dna(1 << 19, seed=17, lo=32, hi=8192).tobytes()
    seed = 2024
    got = sig.shuffled_control_significance(text, with_rc=with_rc, seed=seed)
    real, _ = oracle_lengths(text, with_rc)
    shuf, _ = oracle_lengths(shuffle_ref.shuffle_bytes(text, seed), with_rc)
    _assert_same_result(got, sig.infer_length_significance(real, shuf))
    assert got["seed"] == seed and got["with_rc"] == with_rc
    assert got["real_hist"]["z"] == len(real) and got["shuf_hist"]["z"] == len(shuf)
    drawn = sig.shuffled_control_significance(text[:5000], with_rc=with_rc)
    assert isinstance(drawn["seed"], int) and 0 <= drawn["seed"] < 1 << 64


@pytest.mark.parametrize("with_rc", [True, False])
def test_fasta_shuffled_control_significance(native, sig, tmp_path, with_rc):
    path = _write_fasta(tmp_path)
    seed = 5
    got = sig.fasta_shuffled_control_significance(path, with_rc=with_rc, seed=seed, tau_expected_fp=0.5)
    records = fasta_records(native, path)
    prep = oracle.prepare_multiple_dna_w_rc if with_rc else native.prepare_multiple_dna_sequences_no_rc_bytes
    real, _ = oracle_S_lengths(prep(records)[0], with_rc)
    shuf, _ = oracle_S_lengths(prep(shuffle_ref.shuffle_records(records, seed))[0], with_rc)
    _assert_same_result(got, sig.infer_length_significance(real, shuf, tau_expected_fp=0.5))


def test_threshold_from_written_files(native, sig, tmp_path):
    text = gen.repeat_dna(200_000, seed=31, lo=16, hi=2048).tobytes()
    shuf_text = shuffle_ref.shuffle_bytes(text, 3)
    (tmp_path / "real.txt").write_bytes(text)
    (tmp_path / "shuf.txt").write_bytes(shuf_text)
    native.write_factors_binary_file(str(tmp_path / "real.txt"), str(tmp_path / "real.bin"))
    native.write_factors_binary_file(str(tmp_path / "shuf.txt"), str(tmp_path / "shuf.bin"))
    got = sig.calculate_factor_length_threshold(str(tmp_path / "real.bin"), str(tmp_path / "shuf.bin"))
    real, _ = oracle_lengths(text, False)
    shuf, _ = oracle_lengths(shuf_text, False)
    assert np.array_equal(sig.extract_factor_lengths(str(tmp_path / "real.bin")), real)
    _assert_same_result(got, sig.infer_length_significance(real, shuf))


_ARENA_CHILD = """
import sys
import gen
from nolzss_amd import _noLZSS as native
n = (1 << 26) + 3
text = gen.random_dna(n, seed=1).tobytes()
assert len(native.shuffle_dna(text, 9)) == n
print(native.debug_arena()[0])
"""


def test_shuffle_reserves_its_buffers_only(native):
    # a fresh process: the arena of a context only grows.  The shuffle needs its two byte buffers, not the
    # reservation of a factorization of the text (96 bytes per symbol)
    here = Path(__file__).resolve().parent
    r = subprocess.run([sys.executable, "-c", _ARENA_CHILD], cwd=here, capture_output=True, text=True, timeout=300,
                       env={**os.environ, "PYTHONPATH": f"{here.parent}:{here}"})
    assert r.returncode == 0, r.stderr[-2000:]
    n = (1 << 26) + 3
    assert int(r.stdout.split()[-1]) <= 2 * n + (80 << 20)
