"""CPU: nolzss_amd.genomics.significance against what the reference's own Python code produced on the same inputs
(tests/golden/python_ref_significance.json, written by tests/golden/make_significance_fixtures.py), with exact float
equality; and the host restatement of the keyed shuffle (tests/shuffle_ref.py)."""
import json
import warnings
from pathlib import Path

import numpy as np
import pytest

import shuffle_ref

FIXTURES = json.loads((Path(__file__).resolve().parent / "golden" / "python_ref_significance.json").read_text())
P_AT = FIXTURES["p_at"]


@pytest.fixture(scope="module")
def sig():
    from nolzss_amd.genomics import significance
    return significance


def _arg(x):
    if isinstance(x, str) and x.startswith("np:"):
        return np.array(json.loads(x[3:]), dtype=np.int64)
    return x


def _plain(v):
    if isinstance(v, np.ndarray):
        return v.tolist()
    if isinstance(v, np.integer):
        return int(v)
    if isinstance(v, np.floating):
        return float(v)
    return v


def run(fn, post, tmp=None):
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        try:
            res = {"ok": post(fn())}
        except Exception as e:  # noqa: BLE001
            msg = str(e)
            if tmp:
                msg = msg.replace(str(tmp), "{path}")
            res = {"exc": type(e).__name__, "msg": msg}
    res["warnings"] = [[c.category.__name__, str(c.message)] for c in w]
    return res


def infer_fields(r):
    out = {k: _plain(v) for k, v in r.items() if k != "p_any_ge"}
    out["p_any_ge"] = [float(r["p_any_ge"](L)) for L in P_AT]
    return out


def expect(entry):
    return {k: entry[k] for k in ("ok", "exc", "msg", "warnings") if k in entry}


def test_reference_names_reexported():
    import noLZSS.genomics as g
    import noLZSS.genomics.significance as s
    for name in ("clopper_pearson_upper", "extract_factor_lengths", "infer_length_significance",
                 "calculate_factor_length_threshold"):
        assert getattr(g, name) is getattr(s, name)
    assert not hasattr(s, "plot_significance_analysis")


@pytest.mark.parametrize("entry", FIXTURES["clopper_pearson_upper"], ids=lambda e: f"{e['k']}-{e['n']}-{e['alpha']}")
def test_clopper_pearson_upper(sig, entry):
    assert run(lambda: sig.clopper_pearson_upper(entry["k"], entry["n"], entry["alpha"]), float) == expect(entry)


@pytest.mark.parametrize("entry", FIXTURES["infer"], ids=lambda e: e["name"])
def test_infer_length_significance(sig, entry):
    got = run(lambda: sig.infer_length_significance(_arg(entry["real"]), _arg(entry["shuf"]), **entry["kwargs"]),
              infer_fields)
    assert got == expect(entry)
    if "ok" in got:
        assert list(got["ok"]) == list(entry["ok"])  # key order too


@pytest.mark.parametrize("entry", FIXTURES["extract_lists"], ids=lambda e: e["name"])
def test_extract_factor_lengths_lists(sig, entry):
    facs = [f["list"] if isinstance(f, dict) else tuple(f) for f in entry["factors"]]
    got = run(lambda: sig.extract_factor_lengths(facs), _plain)
    assert got == expect(entry)
    if "ok" in got:
        assert sig.extract_factor_lengths(facs).dtype == np.int64


@pytest.mark.parametrize("entry", FIXTURES["extract_other"], ids=lambda e: e["name"])
def test_extract_factor_lengths_other(sig, entry):
    v = {"int": 5, "tuple": ((0, 1, 0),), "none": None}[entry["name"]]
    assert run(lambda: sig.extract_factor_lengths(v), _plain) == expect(entry)


@pytest.fixture()
def files(tmp_path):
    for name, data in FIXTURES["files"].items():
        (tmp_path / (name + ".bin")).write_bytes(bytes.fromhex(data))
    return tmp_path


@pytest.mark.parametrize("entry", FIXTURES["extract_files"], ids=lambda e: e["file"] + ("-path" if e.get("as_path") else ""))
def test_extract_factor_lengths_files(sig, files, entry):
    p = files / (entry["file"] + ".bin")
    got = run(lambda: sig.extract_factor_lengths(p if entry.get("as_path") else str(p)), _plain, files)
    assert got == expect(entry)
    if "ok" in got:
        assert sig.extract_factor_lengths(str(p)).dtype == np.int64


@pytest.mark.parametrize("entry", FIXTURES["threshold"], ids=lambda e: f"{e['real']}-{e['shuf']}-{len(e['kwargs'])}")
def test_calculate_factor_length_threshold(sig, files, entry):
    got = run(lambda: sig.calculate_factor_length_threshold(str(files / (entry["real"] + ".bin")),
                                                            str(files / (entry["shuf"] + ".bin")), **entry["kwargs"]),
              infer_fields, files)
    assert got == expect(entry)


def test_plot_output_refused(sig, files):
    with pytest.raises(ValueError, match="plots are not part of this package"):
        sig.calculate_factor_length_threshold(str(files / "small.bin"), str(files / "shuf_small.bin"),
                                              plot_output=str(files / "plot.png"))


def test_wilson_fallback_without_scipy(sig, monkeypatch):
    import builtins
    real_import = builtins.__import__

    def no_scipy(name, *a, **k):
        if name.startswith("scipy"):
            raise ImportError("no scipy")
        return real_import(name, *a, **k)

    monkeypatch.setattr(builtins, "__import__", no_scipy)
    with pytest.warns(UserWarning, match="scipy not available"):
        v = sig.clopper_pearson_upper(5, 100, 0.05)
    p, z = 0.05, 1.645
    d = 1 + z**2 / 100
    assert v == float(min((p + z**2 / 200) / d + z * np.sqrt(p * (1 - p) / 100 + z**2 / 40000) / d, 1.0))
    with pytest.raises(ValueError, match="Wilson score fallback only supports"):
        sig.clopper_pearson_upper(5, 100, 0.1)


def test_histogram_statistics_match_lengths(sig):
    """the statistics from a device-style histogram (dense bins + tail) equal those of infer_length_significance on
    the lengths themselves, field by field"""
    rng = np.random.default_rng(5)
    shuf = rng.geometric(0.1, 3000)
    shuf[:3] = [5000, 7000, 5000]
    real = rng.geometric(0.07, 2000)
    real[:2] = [6000, 9000]
    big = shuf >= 2048
    hist = {"fwd": np.bincount(shuf[~big], minlength=2048)[:2048], "rc": np.zeros(2048, np.int64),
            "tail_lengths": shuf[big], "tail_rc": np.zeros(int(big.sum()), bool)}
    hist["rc"][:3], hist["fwd"][:3] = hist["fwd"][:3], 0  # (the strands are summed: any split counts the same)
    vals, counts = sig.hist_values_counts(hist)
    u, c = np.unique(shuf, return_counts=True)
    assert vals.tolist() == u.tolist() and counts.tolist() == c.tolist()
    for kw in ({}, {"tau_expected_fp": 0.5, "alpha_cp": 0.01}):
        got = sig._significance(real.astype(np.uint32), vals, counts, kw.get("tau_expected_fp", 1.0),
                                kw.get("alpha_cp", 0.05))
        exp = sig.infer_length_significance(real, shuf, **kw)
        assert list(got) == list(exp)
        for k in ("N_real", "N_shuf", "L_star", "tau_expected_fp", "alpha_cp"):
            assert got[k] == exp[k], k
        for k in ("rarity_scores_real", "uniq_L", "S0", "S0_upper", "expected_fp_upper"):
            assert np.array_equal(got[k], exp[k]) and got[k].dtype == exp[k].dtype, k
        for L in P_AT:
            assert got["p_any_ge"](L) == exp["p_any_ge"](L)


@pytest.mark.parametrize("seed", [-1, 1 << 64, 1.5, "3"])
def test_seed_out_of_range_refused(seed):
    """the shuffle key is a uint64_t: nothing wraps silently (checked before any device work)"""
    from nolzss_amd import _noLZSS
    from nolzss_amd.genomics import significance
    err = ValueError if isinstance(seed, int) else TypeError
    for call in (lambda: _noLZSS.shuffle_dna(b"ACGT", seed),
                 lambda: _noLZSS.factor_length_histogram(b"ACGT", shuffle_seed=seed),
                 lambda: _noLZSS.fasta_factor_length_histogram("missing.fa", shuffle_seed=seed),
                 lambda: _noLZSS.fasta_shuffled_text("missing.fa", seed),
                 lambda: significance.shuffled_control_significance(b"ACGT", seed=seed)):
        with pytest.raises(err):
            call()


def test_sanitize_mode_refused_by_the_c_abi(tmp_path):
    """the FASTA entry points refuse what nolzss_factorize_fasta_multiple_dna refuses (before any device work)"""
    import ctypes as C
    from nolzss_amd import _lib
    path = tmp_path / "a.fa"
    path.write_bytes(b">a\nACGT\n")
    for mode in (2, -1):
        res = _lib.LengthHist()
        assert _lib.lib.nolzss_fasta_factor_length_histogram(str(path).encode(), 1, mode, 0, 0, 0,
                                                              C.byref(res)) == _lib.ERR_INVALID_ARGUMENT
        assert _lib.lib.nolzss_last_error() == b"sanitize_mode must be 0 or 1"
        assert _lib.lib.nolzss_fasta_factor_length_histogram_with_lengths(str(path).encode(), 0, mode, 0,
                                                                           C.byref(res)) == _lib.ERR_INVALID_ARGUMENT
        S, n = C.c_void_p(), C.c_size_t()
        assert _lib.lib.nolzss_fasta_shuffled_text(str(path).encode(), 1, mode, 0, 0, C.byref(S),
                                                   C.byref(n)) == _lib.ERR_INVALID_ARGUMENT
        assert _lib.lib.nolzss_last_error() == b"sanitize_mode must be 0 or 1"


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 15, 16, 17, 1000, 63, 65, 255, 257, 4095, 4097, 65535, 65537])
def test_shuffle_permutation_is_bijection(n):
    for seed in (0, 1, 0xFFFFFFFFFFFFFFFF):
        p = shuffle_ref.permutation(n, seed)
        assert sorted(p.tolist()) == list(range(n))


def test_shuffle_keys_change_permutation():
    n = 1000
    base = shuffle_ref.permutation(n, 7, 0)
    assert not np.array_equal(base, shuffle_ref.permutation(n, 8, 0))
    assert not np.array_equal(base, shuffle_ref.permutation(n, 7, 1))
    assert np.array_equal(base, shuffle_ref.permutation(n, 7, 0))
    assert not np.array_equal(base, np.arange(n))
