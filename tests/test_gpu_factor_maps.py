"""GPU: the strand-bias grid and the space-scale histogram binned on the device (nolzss_factor_maps_*,
nolzss_amd.genomics.plots).  The device integers must EQUAL those of the exact integer model
(tests/factor_maps_model.py), the counts those of numpy.histogram2d; the factors always come from the CPU oracle,
never from the device."""
import json
import os
from contextlib import contextmanager
from pathlib import Path

import numpy as np
import pytest

import factor_maps_model as model
import gen
import genomes
import oracle_lib as oracle

pytestmark = pytest.mark.gpu

GOLDEN = Path(__file__).resolve().parent / "golden"
KATS = json.loads((GOLDEN / "kats.json").read_text())
FX = json.loads((GOLDEN / "python_ref_factor_maps.json").read_text())
GRIDS = [(50, 50), (37, 64), (4096, 3)]


@pytest.fixture(scope="module")
def native():
    from nolzss_amd import _noLZSS
    assert _noLZSS.device_count() >= 1, "no MI355X visible"
    return _noLZSS


@pytest.fixture(scope="module")
def plots():
    from nolzss_amd.genomics import plots
    return plots


@contextmanager
def env(**kv):
    old = {k: os.environ.get(k) for k in kv}
    try:
        for k, v in kv.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = str(v)
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def both_forms(call):
    """the call with workgroup-private LDS accumulators (where they fit) and with the global form forced: equal"""
    with env(NOLZSS_FACTOR_MAPS_GLOBAL=None):
        a = call()
    with env(NOLZSS_FACTOR_MAPS_GLOBAL="1"):
        b = call()
    for k, v in a.items():
        if isinstance(v, np.ndarray):
            assert np.array_equal(v, b[k]), k
        else:
            assert v == b[k], k
    return a


def oracle_records(text: bytes, with_rc: bool):
    if with_rc:
        S, _, _ = oracle.prepare_multiple_dna_w_rc([text])
        f = oracle.factors_array_multiple_dna_w_rc(S)
    else:
        f = oracle.factors_array(text)
    return np.stack([f["start"], f["length"], f["ref"]], axis=1)


def check_grid(m, recs, grid, total, minlen=1, sentinels=(), what=""):
    xb, yb = grid
    s, l, r, is_rc = model.kept_factors(recs, minlen, sentinels)
    assert m["z"] == len(recs) and m["z_used"] == len(s), what
    assert m["kept_forward"] == int((~is_rc).sum()) and m["kept_rc"] == int(is_rc.sum()), what
    assert (m["x_bins"], m["y_bins"], m["unit"]) == (xb, yb, xb * yb), what
    if len(s) == 0:
        assert not m["forward_units"].any() and not m["rc_units"].any(), what
        return
    fw, rc, x_max, y_max = model.exact_grid_fast(s, l, r, is_rc, xb, yb, total)
    assert (m["x_max"], m["y_max"]) == (x_max, y_max), what
    assert m["forward_units"].dtype == np.uint64 and m["forward_units"].shape == (yb, xb), what
    assert np.array_equal(m["forward_units"], fw), what
    assert np.array_equal(m["rc_units"], rc), what
    assert (m["min_length"], m["max_length"], m["max_start"]) == (int(l.min()), int(l.max()), int(s.max())), what


def check_hist(m, recs, length_edges, position_edges, minlen=1, sentinels=(), what=""):
    s, l, _, is_rc = model.kept_factors(recs, minlen, sentinels)
    if position_edges is None:  # the reference's ladder, plots.py:2566-2574
        genome_end = int(s.max())
        nb = max(50, int(np.ceil(genome_end / 1_000_000)))
        position_edges = np.linspace(0, genome_end, nb + 1)
    assert m["position_edges"].tobytes() == np.asarray(position_edges, dtype=np.float64).tobytes(), what
    fw, rc = model.histogram(s, l, is_rc, length_edges, position_edges)
    assert m["hist_forward"].dtype == np.uint64 and m["hist_forward"].shape == fw.shape, what
    assert np.array_equal(m["hist_forward"], fw), what
    assert np.array_equal(m["hist_rc"], rc), what


LADDER2 = 2.0 ** np.linspace(0, 33, 133)


# ---- known answers ---------------------------------------------------------------------------------------------
def kat_texts():
    kats = [k["input"].encode("latin-1") for g in ("dna_w_rc", "dna_w_rc_partial") for k in KATS.get(g, [])
            if isinstance(k.get("input"), str)]
    return [t for t in kats if t and all(c in b"ACGT" for c in t)] + [b"ACAGAGAT"]


def test_kats(native):
    texts = kat_texts()
    assert len(texts) >= 2
    for text in texts:
        for with_rc in (True, False):
            recs = oracle_records(text, with_rc)
            for grid in [(1, 1), (2, 3), (8, 8)]:
                m = both_forms(lambda: native.factor_maps(text, with_rc=with_rc, grid=grid))
                check_grid(m, recs, grid, None, what=(text, with_rc, grid))


# ---- the golden genomes: text source ------------------------------------------------------------------------------
@pytest.mark.parametrize("with_rc", [True, False])
@pytest.mark.parametrize("name", genomes.NAMES)
def test_genomes_text_source(native, name, with_rc):
    for rid, seq in genomes.records(name):
        recs = oracle_records(seq, with_rc)
        n = len(seq)
        for grid in GRIDS:
            for total in (None, n, n // 2):
                for minlen in (1, 2, 20):
                    what = (name, rid, with_rc, grid, total, minlen)
                    m = both_forms(lambda: native.factor_maps(seq, with_rc=with_rc, grid=grid, total_length=total,
                                                              min_factor_length=minlen))
                    check_grid(m, recs, grid, total, minlen, what=what)
        # both consumers behind one run, ladder and caller's edges, LDS-private and global counts
        for minlen in (1, 20):
            if int((recs[:, 1] >= minlen).sum()) == 0 or int(recs[recs[:, 1] >= minlen, 0].max()) == 0:
                continue
            m = both_forms(lambda: native.factor_maps(seq, with_rc=with_rc, grid=(50, 50), min_factor_length=minlen,
                                                      length_edges=LADDER2))
            check_grid(m, recs, (50, 50), None, minlen, what=(name, rid, "both"))
            check_hist(m, recs, LADDER2, None, minlen, what=(name, rid, "ladder"))
            pe = np.linspace(0, n, 2501)  # more position edges than are staged in LDS
            m = both_forms(lambda: native.factor_maps(seq, with_rc=with_rc, min_factor_length=minlen,
                                                      length_edges=[1, 2, 3, 5, 8, 13, 100, 1e4], position_edges=pe))
            assert m["forward_units"] is None
            check_hist(m, recs, [1, 2, 3, 5, 8, 13, 100, 1e4], pe, minlen, what=(name, rid, "edges"))


# ---- the multi-record genomes: FASTA source -----------------------------------------------------------------------
MULTI = [n for n in genomes.NAMES if len(genomes.records(n)) > 1]


@pytest.mark.parametrize("with_rc", [True, False])
@pytest.mark.parametrize("name", MULTI)
def test_genomes_fasta_source(native, name, with_rc, tmp_path):
    path = genomes.materialize(name, tmp_path)
    seqs = [s for _, s in genomes.records(name)]
    if with_rc:
        S, orig, sent_pos = oracle.prepare_multiple_dna_w_rc(seqs)
        f = oracle.factors_array_multiple_dna_w_rc(S)
    else:
        S, orig, sent_pos = native.prepare_multiple_dna_sequences_no_rc_bytes([s.decode() for s in seqs])
        f = oracle.factors_array(S)
    recs = np.stack([f["start"], f["length"], f["ref"]], axis=1)
    sentinels = np.flatnonzero(np.isin(f["start"], np.asarray(sent_pos, dtype=np.uint64))).tolist()
    assert len(sentinels) >= len(seqs) - 1
    n = int(orig)
    for grid in GRIDS:
        for total in (None, n, n // 2):
            for minlen in (1, 2, 20):
                what = (name, with_rc, grid, total, minlen)
                m = both_forms(lambda: native.fasta_factor_maps(path, with_rc=with_rc, grid=grid, total_length=total,
                                                                min_factor_length=minlen))
                check_grid(m, recs, grid, total, minlen, sentinels, what=what)
    m = both_forms(lambda: native.fasta_factor_maps(path, with_rc=with_rc, grid=(50, 50), min_factor_length=20,
                                                    length_edges=LADDER2))
    check_grid(m, recs, (50, 50), None, 20, sentinels, what=(name, "both"))
    check_hist(m, recs, LADDER2, None, 20, sentinels, what=(name, "ladder"))


# ---- long factors across many cells on both strands ---------------------------------------------------------------
def long_copy_text():
    """2^24 bases: repeat_dna pieces with forward and reverse-complement copies of 10^4 .. 10^5 bases between them"""
    rng = np.random.default_rng(11)
    base = gen.repeat_dna(1 << 22, seed=0x5EED0101, lo=64, hi=4096).tobytes()
    parts, total, k = [base], len(base), 0
    while total < (1 << 24):
        length = int(rng.integers(10_000, 100_001))
        at = int(rng.integers(0, len(base) - length))
        piece = base[at:at + length]
        parts.append(genomes.revcomp(piece) if k % 2 else piece)
        filler = gen.repeat_dna(int(rng.integers(50_000, 400_000)), seed=0x5EED0200 + k, lo=64, hi=4096).tobytes()
        parts.append(filler)
        total += length + len(filler)
        k += 1
    return b"".join(parts)[:1 << 24]


@pytest.mark.parametrize("with_rc", [True, False])
def test_long_factors_cross_many_cells(native, with_rc):
    text = long_copy_text()
    recs = oracle_records(text, with_rc)
    is_rc = (recs[:, 2] >> np.uint64(63)).astype(bool)
    assert int(recs[~is_rc, 1].max()) >= 10_000
    if with_rc:
        assert int(recs[is_rc, 1].max()) >= 10_000
    for grid in [(512, 512), (4096, 64)]:
        m = both_forms(lambda: native.factor_maps(text, with_rc=with_rc, grid=grid, length_edges=LADDER2))
        check_grid(m, recs, grid, None, what=(with_rc, grid))
        check_hist(m, recs, LADDER2, None, what=(with_rc, grid))


# ---- the records source -------------------------------------------------------------------------------------------
def synthetic_records(case):
    rows = [(f[0], f[1], f[2] | (1 << 63) if len(f) == 4 and f[3] else f[2]) for f in case["factors"]
            if len(f) in (3, 4)]
    return np.array(rows, dtype=np.uint64).reshape(-1, 3)


def test_records_source_on_the_fixture_lists(native):
    for case in FX["synthetic"]:
        if "ok" not in case:
            continue
        recs = synthetic_records(case)
        grid = (case["grid"], case["grid"]) if isinstance(case["grid"], int) else tuple(case["grid"])
        for chunk in (None, 2):
            with env(NOLZSS_FACTOR_MAPS_CHUNK=chunk):
                m = both_forms(lambda: native.records_factor_maps(recs, grid=grid, total_length=case["total_length"]))
            check_grid(m, recs, grid, case["total_length"], what=(case["name"], chunk))


def test_records_source_at_the_width_caps(native):
    rng = np.random.default_rng(2024)
    z = 100_000
    top = (1 << 32) - (1 << 19)
    length = rng.integers(1, (1 << 20) + 1, z).astype(np.uint64)
    start = np.sort(rng.integers(0, top - (1 << 20), z)).astype(np.uint64)
    ref = rng.integers(0, top - (1 << 20), z).astype(np.uint64)
    strand = rng.random(z) < 0.5
    recs = np.stack([start, length, ref | (strand.astype(np.uint64) << np.uint64(63))], axis=1)
    sentinels = sorted(rng.choice(z, 200, replace=False).tolist())
    grid = (4096, 4096)
    for total, minlen in ((None, 1), (top, 1 << 19), (1 << 31, 1)):
        with env(NOLZSS_FACTOR_MAPS_CHUNK=7777):
            m = native.records_factor_maps(recs, sentinels, grid=grid, total_length=total, min_factor_length=minlen,
                                           length_edges=LADDER2, position_edges=np.linspace(0, top, 4097))
        s, l, r, is_rc = model.kept_factors(recs, minlen, sentinels)
        assert m["z_used"] == len(s) and (minlen == 1 or len(s) < z)
        fw, rc, unit = model.exact_grid(zip(s.tolist(), l.tolist(), r.tolist(), is_rc.tolist()), *grid, total)
        for got, exp in ((m["forward_units"], fw), (m["rc_units"], rc)):
            ys, xs = np.nonzero(got)
            assert {(y, x): int(v) for y, x, v in zip(ys.tolist(), xs.tolist(), got[ys, xs].tolist())} == exp
        check_hist(m, recs, LADDER2, np.linspace(0, top, 4097), minlen, sentinels)
        one = native.records_factor_maps(recs, sentinels, grid=grid, total_length=total, min_factor_length=minlen)
        assert np.array_equal(one["forward_units"], m["forward_units"])
        assert np.array_equal(one["rc_units"], m["rc_units"])


# ---- the Python layer ---------------------------------------------------------------------------------------------
def fixture_grids(ok):
    yb, xb = ok["shape"]
    fw, rc, bias = np.zeros((yb, xb)), np.zeros((yb, xb)), np.zeros((yb, xb))
    mask = np.ones((yb, xb), dtype=bool)
    for y, x, f, r, b in ok["cells"]:
        fw[y, x], rc[y, x], bias[y, x], mask[y, x] = f, r, b, False
    return fw, rc, bias, mask


def check_against_fixture(plots, got, case, z_used, x_max, what):
    ok = case["ok"]
    ref_fw, ref_rc, ref_bias, ref_mask = fixture_grids(ok)
    yb, xb = ok["shape"]
    assert got["forward_grid"].shape == (yb, xb) and got["z_used"] == z_used, what
    assert list(got["x_edges"][[0, 1, -1]]) == ok["x_edges"] and len(got["x_edges"]) == ok["n_x_edges"], what
    assert list(got["y_edges"][[0, 1, -1]]) == ok["y_edges"] and len(got["y_edges"]) == ok["n_y_edges"], what
    integer_edges = got["x_edges"][-1] % xb == 0 and got["y_edges"][-1] % yb == 0
    if integer_edges:
        assert np.array_equal(got["forward_grid"], ref_fw) and np.array_equal(got["rc_grid"], ref_rc), what
        assert np.array_equal(np.ma.getmaskarray(got["bias_grid"]), ref_mask), what
        np.testing.assert_array_max_ulp(got["bias_grid"].data[~ref_mask], ref_bias[~ref_mask], maxulp=8)
    else:
        bound = 4 * 2.0 ** -52 * x_max * (z_used + 1)
        assert bound < 1 / (4 * got["unit"]), what
        diff = max(np.abs(got["forward_grid"] - ref_fw).max(), np.abs(got["rc_grid"] - ref_rc).max())
        print(f"{what}: max |device - reference| = {diff:.3g} (bound {bound:.3g})")
        assert diff <= bound, what
        again = plots.bias_from_grids(got["forward_grid"], got["rc_grid"])
        assert np.array_equal(np.ma.getmaskarray(got["bias_grid"]), np.ma.getmaskarray(again)), what
        assert np.array_equal(got["bias_grid"].data, again.data), what


def test_python_layer_against_the_reference_fixtures(native, plots, tmp_path):
    for case in FX["genome"]:
        seq = genomes.records(case["genome"])[0][1]
        grid = case["grid"] if isinstance(case["grid"], int) else tuple(case["grid"])
        got = plots.strand_bias_grid(seq, with_rc=case["with_rc"], grid_size=grid, total_length=case["total_length"],
                                     min_factor_length=case["min_factor_length"])
        check_against_fixture(plots, got, case, case["z_used"], got["x_edges"][-1], (case["genome"], grid))
    for case in FX["synthetic"]:
        if "ok" not in case:
            continue
        factors = [tuple(f) for f in case["factors"]]
        grid = case["grid"] if isinstance(case["grid"], int) else tuple(case["grid"])
        got = plots.factors_strand_bias_grid(factors, grid_size=grid, total_length=case["total_length"])
        z_used = sum(1 for f in factors if len(f) in (3, 4))
        check_against_fixture(plots, got, case, z_used, got["x_edges"][-1], case["name"])
    # a v2 factor file: total_length and the sentinel indices come from its footer
    path = genomes.materialize("test_bacterial_dna", tmp_path)
    out = str(tmp_path / "bact.bin")
    native.write_factors_binary_file_fasta_multiple_dna_w_rc(path, out)
    from nolzss_amd.utils import read_factors_binary_file_with_metadata
    meta = read_factors_binary_file_with_metadata(out)
    got = plots.factors_strand_bias_grid(out, grid_size=(16, 8), min_factor_length=20)
    seqs = [s for _, s in genomes.records("test_bacterial_dna")]
    S, _, sent_pos = oracle.prepare_multiple_dna_w_rc(seqs)
    f = oracle.factors_array_multiple_dna_w_rc(S)
    recs = np.stack([f["start"], f["length"], f["ref"]], axis=1)
    sentinels = np.flatnonzero(np.isin(f["start"], np.asarray(sent_pos, dtype=np.uint64))).tolist()
    assert sentinels == meta["sentinel_factor_indices"]
    s, l, r, is_rc = model.kept_factors(recs, 20, sentinels)
    fw, rc, _, _ = model.exact_grid_fast(s, l, r, is_rc, 16, 8, meta["total_length"])
    assert np.array_equal(got["forward_units"], fw) and np.array_equal(got["rc_units"], rc)
    via_fasta = plots.fasta_strand_bias_grid(path, grid_size=(16, 8), min_factor_length=20)
    fw2, rc2, _, _ = model.exact_grid_fast(s, l, r, is_rc, 16, 8, None)
    assert np.array_equal(via_fasta["forward_units"], fw2) and np.array_equal(via_fasta["rc_units"], rc2)
    with pytest.raises(plots.PlotError, match="No factors available"):
        plots.strand_bias_grid(b"ACGT", min_factor_length=100)


def reference_space_scale(recs, genome_bin_size=1.0, base=2.0):
    """plots.py:2566-2610 evaluated with numpy on the given records"""
    is_rc = (recs[:, 2] >> np.uint64(63)).astype(bool)
    starts, lengths = recs[:, 0].astype(np.int64), recs[:, 1].astype(np.int64)
    genome_end = int(starts.max())
    genome_bin_bp = int(genome_bin_size * 1_000_000)
    nb = max(50, int(np.ceil(genome_end / genome_bin_bp)))
    genome_bins = np.linspace(0, genome_end, nb + 1)
    min_length, max_length = max(1, int(lengths.min())), int(lengths.max())
    min_log = np.floor(np.log(min_length) / np.log(base))
    max_log = np.ceil(np.log(max_length) / np.log(base))
    edges = base ** np.linspace(min_log, max_log, int((max_log - min_log) * 4) + 1)
    hists = []
    for sel in (~is_rc, is_rc):
        if not sel.any():
            hists.append(np.zeros((len(edges) - 1, nb)))
            continue
        h, _, _ = np.histogram2d(lengths[sel], starts[sel], bins=[edges, genome_bins])
        hists.append(h)
    return genome_bins, edges, hists[0], hists[1]


@pytest.mark.parametrize("base", [2.0, 1.5, 10.0])
def test_space_scale_histogram(native, plots, base):
    texts = [("T7", genomes.records("T7")[0][1]), ("pow2", gen.random_dna(3000, seed=3).tobytes() * 2 + b"ACGT" * 1024),
             ("repeat", gen.repeat_dna(1 << 20, seed=12).tobytes())]
    for name, text in texts:
        for with_rc in (True, False):
            recs = oracle_records(text, with_rc)
            for minlen in (1, 8):
                kept = recs[recs[:, 1] >= minlen]
                got = plots.space_scale_histogram(text, with_rc=with_rc, length_log_base=base, genome_bin_size=0.01,
                                                  min_factor_length=minlen)
                bins, edges, fw, rc = reference_space_scale(kept, 0.01, base)
                what = (name, with_rc, minlen, base)
                assert got["genome_bins"].tobytes() == bins.tobytes(), what
                assert got["length_bin_edges"].tobytes() == edges.tobytes(), what
                assert got["forward_hist"].dtype == np.float64 and np.array_equal(got["forward_hist"], fw), what
                assert np.array_equal(got["reverse_hist"], rc), what
    tuples = [(0, 1, 0), (1, 4, 0, True), (5, 16, 1), (21, 3, 2, True)]
    got = plots.space_scale_histogram(factors=tuples, length_log_base=base)
    recs = np.array([(0, 1, 0), (1, 4, 1 << 63), (5, 16, 1), (21, 3, 2 | (1 << 63))], dtype=np.uint64)
    bins, edges, fw, rc = reference_space_scale(recs, 1.0, base)
    assert got["length_bin_edges"].tobytes() == edges.tobytes() and np.array_equal(got["forward_hist"], fw)
    assert np.array_equal(got["reverse_hist"], rc) and got["genome_bins"].tobytes() == bins.tobytes()
    with pytest.raises(plots.PlotError):
        plots.space_scale_histogram(b"A")


# ---- refusals -----------------------------------------------------------------------------------------------------
def test_refusals_mirror_the_entry_points(native, tmp_path):
    for bad in (b"ACGTNACGT", b"ACGxT"):
        with pytest.raises(RuntimeError) as e1:
            native.count_factors_dna_w_rc(bad)
        with pytest.raises(RuntimeError) as e2:
            native.factor_maps(bad, with_rc=True, grid=(4, 4))
        assert str(e2.value) == str(e1.value)
    assert native.factor_maps(b"", with_rc=True, grid=(4, 4))["z"] == 0
    assert native.factor_maps(b"", grid=(4, 4))["z_used"] == 0
    m = native.factor_maps(b"ACGTNACGT", grid=(4, 4))  # plain mode takes any bytes, as count_factors does
    assert m["z"] == native.count_factors(b"ACGTNACGT")
    bad_fa = tmp_path / "many.fa"
    gen.write_fasta(bad_fa, [(f"r{i}", b"ACGT" * 3) for i in range(130)])
    with pytest.raises(ValueError) as e1:
        native.factorize_fasta_multiple_dna_w_rc(str(bad_fa))
    with pytest.raises(ValueError) as e2:
        native.fasta_factor_maps(str(bad_fa), grid=(4, 4))
    assert str(e2.value) == str(e1.value)
    with pytest.raises(Exception) as e1:
        native.factorize_fasta_multiple_dna_w_rc(str(tmp_path / "missing.fa"))
    with pytest.raises(Exception) as e2:
        native.fasta_factor_maps(str(tmp_path / "missing.fa"), grid=(4, 4))
    assert type(e2.value) is type(e1.value) and str(e2.value) == str(e1.value)
    with pytest.raises(ValueError, match="sanitize_mode"):
        native.fasta_factor_maps(str(bad_fa), sanitize_mode="other", grid=(4, 4))
    text = b"ACGTACGTAC"
    for grid in [(0, 5), (5, 0), (4097, 1), (1, 4097)]:
        with pytest.raises(ValueError, match="between 1 and 4096"):
            native.factor_maps(text, grid=grid)
    with pytest.raises(ValueError, match="ascending"):
        native.factor_maps(text, length_edges=[1.0, 4.0, 2.0])
    with pytest.raises(ValueError, match="beyond 2\\^33"):
        native.records_factor_maps(np.array([[1 << 34, 5, 0]], dtype=np.uint64), grid=(4, 4))
    # no device work was left half done: the next call answers
    assert native.factor_maps(text, grid=(2, 2))["z"] == native.count_factors(text)
