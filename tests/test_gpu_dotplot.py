"""GPU: self dot-plot rasters rendered on the device from resident factor records (nolzss_dotplot_*,
nolzss_amd.genomics.plots.self_dotplot).  Every raster, count, visible number and hover table must EQUAL the
per-base-pair model of tests/dotplot_model.py: integers, no tolerance.  The factors always come from the CPU checker
or are synthetic, never from the device."""
import os
from contextlib import contextmanager

import numpy as np
import pytest

import dotplot_model as model
import gen
import genomes
import oracle_lib as oracle

pytestmark = pytest.mark.gpu

RC = 1 << 63
RASTERS = [(1, 1), (64, 64), (37, 101), (800, 800), (4096, 3), (3, 4096)]
HOVER = [1, 50, 2000]


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


def same(a, b, what=""):
    assert a.keys() == b.keys(), what
    for k, v in a.items():
        if isinstance(v, np.ndarray):
            assert np.array_equal(v, b[k]), (what, k)
        else:
            assert v == b[k], (what, k)


def both_forms(dp, *args, **kw):
    """the render with the LDS strip and with NOLZSS_DOTPLOT_GLOBAL=1: equal"""
    with env(NOLZSS_DOTPLOT_GLOBAL=None):
        a = dp.render(*args, **kw)
    with env(NOLZSS_DOTPLOT_GLOBAL="1"):
        b = dp.render(*args, **kw)
    same(a, b, ("forms", args, kw))
    return a


def check(dp, recs, x_range, y_range, W, H, sentinels=(), what="", **kw):
    """device (both forms) against the model for one view; kw: min_factor_length, length_range, hover_bins, counts"""
    exp = model.render(recs, x_range, y_range, W, H, sentinels=sentinels, **kw)
    got = both_forms(dp, x_range, y_range, width=W, height=H, **kw)
    model.assert_equal(got, exp, (what, x_range, y_range, W, H, kw))
    return exp


# ---- 1. synthetic records -------------------------------------------------------------------------------------------
def synthetic_records(z=3000, n_long=90, seed=2025, zoom=None):
    """both strands, sorted by start as the pipeline leaves them: lengths mostly 1-30, n_long of 10^3 .. 10^5
    (log-uniform, about 2 M base pairs in all); starts and refs below 2^20.  zoom: four more factors that cross the
    left, right, lower and upper side of that window."""
    rng = np.random.default_rng(seed)
    length = rng.integers(1, 31, z)
    long_at = rng.choice(z, n_long, replace=False)
    length[long_at] = np.exp(rng.uniform(np.log(1e3), np.log(1e5), n_long)).astype(np.int64)
    start = rng.integers(0, 1 << 20, z)
    ref = rng.integers(0, 1 << 20, z)
    strand = rng.integers(0, 2, z)
    rows = np.stack([start, length, ref, strand], axis=1).tolist()
    if zoom is not None:
        (x0, x1), (y0, y1) = zoom
        ym = (y0 + y1) // 2
        rows += [[x0 - 300, 900, ym - 300, 0],        # enters through the left side
                 [x1 - 400, 2000, ym, 1],             # leaves through the right side (rc: going down)
                 [x0 + 1000, 5000, y0 - 700, 0],      # enters through the lower side
                 [x0 + 2000, 4000, y1 - 1500, 1]]     # rc: starts above the upper side
    rows.sort(key=lambda r: r[0])
    return np.array([(s, l, r | (RC if k else 0)) for s, l, r, k in rows], dtype=np.uint64)


ZOOM = ((300_000, 340_000), (500_000, 530_000))


@pytest.fixture(scope="module")
def synthetic(native):
    recs = synthetic_records(zoom=ZOOM)
    dp = native.DotPlot.from_records(recs)
    yield recs, dp
    dp.close()


def views_for(recs, W, H):
    s, l, r, is_rc = model.split(recs)
    extent = int(max((s + l).max(), (r + l).max()))
    k = int(np.argmax(l))  # the longest factor: the one-base-per-pixel window sits on its middle base pair
    t = int(l[k] // 2)
    ax, ay = int(s[k]) + t, int(r[k] + l[k]) - 1 - t if is_rc[k] else int(r[k]) + t
    return [("full square", (0, extent), (0, extent)),
            ("one base per pixel", (ax, ax + W), (max(0, ay - H // 2), max(0, ay - H // 2) + H)),
            ("spans not divisible", (3, 3 + (extent // W) * W + 1 + (W > 1)), (5, 5 + (extent // H) * H + 1 + (H > 1))),
            ("zoom", *ZOOM)]


@pytest.mark.parametrize("raster", RASTERS, ids=[f"{w}x{h}" for w, h in RASTERS])
def test_synthetic_records(synthetic, raster):
    recs, dp = synthetic
    W, H = raster
    assert dp.info["z"] == len(recs)
    for n, (name, xr, yr) in enumerate(views_for(recs, W, H)):
        exp = check(dp, recs, xr, yr, W, H, what=name, counts=True, hover_bins=HOVER[(n + W) % 3])
        assert exp["visible_forward"] + exp["visible_rc"] >= 1, name
        if name in ("full square", "zoom"):
            assert exp["visible_forward"] >= 2 and exp["visible_rc"] >= 2, name
        plain = dp.render(xr, yr, width=W, height=H)  # without counts, without a table
        assert plain["count_forward"] is None and plain["hover_length"] is None
        assert np.array_equal(plain["max_forward"], exp["max_forward"]), name
        assert np.array_equal(plain["max_rc"], exp["max_rc"]), name
        assert (plain["visible_forward"], plain["visible_rc"]) == (exp["visible_forward"], exp["visible_rc"])
    # the keep rule and the slider
    name, xr, yr = views_for(recs, W, H)[0]
    check(dp, recs, xr, yr, W, H, what="minlen", min_factor_length=25, counts=True, hover_bins=50)
    check(dp, recs, xr, yr, W, H, what="slider", length_range=(7, 1500), counts=True, hover_bins=50)


def test_info_of_the_records_source(synthetic):
    recs, dp = synthetic
    s, l, r, is_rc = model.split(recs)
    assert dp.info["x_max"] == int((s + l).max()) and dp.info["y_max"] == int((r + l).max())
    assert (dp.info["min_length"], dp.info["max_length"]) == (int(l.min()), int(l.max()))
    assert (dp.info["kept_forward"], dp.info["kept_rc"]) == (int((~is_rc).sum()), int(is_rc.sum()))
    assert dp.info["sentinel_starts"].size == 0


# ---- 2. edges ---------------------------------------------------------------------------------------------------
X0, Y0, SPAN = 1000, 2000, 6400  # the edge view: [1000, 7400) x [2000, 8400)


def edge_records(x0=X0, y0=Y0, span=SPAN):
    x1, y1 = x0 + span, y0 + span
    rows = [(x0 - 100, span + 200, y0 - 100, 0)]                     # corner to corner, forward
    rows += [(x0 - 100, span + 200, y0 - 100, 1)]                    # corner to corner, rc: (x0, y1 - 1) is a base pair
    rows += [(x0 - 90 + k, span + 200, y0 - 100 + 7 * k, k & 1) for k in range(6)]   # several long ones in one wave
    rows += [(x0 + 100, 30, y0 + 1000, 0), (x0 + 105, 30, y0 + 1100, 1)]          # hover tie: the first one wins
    rows += [(x0 + 900, 9, y0 + 50, 0), (x0 + 910, 10, y0 + 60, 0),                 # the slider (10, 30) is inclusive
             (x0 + 920, 30, y0 + 70, 1), (x0 + 930, 31, y0 + 80, 1)]
    rows += [(x1 - 10, 10, y0 + 500, 0)]                             # ends exactly at x_hi
    rows += [(x1, 10, y0 + 500, 0)]                                  # starts at x_hi: not visible
    rows += [(x1 - 1, 1, y1 - 1, 0)]                                 # only the last pixel
    rows += [(x1 - 1, 40, y1 - 40, 1)]                               # rc whose first base pair alone is in view: the last pixel
    rows += [(x0 + 300, 50, y1, 0), (x0 + 300, 50, y0 - 50, 1)]      # just above, just below
    rows += [(3 * x1, 50, 100, 0), (10, 50, 3 * y1, 1)]              # wholly outside
    rows.sort(key=lambda r: r[0])
    return np.array([(s, l, r | (RC if k else 0)) for s, l, r, k in rows], dtype=np.uint64)


@pytest.mark.parametrize("origin", [(X0, Y0), ((1 << 33) - SPAN, (1 << 33) - SPAN - 12345)], ids=["low", "at 2^33"])
def test_edges(native, origin):
    x0, y0 = origin
    recs = edge_records(x0, y0)
    xr, yr = (x0, x0 + SPAN), (y0, y0 + SPAN)
    short = int(np.flatnonzero(recs[:, 1] == 9)[0])
    with native.DotPlot.from_records(recs, [short]) as dp:
        assert dp.info["sentinel_starts"].tolist() == [int(recs[short, 0])]
        for W, H in [(64, 48), (4096, 100), (640, 4096), (1, 1)]:
            exp = check(dp, recs, xr, yr, W, H, [short], what="all", counts=True, hover_bins=8)
            if (W, H) != (1, 1):  # the upper right pixel: the one-base factor and the corner-to-corner one | the rc of 40
                assert exp["max_forward"][H - 1, W - 1] == SPAN + 200 and exp["max_rc"][H - 1, W - 1] == 40
                assert exp["count_forward"][H - 1, W - 1] >= 2
            assert exp["visible_forward"] == 9 and exp["visible_rc"] == 8
            tie = check(dp, recs, xr, yr, W, H, [short], what="tie", length_range=(30, 30), hover_bins=8)
            assert tie["hover_start"][0] == x0 + 100 and tie["hover_ref"][0] == y0 + 1000  # the smaller index
            exp = check(dp, recs, xr, yr, W, H, [short], what="slider", length_range=(10, 30), counts=True)
            assert (exp["visible_forward"], exp["visible_rc"]) == (3, 2)   # 10, 30, 10 (ends at x_hi) | 30, 30
            exp = check(dp, recs, xr, yr, W, H, [short], what="sentinel stays", min_factor_length=20, counts=True,
                        hover_bins=64)
            assert exp["visible_forward"] == 4 + 2  # four crossing ones, the hover tie's first, the sentinel factor of 9


# ---- 3. both forms, records that are not sorted -----------------------------------------------------------------
def test_shuffled_records_over_several_workgroups(native):
    """9000 records: three chunks, so more than one workgroup meets in the rasters; in shuffled order the strip mostly
    misses"""
    recs = synthetic_records(z=9000, n_long=60, seed=77, zoom=ZOOM)
    order = np.random.default_rng(5).permutation(len(recs))
    s, l, r, _ = model.split(recs)
    extent = int(max((s + l).max(), (r + l).max()))
    sentinels = [11, 4000, 8999]
    for name, rr, sent in (("sorted", recs, sentinels), ("shuffled", recs[order], sentinels)):
        with native.DotPlot.from_records(rr, sent) as dp:
            for W, H, xr, yr in [(800, 800, (0, extent), (0, extent)), (64, 4096, *ZOOM), (333, 77, (0, extent), (7, extent))]:
                check(dp, rr, xr, yr, W, H, sent, what=name, min_factor_length=12, counts=True, hover_bins=2000)


# ---- 4. sources -------------------------------------------------------------------------------------------------
def oracle_records(text: bytes, with_rc: bool):
    if with_rc:
        S, _, _ = oracle.prepare_multiple_dna_w_rc([text])
        f = oracle.factors_array_multiple_dna_w_rc(S)
    else:
        f = oracle.factors_array(text)
    return np.stack([f["start"], f["length"], f["ref"]], axis=1)


@pytest.mark.parametrize("with_rc", [True, False])
def test_text_source(native, plots, with_rc):
    text = gen.repeat_dna(1 << 16, seed=0x5EED0D07).tobytes()
    recs = oracle_records(text, with_rc)
    with plots.self_dotplot(text, with_rc=with_rc) as dp:
        assert dp.info["z"] == len(recs) and dp.info["sentinel_starts"].size == 0
        extent = max(dp.info["x_max"], dp.info["y_max"])
        assert extent == len(text)
        got = dp.render(width=256, height=200, counts=True, hover_bins=50)  # the default view
        assert (got["x_range"], got["y_range"]) == ((0, extent), (0, extent))
        exp = model.render(recs, (0, extent), (0, extent), 256, 200, counts=True, hover_bins=50)
        model.assert_equal(got, exp, "default view")
        assert exp["visible_forward"] + exp["visible_rc"] == len(recs)
        check(dp, recs, (20_000, 24_096), (0, 30_000), 4096, 800, what="zoom", counts=True, hover_bins=2000)
        check(dp, recs, (0, extent), (0, extent), 800, 800, what="minlen", min_factor_length=20, hover_bins=1)
        assert dp.sequence_boundaries == [(0, extent, "sequence")]


@pytest.mark.parametrize("with_rc", [True, False])
@pytest.mark.parametrize("name", ["short_dna1", "T7"])
def test_fasta_and_records_sources(native, plots, name, with_rc):
    path = str(genomes.DIR / f"{name}.fasta")
    seqs = [s for _, s in genomes.records(name)]
    if with_rc:
        S, _, sent_pos = oracle.prepare_multiple_dna_w_rc(seqs)
        f = oracle.factors_array_multiple_dna_w_rc(S)
    else:
        S, _, sent_pos = native.prepare_multiple_dna_sequences_no_rc_bytes([s.decode() for s in seqs])
        f = oracle.factors_array(S)
    recs = np.stack([f["start"], f["length"], f["ref"]], axis=1)
    sentinels = np.flatnonzero(np.isin(f["start"], np.asarray(sent_pos, dtype=np.uint64))).tolist()
    names = [rid for rid, _ in genomes.records(name)]
    with plots.self_dotplot(fasta_filepath=path, with_rc=with_rc) as a, \
            plots.self_dotplot(factors=recs, sentinel_factor_indices=sentinels, sequence_names=names) as b:
        assert a.info["z"] == b.info["z"] == len(recs)
        assert a.info["sentinel_starts"].tolist() == f["start"][sentinels].tolist() == b.info["sentinel_starts"].tolist()
        assert {k: v for k, v in a.info.items() if k != "sentinel_starts"} == \
            {k: v for k, v in b.info.items() if k != "sentinel_starts"}
        assert a.sequence_boundaries == b.sequence_boundaries
        assert len(a.sequence_boundaries) == len(sentinels) + 1 and a.sequence_boundaries[0][2] == names[0]
        extent = max(a.info["x_max"], a.info["y_max"])
        zoom = min(700, extent - extent // 3)  # (short_dna1 is a few dozen bases: the rasters shrink to the spans)
        for W, H, xr, yr in [(min(400, extent), min(300, extent), (0, extent), (0, extent)),
                             (min(50, zoom), min(64, extent), (extent // 3, extent // 3 + zoom), (0, extent))]:
            kw = dict(min_factor_length=20, counts=True, hover_bins=50)
            exp = check(a, recs, xr, yr, W, H, sentinels, what=(name, "fasta"), **kw)
            got = both_forms(b, xr, yr, width=W, height=H, **kw)
            model.assert_equal(got, exp, (name, "records"))
        # the sentinel factors stay whatever min_factor_length: with one above every length they are all that is left
        beyond = int(f["length"].max()) + 1
        exp = check(a, recs, (0, extent), (0, extent), min(64, extent), min(64, extent), sentinels,
                    what=(name, "sentinels only"), min_factor_length=beyond, counts=True, hover_bins=8)
        assert exp["visible_forward"] + exp["visible_rc"] == len(sentinels)


# ---- 5. residency -------------------------------------------------------------------------------------------------
def test_handles_outlive_other_calls(native):
    t1 = gen.repeat_dna(1 << 16, seed=0x5EED0D11).tobytes()
    t2 = gen.repeat_dna(1 << 16, seed=0x5EED0D12).tobytes()
    other = gen.repeat_dna((1 << 16) + 999, seed=0x5EED0D13).tobytes()
    r1, r2 = oracle_records(t1, True), oracle_records(t2, False)
    n = len(t1)
    v1 = dict(width=300, height=200, counts=True, hover_bins=50)
    v2 = dict(width=64, height=64, counts=True, hover_bins=1)
    a = native.DotPlot.from_text(t1, with_rc=True)
    got = native.factorize_array(other)  # an ordinary call recycles the device arena
    exp = oracle.factors_array(other)
    assert all(np.array_equal(got[k], exp[k]) for k in ("start", "length", "ref"))
    b = native.DotPlot.from_text(t2, with_rc=False)
    first = a.render((0, n), (0, n), **v1)
    model.assert_equal(first, model.render(r1, (0, n), (0, n), 300, 200, counts=True, hover_bins=50), "A")
    model.assert_equal(b.render((0, n), (0, n), **v1), model.render(r2, (0, n), (0, n), 300, 200, counts=True, hover_bins=50), "B")
    zoom = a.render((n // 2, n // 2 + 640), (0, n), **v2)  # another view in between: the rasters start from zero again
    model.assert_equal(zoom, model.render(r1, (n // 2, n // 2 + 640), (0, n), 64, 64, counts=True, hover_bins=1), "A zoom")
    same(a.render((0, n), (0, n), **v1), first, "A again")
    a.close()
    a.close()  # harmless
    with pytest.raises(ValueError, match="closed"):
        a.render((0, n), (0, n))
    assert native.count_factors(other) == len(exp)
    model.assert_equal(b.render((0, n), (0, n), **v2), model.render(r2, (0, n), (0, n), 64, 64, counts=True, hover_bins=1), "B after A closed")
    b.close()


# ---- 6. refusals ----------------------------------------------------------------------------------------------------
def test_refusals(native):
    recs = np.array([(0, 5, 0), (5, 3, 1 | RC)], dtype=np.uint64)
    with native.DotPlot.from_records(recs) as dp:
        ok = dict(x_range=(0, 100), y_range=(0, 100), width=10, height=10)
        assert dp.render(**ok)["visible_forward"] == 1
        for change, field in [(dict(x_range=(0, 9)), "x_hi - x_lo is below width"),
                              (dict(y_range=(0, 9)), "y_hi - y_lo is below height"),
                              (dict(width=0), "width"), (dict(height=4097), "height"), (dict(width=4097), "width"),
                              (dict(x_range=(50, 50)), "x_lo"), (dict(x_range=(60, 50)), "x_lo"),
                              (dict(y_range=(60, 50)), "y_lo"), (dict(hover_bins=4097), "hover_bins"),
                              (dict(x_range=(0, (1 << 33) + 1)), "x_hi"), (dict(length_range=(5, 4)), "len_lo")]:
            with pytest.raises(ValueError, match=field):
                dp.render(**{**ok, **change})
        with pytest.raises(ValueError, match="shrink the raster"):
            dp.render(x_range=(0, 99), y_range=(0, 100), width=100, height=10)
        assert dp.render(**ok)["visible_rc"] == 1  # nothing was left half done
    with pytest.raises(ValueError, match="length"):
        native.DotPlot.from_records(np.array([(0, 5, 0), (9, 1 << 32, 0)], dtype=np.uint64))
    for with_rc in (False, True):
        with native.DotPlot.from_text(b"", with_rc=with_rc) as dp:
            assert dp.info["z"] == 0 and dp.info["x_max"] == 0 and dp.info["max_length"] == 0
            got = dp.render((0, 64), (0, 64), width=64, height=32, counts=True, hover_bins=4)
            assert got["max_forward"].shape == (32, 64) and not got["max_forward"].any() and not got["max_rc"].any()
            assert not got["count_forward"].any() and not got["hover_length"].any()
            assert (got["visible_forward"], got["visible_rc"]) == (0, 0)
    with native.DotPlot.from_records(np.zeros((0, 3), dtype=np.uint64)) as dp:
        assert dp.info["z"] == 0
    for bad in (b"ACGTNACGT", b"ACGxT"):  # the refusals of the factor maps' text source
        with pytest.raises(RuntimeError) as e1:
            native.count_factors_dna_w_rc(bad)
        with pytest.raises(RuntimeError) as e2:
            native.DotPlot.from_text(bad, with_rc=True)
        assert str(e2.value) == str(e1.value)
