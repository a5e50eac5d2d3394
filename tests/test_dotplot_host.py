"""CPU suite of the self dot plot: the per-base-pair model (tests/dotplot_model.py) against hand-worked rasters, the
column walk the device kernel uses against that model, and the host half of nolzss_amd.genomics.plots.self_dotplot
(sequence boundaries, the default view, the source rule) -- nothing here needs a device."""
import numpy as np
import pytest

import dotplot_model as model

RC = 1 << 63


@pytest.fixture(scope="module")
def plots():
    from nolzss_amd.genomics import plots
    return plots


def test_model_on_atgcat_in_rc_mode():
    """ATGCAT is its own reverse complement: three literals, then CAT as the reverse complement of ATG at 0.  One
    base per pixel: the forward literals sit on the diagonal, the rc factor runs from (3, 2) down to (5, 0)."""
    recs = [(0, 1, 0), (1, 1, 1), (2, 1, 2), (3, 3, 0 | RC)]
    got = model.render(recs, (0, 6), (0, 6), 6, 6, counts=True, hover_bins=6)
    fw = np.zeros((6, 6), dtype=np.uint32)
    fw[0, 0] = fw[1, 1] = fw[2, 2] = 1
    rc = np.zeros((6, 6), dtype=np.uint32)
    rc[2, 3] = rc[1, 4] = rc[0, 5] = 3
    assert np.array_equal(got["max_forward"], fw) and np.array_equal(got["max_rc"], rc)
    assert np.array_equal(got["count_forward"], fw) and np.array_equal(got["count_rc"], rc // 3)
    assert (got["visible_forward"], got["visible_rc"]) == (3, 1)
    # midpoints 0.5, 1.5, 2.5 and 4.5 of 6 columns over [0, 6)
    assert got["hover_start"].tolist() == [0, 1, 2, 0, 3, 0]
    assert got["hover_length"].tolist() == [1, 1, 1, 0, 3, 0]
    assert got["hover_ref"].tolist() == [0, 1, 2, 0, RC, 0]
    # the length window is inclusive and min_factor_length spares the sentinel factor (index 1 here)
    got = model.render(recs, (0, 6), (0, 6), 6, 6, length_range=(1, 1))
    assert np.array_equal(got["max_forward"], fw) and not got["max_rc"].any()
    got = model.render(recs, (0, 6), (0, 6), 6, 6, min_factor_length=2, sentinels=[1])
    assert got["max_forward"].nonzero()[0].tolist() == [1] and np.array_equal(got["max_rc"], rc)
    got = model.render(recs, (0, 6), (0, 6), 6, 6, min_factor_length=2, sentinels=[1], length_range=(2, 0))
    assert not got["max_forward"].any() and np.array_equal(got["max_rc"], rc)


def test_model_on_a_3_by_2_raster_over_a_7_by_5_window():
    """px = x * 3 // 7: x 0 1 2 -> 0, 3 4 -> 1, 5 6 -> 2;  py = y * 2 // 5: y 0 1 2 -> 0, 3 4 -> 1.
    forward (0, 7, 0): base pairs (t, t), t = 0 .. 4 in view (y = 5, 6 are outside): pixels (0, 0) (0, 0) (0, 0) (1, 1)
    (1, 1).  rc (1, 6, 0): y = 5 - t: (1, 5) outside, (2, 4) -> (0, 1), (3, 3) -> (1, 1), (4, 2) -> (1, 0), (5, 1) ->
    (2, 0), (6, 0) -> (2, 0)."""
    recs = [(0, 7, 0), (1, 6, 0 | RC)]
    got = model.render(recs, (0, 7), (0, 5), 3, 2, counts=True, hover_bins=2)
    assert got["max_forward"].tolist() == [[7, 0, 0], [0, 7, 0]]
    assert got["max_rc"].tolist() == [[0, 6, 6], [6, 6, 0]]
    assert got["count_forward"].tolist() == [[1, 0, 0], [0, 1, 0]]
    assert got["count_rc"].tolist() == [[0, 1, 1], [1, 1, 0]]
    assert (got["visible_forward"], got["visible_rc"]) == (1, 1)
    # midpoints 3.5 and 4 of [0, 7) in two columns: both in column 1, the longer factor stays
    assert got["hover_length"].tolist() == [0, 7] and got["hover_start"].tolist() == [0, 0]
    # a window that shows the full factor length although only one base pair is inside
    got = model.render(recs, (6, 9), (0, 2), 3, 2)
    assert got["max_rc"].tolist() == [[6, 0, 0], [0, 0, 0]] and not got["max_forward"].any()


def walk(rec, x_range, y_range, W, H):
    """the pixels of one factor by the column walk of dotplot.hip: {(px, py)}, each produced once"""
    start, length, ref = rec[0], rec[1], rec[2] & ~RC
    rc = bool(rec[2] & RC)
    (x_lo, x_hi), (y_lo, y_hi) = x_range, y_range
    Xs, Ys = x_hi - x_lo, y_hi - y_lo
    ty0, ty1 = (ref + length - y_hi, ref + length - y_lo) if rc else (y_lo - ref, y_hi - ref)
    t0, t1 = max(0, x_lo - start, ty0), min(length, x_hi - start, ty1)
    pixels = []
    if t0 >= t1:
        return pixels
    y_of = (lambda t: ref + length - 1 - t) if rc else (lambda t: ref + t)
    for px in range((start + t0 - x_lo) * W // Xs, (start + t1 - 1 - x_lo) * W // Xs + 1):
        ta = max(t0, -(-px * Xs // W) + x_lo - start)
        tb = min(t1, -(-(px + 1) * Xs // W) + x_lo - start)
        assert ta < tb  # a column is at least one base wide
        ra, rb = ((y_of(t) - y_lo) * H // Ys for t in (ta, tb - 1))
        pixels += [(px, py) for py in range(min(ra, rb), max(ra, rb) + 1)]
    return pixels


def test_column_walk_equals_the_definition():
    """300 random cases: per factor the walk yields every pixel of the definition once, at most W + H - 1 of them,
    so max and count rasters built from the walk equal the model's"""
    rng = np.random.default_rng(7)
    for case in range(300):
        W, H = (int(v) for v in rng.integers(1, 40, 2))
        x_lo, y_lo = (int(v) for v in rng.integers(0, 200, 2))
        x_hi, y_hi = x_lo + W + int(rng.integers(0, 300)), y_lo + H + int(rng.integers(0, 300))
        n = 12
        recs = np.stack([rng.integers(0, 500, n), rng.integers(1, 400, n),
                         rng.integers(0, 500, n) | (rng.integers(0, 2, n) << 63)], axis=1).astype(np.uint64)
        exp = model.render(recs, (x_lo, x_hi), (y_lo, y_hi), W, H, counts=True)
        maxp, cnt = np.zeros((2, H, W), dtype=np.uint32), np.zeros((2, H, W), dtype=np.uint32)
        for rec in recs.tolist():
            pixels = walk(rec, (x_lo, x_hi), (y_lo, y_hi), W, H)
            assert len(pixels) == len(set(pixels)) <= W + H - 1, case
            for px, py in pixels:
                strand = 1 if rec[2] & RC else 0
                maxp[strand, py, px] = max(maxp[strand, py, px], rec[1])
                cnt[strand, py, px] += 1
        assert np.array_equal(maxp[0], exp["max_forward"]) and np.array_equal(maxp[1], exp["max_rc"]), case
        assert np.array_equal(cnt[0], exp["count_forward"]) and np.array_equal(cnt[1], exp["count_rc"]), case


def test_sequence_boundaries_follow_the_reference_rule(plots):
    """plots.py:522-553: a sequence between two sentinel factors, the sentinel itself skipped, names or seq_<i>, the
    last one up to the largest x or y"""
    f = plots.sequence_boundaries_from
    assert f([10, 25], ["a", "b", "c"], 40) == [(0, 10, "a"), (11, 25, "b"), (26, 40, "c")]
    assert f([10, 25], ["a"], 40) == [(0, 10, "a"), (11, 25, "seq_1"), (26, 40, "seq_2")]
    assert f(np.array([7], dtype=np.uint64), None, 9) == [(0, 7, "seq_0"), (8, 9, "seq_1")]
    assert f([], ["only"], 33) == [(0, 33, "only")]
    assert f([], None, 33) == [(0, 33, "sequence")]
    assert f([], None, None) == [(0, 1000, "sequence")]
    assert f([4], ["a", "b"], None) == [(0, 4, "a"), (5, 5, "b")]


def test_default_view_arithmetic(plots):
    f = plots.default_view
    assert f(1000, 700, 800, 800) == ((0, 1000), (0, 1000))          # the square of the diagonal extent
    assert f(700, 1000, 800, 600) == ((0, 1000), (0, 1000))
    assert f(500, 300, 800, 600) == ((0, 800), (0, 600))             # raised to one base per pixel
    assert f(0, 0, 800, 800) == ((0, 800), (0, 800))
    assert f(1000, 700, 800, 800, x_range=(10, 20)) == ((10, 20), (0, 1000))  # a given range is not touched
    assert f(1000, 700, 64, 64, y_range=(5, 900)) == ((0, 1000), (5, 900))


def test_exactly_one_source(plots):
    with pytest.raises(ValueError, match="Exactly one"):
        plots.self_dotplot()
    with pytest.raises(ValueError, match="Exactly one"):
        plots.self_dotplot(b"ACGT", factors=[(0, 1, 0)])
    with pytest.raises(ValueError, match="Exactly one"):
        plots.self_dotplot(fasta_filepath="a.fa", factors=[(0, 1, 0)])
    with pytest.raises(FileNotFoundError):
        plots.self_dotplot(fasta_filepath="/nonexistent/in.fa")
    import noLZSS.genomics.plots as ref_named
    assert ref_named.self_dotplot is plots.self_dotplot and ref_named.DotPlot is plots.DotPlot


def test_view_refusals_and_empty_sources_need_no_device(plots):
    """a handle without factors is valid, renders zero rasters, and refuses a bad view from the request alone"""
    from nolzss_amd import _noLZSS as native
    ok = dict(x_range=(0, 100), y_range=(0, 100), width=10, height=10)
    with native.DotPlot.from_records(np.zeros((0, 3), dtype=np.uint64)) as dp:
        assert dp.info["z"] == 0 and dp.info["sentinel_starts"].size == 0
        for change, field in [(dict(x_range=(0, 9)), "x_hi - x_lo is below width"), (dict(width=0), "width"),
                              (dict(height=4097), "height"), (dict(x_range=(50, 50)), "x_lo"),
                              (dict(y_range=(60, 50)), "y_lo"), (dict(hover_bins=4097), "hover_bins"),
                              (dict(y_range=(0, (1 << 33) + 1)), "y_hi"), (dict(length_range=(5, 4)), "len_lo")]:
            with pytest.raises(ValueError, match=field):
                dp.render(**{**ok, **change})
        with pytest.raises(ValueError, match="shrink the raster"):
            dp.render(x_range=(0, 100), y_range=(0, 9), width=10, height=10)
    dp.close()  # a second and a third close are harmless
    with pytest.raises(ValueError, match="closed"):
        dp.render(**ok)
    for with_rc in (False, True):
        with plots.self_dotplot(b"", with_rc=with_rc) as dp:
            got = dp.render(width=64, height=32, counts=True, hover_bins=4)
            assert (got["x_range"], got["y_range"]) == ((0, 64), (0, 32))
            assert got["max_forward"].shape == (32, 64) and got["max_forward"].dtype == np.uint32
            assert not got["max_forward"].any() and not got["max_rc"].any() and not got["count_rc"].any()
            assert got["hover_length"].tolist() == [0] * 4 and (got["visible_forward"], got["visible_rc"]) == (0, 0)
            assert dp.sequence_boundaries == [(0, 1000, "sequence")]
