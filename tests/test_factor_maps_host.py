"""CPU suite: the exact integer model of the strand-bias grid (tests/factor_maps_model.py) against what the
reference's own _compute_strand_bias_grid produced (tests/golden/python_ref_factor_maps.json, written by
tests/golden/make_factor_map_fixtures.py), the host half of nolzss_amd.genomics.plots (bias, units -> floats, the two
ladders, argument checking) -- nothing here needs a device."""
import json
from pathlib import Path

import numpy as np
import pytest

import factor_maps_model as model
import genomes
import oracle_lib as oracle

FX = json.loads((Path(__file__).resolve().parent / "golden" / "python_ref_factor_maps.json").read_text())


@pytest.fixture(scope="module")
def plots():
    from nolzss_amd.genomics import plots
    return plots


def bins_of(grid):
    return (grid, grid) if isinstance(grid, int) else tuple(grid)


def genome_tuples(case):
    seq = genomes.records(case["genome"])[0][1]
    fac = oracle.factorize_dna_w_rc(seq) if case["with_rc"] else [f + (False,) for f in oracle.factorize(seq)]
    return [f for f in fac if f[1] >= case["min_factor_length"]]


def synthetic_tuples(case):
    return [(f[0], f[1], f[2], bool(f[3]) if len(f) == 4 else False) for f in case["factors"] if len(f) in (3, 4)]


def ok_cases():
    for c in FX["genome"]:
        yield f"{c['genome']}-{'rc' if c['with_rc'] else 'plain'}-{c['grid']}-{c['total_length']}-{c['min_factor_length']}", c
    for c in FX["synthetic"]:
        if "ok" in c:
            yield c["name"], c


OK_CASES = list(ok_cases())


def fixture_grids(ok):
    yb, xb = ok["shape"]
    fw, rc, bias = np.zeros((yb, xb)), np.zeros((yb, xb)), np.zeros((yb, xb))
    mask = np.ones((yb, xb), dtype=bool)
    for y, x, f, r, b in ok["cells"]:
        fw[y, x], rc[y, x], bias[y, x], mask[y, x] = f, r, b, False
    assert int(mask.sum()) == ok["masked"]
    return fw, rc, bias, mask


def extents_of(factors, total):
    if total is not None:
        return total, total
    return max(s + l for s, l, *_ in factors), max(r + l for _, l, r, *_ in factors)


@pytest.mark.parametrize("name,case", OK_CASES, ids=[n for n, _ in OK_CASES])
def test_model_matches_reference(name, case):
    factors = genome_tuples(case) if "genome" in case else synthetic_tuples(case)
    if "z_used" in case:
        assert len(factors) == case["z_used"]
    xb, yb = bins_of(case["grid"])
    total = case["total_length"]
    ok = case["ok"]
    assert ok["shape"] == [yb, xb] and ok["n_x_edges"] == xb + 1 and ok["n_y_edges"] == yb + 1
    ref_fw, ref_rc, _, _ = fixture_grids(ok)
    mf, mr, unit = model.exact_grid(factors, xb, yb, total)
    fw, rc = model.dense(mf, xb, yb), model.dense(mr, xb, yb)
    # the vectorised single-cell path gives the same integers
    arr = np.array([(s, l, r) for s, l, r, _ in factors], dtype=np.uint64).reshape(-1, 3)
    flags = np.array([bool(f[3]) for f in factors], dtype=bool)
    ffw, frc, x_max, y_max = model.exact_grid_fast(arr[:, 0], arr[:, 1], arr[:, 2], flags, xb, yb, total)
    assert np.array_equal(ffw, fw) and np.array_equal(frc, rc)
    assert (x_max, y_max) == extents_of(factors, total)
    assert ok["x_edges"] == list(np.linspace(0, float(x_max), xb + 1)[[0, 1, -1]])
    assert ok["y_edges"] == list(np.linspace(0, float(y_max), yb + 1)[[0, 1, -1]])
    got_fw, got_rc = model.units_to_float(fw, unit), model.units_to_float(rc, unit)
    # per-strand sums: exact in the model; the reference's float sums agree to rounding
    if x_max % xb == 0 and y_max % yb == 0:
        # every edge an integer: every float of the reference is an exact integer below 2^53
        assert np.array_equal(got_fw, ref_fw) and np.array_equal(got_rc, ref_rc)
        assert not (fw % np.uint64(unit)).any() and not (rc % np.uint64(unit)).any()
    else:
        # each part's length is a difference of two float64 values of magnitude at most x_max
        bound = 4 * 2.0 ** -52 * x_max * (len(factors) + 1)
        assert bound < 1 / (4 * unit), "reference-float fixtures stay where a wrong move of 1 / unit shows"
        diff = max(np.abs(got_fw - ref_fw).max(), np.abs(got_rc - ref_rc).max())
        print(f"{name}: max |model - reference| = {diff:.3g} (bound {bound:.3g})")
        assert diff <= bound


@pytest.mark.parametrize("name,case", OK_CASES, ids=[n for n, _ in OK_CASES])
def test_bias_from_fixture_grids(plots, name, case):
    fw, rc, bias, mask = fixture_grids(case["ok"])
    got = plots.bias_from_grids(fw, rc)
    assert isinstance(got, np.ma.MaskedArray) and got.shape == fw.shape
    assert np.array_equal(np.ma.getmaskarray(got), mask)
    np.testing.assert_array_max_ulp(got.data[~mask], bias[~mask], maxulp=8)


def test_units_to_float_is_exact_on_integer_edges(plots):
    seen = 0
    for name, case in OK_CASES:
        factors = genome_tuples(case) if "genome" in case else synthetic_tuples(case)
        xb, yb = bins_of(case["grid"])
        x_max, y_max = extents_of(factors, case["total_length"])
        if x_max % xb or y_max % yb:
            continue
        seen += 1
        mf, mr, unit = model.exact_grid(factors, xb, yb, case["total_length"])
        ref_fw, ref_rc, _, _ = fixture_grids(case["ok"])
        assert np.array_equal(plots.units_to_grid(model.dense(mf, xb, yb), unit), ref_fw), name
        assert np.array_equal(plots.units_to_grid(model.dense(mr, xb, yb), unit), ref_rc), name
    assert seen >= 5
    # fractions: k / unit nucleotides come back as the nearest float64 of whole + fraction
    u = np.array([[0, 1, 2500, 2501, (1 << 40) * 2500 + 1]], dtype=np.uint64)
    got = plots.units_to_grid(u, 2500)
    assert got.tolist() == [[0.0, 1 / 2500, 1.0, 1.0 + 1 / 2500, float(1 << 40) + 1 / 2500]]


def test_position_ladder_is_numpy_linspace():
    from nolzss_amd import _noLZSS as native
    rng = np.random.default_rng(20)
    pairs = [(1, 50), (49, 50), (50, 50), (51, 50), (999_999, 50), (1_000_000, 50), (1_000_001, 50), (2 ** 32 - 1, 4295)]
    pairs += [(int(g), int(nb)) for g, nb in zip(rng.integers(1, 2 ** 32, 1500), rng.integers(1, 5000, 1500))]
    for genome_end, nb in pairs:
        got = native.debug_position_edges(genome_end, nb, 2 ** 40)  # (bin_bp so large that min_bins decides)
        assert got.tobytes() == np.linspace(0, genome_end, nb + 1).tobytes(), (genome_end, nb)
    # the reference's bin count: max(50, int(np.ceil(genome_end / genome_bin_bp)))
    for genome_end, bp in [(39_936, 1_000_000), (123_456_789, 1_000_000), (4_000_000_000, 1_000_000),
                           (5_000_000, 100_000), (5_000_001, 100_000), (77, 1)] + \
            [(int(g), int(b)) for g, b in zip(rng.integers(1, 2 ** 32, 1500), rng.integers(1, 3_000_000, 1500))]:
        nb = max(50, int(np.ceil(genome_end / bp)))
        if nb > 1 << 20:
            with pytest.raises(ValueError):
                native.debug_position_edges(genome_end, 50, bp)
            continue
        got = native.debug_position_edges(genome_end, 50, bp)
        assert got.tobytes() == np.linspace(0, genome_end, nb + 1).tobytes(), (genome_end, bp)
    for bad in [(0, 50, 1_000_000), (10, 50, 0)]:
        with pytest.raises(ValueError):
            native.debug_position_edges(*bad)


@pytest.mark.parametrize("base", [2.0, 10.0, 1.5, float(np.e)])
def test_length_ladder_slices_are_the_reference_ladders(plots, base):
    ladder = plots.length_ladder(base)
    assert ladder[0] == 1.0 and ladder[-1] >= 2.0 ** 32 and len(ladder) <= 4097
    rng = np.random.default_rng(5)
    for _ in range(300):
        lo, hi = sorted(rng.integers(1, 2 ** 32, 2).tolist())
        min_log = np.floor(np.log(lo) / np.log(base))
        max_log = np.ceil(np.log(hi) / np.log(base))
        n = int((max_log - min_log) * 4)
        ref = base ** np.linspace(min_log, max_log, n + 1)  # plots.py:2584-2590
        assert ladder[4 * int(min_log):4 * int(max_log) + 1].tobytes() == ref.tobytes(), (lo, hi)
    with pytest.raises(ValueError):
        plots.length_ladder(1.0)
    with pytest.raises(ValueError):
        plots.length_ladder(1.001)


def test_argument_checks_need_no_device(plots):
    for c in FX["synthetic"]:
        if "exc" not in c:
            continue
        grid = c["grid"]
        with pytest.raises(Exception) as e:
            plots.factors_strand_bias_grid([tuple(f) for f in c["factors"]], grid_size=grid,
                                           total_length=c["total_length"])
        assert type(e.value).__name__ == c["exc"] and str(e.value) == c["msg"], c["name"]
        if c["factors"]:  # the same checks in front of the text and FASTA forms
            with pytest.raises(Exception) as e:
                plots.strand_bias_grid(b"ACGT", grid_size=grid, total_length=c["total_length"])
            assert type(e.value).__name__ == c["exc"] and str(e.value) == c["msg"], c["name"]
    assert issubclass(plots.PlotError, __import__("nolzss_amd").utils.NoLZSSError)
    with pytest.raises(FileNotFoundError):
        plots.fasta_strand_bias_grid("/nonexistent/in.fa")
    with pytest.raises(ValueError):
        plots.space_scale_histogram()
    with pytest.raises(ValueError):
        plots.space_scale_histogram(b"ACGT", factors=[(0, 1, 0)])
    with pytest.raises(ValueError):
        plots.space_scale_histogram(b"ACGT", genome_bin_size=0.0)
    with pytest.raises(ValueError):
        plots.space_scale_histogram(b"ACGT", length_log_base=1.0)
    with pytest.raises(plots.PlotError):
        plots.space_scale_histogram(factors=[])
    import noLZSS.genomics.plots as ref_named
    assert ref_named.strand_bias_grid is plots.strand_bias_grid and ref_named.PlotError is plots.PlotError


def test_request_refusals_before_any_device_work():
    """bins 0 or 4097, unsorted or too few edges: refused from the request alone (no device is opened)"""
    from nolzss_amd import _noLZSS as native
    recs = np.array([[0, 4, 0]], dtype=np.uint64)
    for grid in [(0, 5), (5, 0), (4097, 1), (1, 4097)]:
        with pytest.raises(ValueError, match="between 1 and 4096"):
            native.records_factor_maps(recs, grid=grid)
    for edges in ([1.0], [1.0, 3.0, 2.0], [1.0, float("nan")], [1.0, float("inf")], np.arange(4098.0)):
        with pytest.raises(ValueError, match="length_edges"):
            native.records_factor_maps(recs, length_edges=edges, position_edges=[0.0, 1.0])
    with pytest.raises(ValueError, match="position_edges"):
        native.records_factor_maps(recs, length_edges=[1.0, 2.0], position_edges=[2.0, 1.0])
    with pytest.raises(ValueError, match="total_length"):
        native.records_factor_maps(recs, grid=(2, 2), total_length=(1 << 33) + 1)
