#!/usr/bin/env python3
"""Pins the strand-bias grid to what the reference's own Python code produces.

Build container only (never on the GPU box, which has no reference tree): the reference's `noLZSS` package is loaded
by path under a private name with a stub compiled module, exactly as tests/golden/make_significance_fixtures.py does,
and its `genomics.plots._compute_strand_bias_grid` runs on the inputs below.  tests/golden/python_ref_factor_maps.json
records each input and then the observed output (non-zero cells of the two grids, the edges' ends, the unmasked bias
values), or the exception class and message.  Genome cases name their input (genome, mode, grid, total_length,
min_factor_length): the tests rebuild the factors with the CPU oracle.  Synthetic cases carry the factor list itself.
Inputs and observed outputs only: nothing of the reference's text is copied.

"_measured": the largest absolute difference between the reference's float cells and the exact integer model
(tests/factor_maps_model.py) over the cases whose edges are not integers.

    python tests/golden/make_factor_map_fixtures.py     (rewrites tests/golden/python_ref_factor_maps.json)
"""
import importlib
import importlib.util
import json
import sys
import types
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import factor_maps_model as model  # noqa: E402
import genomes  # noqa: E402
import oracle_lib as oracle  # noqa: E402

REF_PKG = Path("/root/reference/src/noLZSS")
OUT = Path(__file__).resolve().parent / "python_ref_factor_maps.json"
PRIVATE = "_reference_noLZSS_plots"

# (genome, with_rc, grid, total_length, min_factor_length)
GENOME_CASES = [
    ("T7", True, 50, None, 1), ("T7", True, 16, 40000, 1),
    ("T7", True, 16, 20000, 1), ("T7", True, 1, None, 1), ("T7", True, [7, 3], 12345, 1),
    ("T7", True, 16, None, 20), ("T7", False, 16, None, 1), ("T3", True, [7, 3], None, 1),
    ("short_dna1", True, [5, 4], None, 1), ("test_bacterial_dna", True, 50, None, 1),
    ("test_bacterial_dna", False, [16, 8], None, 2),
]

SYNTHETIC = [
    # a factor crossing more than 10 cells on each strand (16 x 16 over 1600: cells of 100)
    ("long_crossers", [(0, 5, 0), (5, 1500, 40, False), (1505, 95, 3, True), (40, 1400, 60, True)], 16, None),
    # a reverse-complement factor ending exactly on a y edge (r + length = 400 = 4 * 100), and one starting on it
    ("rc_on_y_edge", [(0, 10, 0), (100, 150, 250, True), (300, 100, 400, True), (1500, 100, 1500)], 16, None),
    # total_length smaller than the coordinates: dropped parts on both strands
    ("dropped_parts", [(0, 300, 100), (250, 400, 500, True), (700, 200, 900), (950, 100, 10, True), (1200, 50, 0)],
     [8, 8], 1000),
    # total_length a multiple of both bin counts: every edge an integer
    ("integer_edges", [(0, 7, 0), (7, 130, 2), (137, 211, 40, True), (348, 100, 348), (448, 64, 0, True)], [8, 4], 512),
    ("non_square_37_64", [(0, 3, 0), (3, 700, 1), (703, 1200, 300, True), (1903, 97, 1000), (2000, 368, 0, True)],
     [37, 64], None),
    ("seven_by_three", [(0, 1, 0), (1, 20, 0), (21, 33, 5, True), (54, 46, 10)], [7, 3], None),
    ("one_by_one", [(0, 1, 0), (1, 9, 0, True), (10, 5, 2)], [1, 1], None),
    ("one_by_one_int", [(0, 1, 0), (1, 9, 0, True), (10, 5, 2)], 1, None),
    # 3-tuples and 4-tuples mixed, other sizes skipped
    # (the 5-tuple lies inside the extents of the others: the reference takes x_max / y_max over every tuple)
    ("mixed_tuples", [(0, 4, 0), (4, 4, 0, False), (8, 6, 1, True), (2, 3, 1, True, 9), (14, 10, 3), (24, 8, 2, True)],
     4, None),
    ("grid_zero", [(0, 4, 0)], 0, None),
    ("grid_negative", [(0, 4, 0)], [4, -1], None),
    ("grid_triple", [(0, 4, 0)], [4, 4, 4], None),
    ("grid_string", [(0, 4, 0)], "50", None),
    ("no_factors", [], 8, None),
    ("zero_total_length", [(0, 4, 0)], 4, 0),
]


def load_reference_plots():
    stub = types.ModuleType(PRIVATE + "._noLZSS")
    stub.__version__ = "0.0.0-stub"
    stub.__getattr__ = lambda name: (lambda *a, **k: None)
    sys.modules[PRIVATE + "._noLZSS"] = stub
    spec = importlib.util.spec_from_file_location(PRIVATE, REF_PKG / "__init__.py",
                                                  submodule_search_locations=[str(REF_PKG)])
    pkg = importlib.util.module_from_spec(spec)
    sys.modules[PRIVATE] = pkg
    spec.loader.exec_module(pkg)
    return importlib.import_module(PRIVATE + ".genomics.plots")


def genome_factors(name, with_rc, min_factor_length):
    """the oracle's factors of the first record of a golden genome, as the tuples the reference works on"""
    seq = genomes.records(name)[0][1]
    if with_rc:
        fac = oracle.factorize_dna_w_rc(seq)
    else:
        fac = oracle.factorize(seq)
    return [f for f in fac if f[1] >= min_factor_length]


def observe(plots, factors, grid, total_length):
    g = tuple(grid) if isinstance(grid, list) else grid
    try:
        xe, ye, fw, rc, bias = plots._compute_strand_bias_grid(factors, g, total_length=total_length)
    except Exception as e:  # noqa: BLE001  (the class is what is recorded)
        return {"exc": type(e).__name__, "msg": str(e)}, None
    mask = np.ma.getmaskarray(bias)
    assert np.array_equal(mask, (fw == 0) & (rc == 0))  # the unmasked cells are the non-zero ones: one list serves
    ys, xs = np.nonzero(~mask)

    def num(v):  # (an integral float is written as an integer: it reads back as the same float64)
        return int(v) if float(v).is_integer() else float(v)

    res = {"shape": list(fw.shape), "x_edges": [float(xe[0]), float(xe[1]), float(xe[-1])],
           "y_edges": [float(ye[0]), float(ye[1]), float(ye[-1])], "n_x_edges": len(xe), "n_y_edges": len(ye),
           "masked": int(mask.sum()),
           # [yi, xi, forward_grid, rc_grid, bias_grid] of every unmasked cell
           "cells": [[int(y), int(x), num(fw[y, x]), num(rc[y, x]), float(bias.data[y, x])]
                     for y, x in zip(ys.tolist(), xs.tolist())]}
    return {"ok": res}, (fw, rc)


def model_difference(factors, grid, total_length, fw, rc):
    xb, yb = (grid, grid) if isinstance(grid, int) else grid
    four = [(f[0], f[1], f[2], f[3] if len(f) == 4 else False) for f in factors if len(f) in (3, 4)]
    mf, mr, unit = model.exact_grid(four, xb, yb, total_length)
    d = 0.0
    for sp, ref in ((mf, fw), (mr, rc)):
        got = model.units_to_float(model.dense(sp, xb, yb), unit)
        d = max(d, float(np.abs(got - ref).max()))
    return d


def main():
    plots = load_reference_plots()
    fx = {"_how": "tests/golden/make_factor_map_fixtures.py: the reference's noLZSS package loaded by path with a stub "
                  "compiled module; _compute_strand_bias_grid on the inputs named here; inputs and observed outputs only",
          "genome": [], "synthetic": [], "_measured": {}}
    worst = 0.0
    for name, with_rc, grid, total, minlen in GENOME_CASES:
        factors = genome_factors(name, with_rc, minlen)
        res, grids = observe(plots, factors, grid, total)
        d = model_difference(factors, grid, total, *grids)
        fx["_measured"][f"{name}/{'rc' if with_rc else 'plain'}/{grid}/{total}/{minlen}"] = d
        worst = max(worst, d)
        fx["genome"].append({"genome": name, "with_rc": with_rc, "grid": grid, "total_length": total,
                             "min_factor_length": minlen, "z_used": len(factors), **res})
    for name, factors, grid, total in SYNTHETIC:
        res, grids = observe(plots, factors, grid, total)
        if grids is not None:
            d = model_difference(factors, grid, total, *grids)
            fx["_measured"]["synthetic/" + name] = d
            worst = max(worst, d)
        fx["synthetic"].append({"name": name, "factors": [list(f) for f in factors], "grid": grid,
                                "total_length": total, **res})
    fx["_measured"]["max"] = worst
    OUT.write_text(json.dumps(fx, indent=None, ensure_ascii=True) + "\n")
    print(f"wrote {OUT} ({OUT.stat().st_size} bytes): {len(fx['genome'])} genome cases, {len(fx['synthetic'])} synthetic "
          f"cases, max |reference - model| = {worst:.3g}")
    for k, v in fx["_measured"].items():
        print(f"  {k}: {v:.3g}")


if __name__ == "__main__":
    sys.exit(main())
