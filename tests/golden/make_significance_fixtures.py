#!/usr/bin/env python3
"""Pins the factor-length significance analysis to what the reference's own Python code produces.

Build container only (never on the GPU box, which has no reference tree): the reference's `noLZSS` package is loaded
by path under a private name with a stub compiled module (every name a no-op: the significance functions use none of
them), and its `clopper_pearson_upper`, `infer_length_significance`, `extract_factor_lengths` and
`calculate_factor_length_threshold` run on the inputs below.  tests/golden/python_ref_significance.json records each
input and then every returned field, the warnings, or the exception class and message (file paths replaced by
"{path}").  v2 factor files are written by the host-only nolzss_write_factor_file and recorded as bytes.  Inputs and
observed outputs only: nothing of the reference's text is copied.

tests/test_significance_host.py (CPU suite) replays the entries through nolzss_amd.genomics.significance.

    python tests/golden/make_significance_fixtures.py      (rewrites tests/golden/python_ref_significance.json)
"""
import ctypes as C
import importlib.util
import json
import sys
import tempfile
import types
import warnings
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))

REF_PKG = Path("/root/reference/src/noLZSS")
OUT = Path(__file__).resolve().parent / "python_ref_significance.json"
PRIVATE = "_reference_noLZSS_sig"

CP_GRID = [(k, n, a) for n in (1, 2, 7, 100, 1000, 123457) for k in sorted({0, 1, n // 3, n // 2, n - 1, n})
           for a in (0.05, 0.01, 0.2)] + [
    (0, 0, 0.05), (1, -3, 0.05), (-1, 10, 0.05), (11, 10, 0.05), (3, 10, 0.0), (3, 10, 1.0), (3, 10, -0.5),
    (3, 10, 1.5)]


def _rng_lengths(seed, n, p):
    return (np.random.default_rng(seed).geometric(p, n)).tolist()


INFER = [
    ("docstring", [5, 10, 15, 20, 25], [2, 3, 4, 5, 6, 7, 8, 9, 10], {"tau_expected_fp": 0.5}),
    ("defaults", [5, 10, 15, 20, 25], [2, 3, 4, 5, 6, 7, 8, 9, 10], {}),
    ("ties", [3, 3, 3, 7, 7, 1, 1, 12], [1, 1, 1, 2, 2, 3, 3, 3, 3, 5, 5, 8], {"tau_expected_fp": 2.0}),
    ("real_longer_than_all", [40, 50, 2, 60], [1, 2, 2, 3, 4], {"tau_expected_fp": 10.0}),
    ("empty_real", [], [1, 2, 3, 3], {}),
    ("empty_shuffled", [1, 2, 3], [], {}),
    ("arrays", "np:[4, 9, 1, 30]", "np:[1, 1, 2, 3, 5, 8, 13, 21]", {"tau_expected_fp": 0.3, "alpha_cp": 0.01}),
    ("single_shuffled", [1, 2], [7], {}),
    ("all_real_below", [1, 1, 1], [2, 3, 4, 5], {"tau_expected_fp": 100.0}),
    ("geometric_large", _rng_lengths(11, 4000, 0.08), _rng_lengths(12, 5000, 0.1), {"tau_expected_fp": 1.0}),
    ("geometric_alpha", _rng_lengths(13, 3000, 0.05), _rng_lengths(14, 3500, 0.12),
     {"tau_expected_fp": 0.5, "alpha_cp": 0.2}),
]
P_AT = [0, 1, 2, 2.5, 3, 5, 7.5, 10, 20, 1000]

EXTRACT_LISTS = [
    ("tuples", [(0, 5, 0), (5, 3, 2), (8, 10, 1)]),
    ("four_tuples", [(0, 1, 0, False), (1, 4, 0, True)]),
    ("two_tuples", [(0, 2), (2, 9)]),
    ("empty", []),
    ("bad_list_element", [(0, 1, 0), [1, 1, 0]]),
    ("short_tuple", [(0, 1, 0), (1,)]),
]
EXTRACT_OTHER = [("int", 5), ("tuple", ((0, 1, 0),)), ("none", None)]

FILES = {
    "small": [(0, 1, 0), (1, 1, 1), (2, 3, 0), (5, 7, 1), (12, 2, 3)],
    "shuf_small": [(0, 1, 0), (1, 2, 0), (3, 1, 3), (4, 1, 4), (5, 2, 1), (7, 1, 7), (8, 3, 2)],
    "rc_flags": [(0, 1, 0), (1, 4, (1 << 63) | 0), (5, 2, 1), (7, 9, (1 << 63) | 3)],
    "empty": [],
}


def load_reference_significance():
    stub = types.ModuleType(PRIVATE + "._noLZSS")
    stub.__version__ = "0.0.0-stub"
    stub.__getattr__ = lambda name: (lambda *a, **k: None)
    sys.modules[PRIVATE + "._noLZSS"] = stub
    spec = importlib.util.spec_from_file_location(PRIVATE, REF_PKG / "__init__.py",
                                                  submodule_search_locations=[str(REF_PKG)])
    pkg = importlib.util.module_from_spec(spec)
    sys.modules[PRIVATE] = pkg
    spec.loader.exec_module(pkg)
    return importlib.import_module(PRIVATE + ".genomics.significance")


def _arg(x):
    if isinstance(x, str) and x.startswith("np:"):
        return np.array(json.loads(x[3:]), dtype=np.int64)
    return x


def _plain(v):
    if isinstance(v, np.ndarray):
        return v.tolist()
    if isinstance(v, (np.integer,)):
        return int(v)
    if isinstance(v, (np.floating,)):
        return float(v)
    return v


def outcome(fn, post, tmp=None):
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        try:
            res = {"ok": post(fn())}
        except Exception as e:  # noqa: BLE001  (the class is what is recorded)
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


def write_v2(path, factors):
    from nolzss_amd._lib import lib, check, Factor
    arr = (Factor * max(len(factors), 1))(*[Factor(*f) for f in factors])
    total = sum(f[1] for f in factors)
    check(lib.nolzss_write_factor_file(str(path).encode(), arr, len(factors), 1, 0, total, None, 0))


def main():
    sig = load_reference_significance()
    fx = {"_how": "tests/golden/make_significance_fixtures.py: the reference's noLZSS package loaded by path with a "
                  "stub compiled module; inputs and observed outputs only", "p_at": P_AT}
    fx["clopper_pearson_upper"] = [{"k": k, "n": n, "alpha": a,
                                    **outcome(lambda: sig.clopper_pearson_upper(k, n, a), float)}
                                   for k, n, a in CP_GRID]
    fx["infer"] = []
    for name, real, shuf, kw in INFER:
        fx["infer"].append({"name": name, "real": real, "shuf": shuf, "kwargs": kw,
                            **outcome(lambda: sig.infer_length_significance(_arg(real), _arg(shuf), **kw),
                                      infer_fields)})
    fx["extract_lists"] = [{"name": name, "factors": [list(f) if isinstance(f, tuple) else {"list": f} for f in facs],
                            **outcome(lambda: sig.extract_factor_lengths(facs), _plain)}
                           for name, facs in EXTRACT_LISTS]
    fx["extract_other"] = [{"name": name, **outcome(lambda: sig.extract_factor_lengths(v), _plain)}
                           for name, v in EXTRACT_OTHER]
    with tempfile.TemporaryDirectory() as td:
        td = Path(td)
        files = {}
        for name, facs in FILES.items():
            write_v2(td / (name + ".bin"), facs)
            files[name] = (td / (name + ".bin")).read_bytes()
        files["bad_magic"] = files["small"][:-48] + b"notLZSS!" + files["small"][-40:]
        files["too_small"] = b"abc"
        files["truncated"] = files["small"][:24] + files["small"][-48:]
        for name, data in files.items():
            (td / (name + ".bin")).write_bytes(data)
        fx["files"] = {name: data.hex() for name, data in files.items()}
        fx["extract_files"] = [{"file": name, **outcome(lambda: sig.extract_factor_lengths(str(td / (name + ".bin"))),
                                                        _plain, td)}
                               for name in list(files) + ["missing"]]
        fx["extract_files"].append({"file": "small", "as_path": True,
                                    **outcome(lambda: sig.extract_factor_lengths(td / "small.bin"), _plain, td)})
        pairs = [("small", "shuf_small", {}), ("small", "shuf_small", {"tau_expected_fp": 3.0}),
                 ("rc_flags", "small", {"alpha_cp": 0.01}), ("shuf_small", "small", {"tau_expected_fp": 0.01}),
                 ("empty", "small", {}), ("small", "empty", {}), ("missing", "small", {}), ("small", "missing", {}),
                 ("bad_magic", "small", {})]
        fx["threshold"] = [{"real": r, "shuf": s, "kwargs": kw,
                            **outcome(lambda: sig.calculate_factor_length_threshold(
                                str(td / (r + ".bin")), str(td / (s + ".bin")), **kw), infer_fields, td)}
                           for r, s, kw in pairs]
    OUT.write_text(json.dumps(fx, indent=None, ensure_ascii=True) + "\n")
    print(f"wrote {OUT}: {len(fx['clopper_pearson_upper'])} bounds, {len(fx['infer'])} inference cases, "
          f"{len(fx['threshold'])} threshold cases")


if __name__ == "__main__":
    sys.exit(main())
