"""Reverse-complement mode at EVERY position against the oracle (tests/rc_positions.py): the codes of rc_tile_kernel,
rc_far_kernel and rc_fallback_kernel, the records of factor_kernel, the plain-mode by-product, and SA / LCP / ISA of the
prepared string -- a factorization reads them on its greedy chain only, one position in hundreds on the texts where
the exact search does nearly all the work.  Plain mode: the record of every position, not only its length."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle_lib as oracle
import rc_positions as rp
from test_gpu_pipeline import CASES as PLAIN_CASES

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def native():
    from nolzss_amd import _noLZSS
    assert _noLZSS.device_count() >= 1, "no MI355X visible"
    return _noLZSS


@pytest.mark.parametrize("want_plain", [False, True], ids=["codes", "codes_and_plain"])
@pytest.mark.parametrize("name", list(rp.all_cases()))
def test_every_position(native, name, want_plain):
    rp.check_every_position(native, rp.all_cases()[name], want_plain, rp.expected(name))


PATHS = {
    "default": {},
    "compact": {"NOLZSS_RC_COMPACT_MIN": "1"},
    "compact_bucketed_sort": {"NOLZSS_DNA_FAST_MIN": "1", "NOLZSS_RC_COMPACT_MIN": "1"},
    "pending_lcp": {"NOLZSS_TEST_INJECT_PENDING": "1"},
    "pair_runs": {"NOLZSS_REFINE_WORDS": "1", "NOLZSS_PIVOT_MIN": "1", "NOLZSS_PAIR_RUNS_MIN": "1"},
}


@functools.lru_cache(maxsize=None)
def _child(path):
    """one child process per environment: the thresholds are function-local statics, read once per process"""
    env = dict(os.environ, **PATHS[path])
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join("tests", "rc_positions.py")], cwd=root, env=env, capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0 and "\nok" in r.stdout, r.stdout[-4000:] + r.stderr[-4000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("COUNTERS ")][0]
    print(path, r.stdout[r.stdout.index("TOTAL "):])
    return json.loads(line[len("COUNTERS "):])


@pytest.mark.parametrize("path", list(PATHS))
def test_every_position_paths(path):
    """The single-sequence, multi-sequence and tile-geometry lists through the checker in one child process per
    environment, and the queue counters of the runs: they say that the far queue, the far-to-exact hand-off, the
    compact output and the repair of an undecided LCP entry really ran on these inputs."""
    report = _child(path)
    assert set(report) == set(rp.all_cases(kats=False))
    assert sum(c["far_ranks"] for c in report.values()) > 0, report
    assert any(c["exact_total"] > c["exact_from_tiles"] for c in report.values()), report  # far-to-exact hand-off
    for name in rp.PERIODIC + rp.PERIODIC_IN_TILES:  # the exact search on nearly every position, through either queue
        assert report[name]["exact_total"] >= 0.9 * report[name]["N"], (name, report[name])
    for name in rp.PERIODIC_IN_TILES:  # ... queued by the tile kernel itself (rc_positions.py says why only these)
        assert report[name]["exact_from_tiles"] >= 0.9 * report[name]["N"], (name, report[name])
    if "NOLZSS_RC_COMPACT_MIN" in PATHS[path]:
        assert any(c["compact"] == 1 for c in report.values()), report
    if path == "default":  # (periodic texts need doubling rounds and stay non-compact in every child)
        assert not any(c["compact"] for c in report.values()), report
    if path == "pending_lcp":
        assert any(c["pending_relaunch"] == 1 for c in report.values()), report


@pytest.mark.parametrize("name", list(PLAIN_CASES))
def test_plain_refs_at_every_position(native, name):
    """factor_kernel's interval search and leftmost-occurrence lookup at every position of the plain-mode cases
    (test_intermediate_arrays compares the lengths; the chain reaches the references of its own positions only)"""
    t = PLAIN_CASES[name]
    n = len(t)
    ln, rf = oracle.lpnf_all(t)
    rec = native.debug_position_factors(t)
    assert len(rec) == n
    for what, got, exp in (("start", rec["start"], np.arange(n)), ("length", rec["length"], ln), ("ref", rec["ref"], rf)):
        bad = np.flatnonzero(got != exp.astype(np.uint64))
        assert bad.size == 0, f"{what}: {bad.size} mismatches, first at {int(bad[0])}: {got[bad[0]]} != {exp[bad[0]]}"
    lit = rec["ref"] == rec["start"]  # a literal has ref = i; a match lies entirely in front of i
    assert (rec["length"][lit] == 1).all()
    assert (rec["ref"][~lit] + rec["length"][~lit] <= rec["start"][~lit]).all()
