"""The speculative cursor (chain.hip: chain_spec_walk_kernel, spec_edges_kernel, wyllie_kernel over the tiles,
spec_entries_kernel, chain_spec_fix_kernel and the fall-back of mark_chain) on caller codes, through nolzss_debug_chain:
z, the starts and (32-bit codes) the lengths against the definition of tests/chain_model.py by integer equality, and the
path that ran with the number of failed tiles against what every case of tests/chain_spec_model.py states.
tests/test_chain_spec_host.py shows without a GPU what every input is there for.  At most 131 073 positions per call;
every case with 32-bit codes, and with 16-bit codes (padding poisoned with 0x0000 and with 0xffff) where all codes lie
below 0xffff:
  entry_is_* / merge_*    the walk from the entry lands on a mark at once, at the first hop, and at offsets 1, 63, 64, 1023,
                          1024 and 4095 of the tile, from the offset in front of it and from the head of the tile
  leaves_*                a walk that meets no mark and leaves exactly at the speculative exit (accepted), and one position
                          beside it (the exact stages run)
  twos_* / interleaved_*  L = 2 from an odd start, two interleaved chains with exits tiles apart: fail over, still exact
  jumped_* / lands_* / whole_*   tiles under one long factor, whose speculative marks must all go; a factor that lands 20
                          tiles on; a factor over the whole text
  start_* / n_* / partial_*   start_pos inside a tile with tiles in front, at n - 1; n = 1 .. a tile + 1; a partial last tile
                          entered at its last position
  ramps_* / dense_ramps_* code[i + 1] >= code[i] - 1 as the pipeline's codes: the fast path, no failed tile
  uniform_*               independent codes
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import chain_spec_model as S

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def native():
    from nolzss_amd import _noLZSS as native
    assert native.device_count() >= 1, "no MI355X visible"
    return native


def run_one(native, name, width, poison=0, path=None, failed=None):
    """one call of the hook: the result against the definition, the path against the case (or against path / failed)"""
    c, exp = S.case(name), S.expected(name)
    got = native.debug_chain(c.codes, c.start, width, poison, want_lengths=width == 32, want_hist=False)
    where = (name, width, hex(poison))
    assert got["z"] == exp["z"], (where, got["z"], exp["z"], got["cursor"])
    for key in ("starts",) + (("lengths",) if width == 32 else ()):
        assert got[key].shape == exp[key].shape, (where, key)
        bad = np.nonzero(got[key] != exp[key])[0]
        assert bad.size == 0, (where, key, bad[:8].tolist(), got[key][bad[:8]].tolist(), exp[key][bad[:8]].tolist())
    want = (c.path if path is None else path, c.failed if failed is None else failed)
    assert got["cursor"] == want, (where, got["cursor"], want)
    return got["cursor"]


def run_case(native, name, **kw):
    return [run_one(native, name, width, poison, **kw) for width in S.widths_of(name)
            for poison in ((0, 0xffff) if width == 16 else (0,))]


@pytest.mark.parametrize("name", list(S.CASES))
def test_result_and_path(native, name):
    run_case(native, name)


def test_nothing_to_walk(native):
    codes = S.case("n_65").codes
    for start in (65, 70):
        got = native.debug_chain(codes, start, 32)
        assert got["z"] == 0 and got["cursor"] == ("none", 0)


def test_a_call_on_the_fast_path_behind_one_that_failed_over(native):
    """the flag, the entries and the marks of a call do not reach the next one"""
    for name in ("interleaved_far_exits", "merge_far_4095", "uniform_0_fffe", "ramps_seed31_s4097", "twos_from_odd_start",
                 "n_1", "leaves_beside_spec_exit", "leaves_at_spec_exit"):
        run_case(native, name)


CHILD = r'''
import json, sys
sys.path.insert(0, "tests")
import chain_spec_model as S
import test_gpu_chain_spec as T
from nolzss_amd import _noLZSS as native
assert native.device_count() >= 1, "no MI355X visible"
mode = sys.argv[1]
ran = []
for name in S.CASES:
    c = S.case(name)
    if mode == "exact":
        want = dict(path="exact", failed=0)
    else:  # the tile of start_pos raises the flag on top of the tiles that fail by themselves
        want = dict(path="failed_over", failed=c.failed + 1)
    ran += T.run_case(native, name, **want)
print("RAN " + json.dumps(ran))
'''


@pytest.mark.parametrize("knob, mode", [("NOLZSS_NO_SPEC_CURSOR", "exact"), ("NOLZSS_TEST_SPEC_CURSOR_FAILS", "forced")])
def test_knobs_in_a_child_process(knob, mode):
    """The knobs are frozen at first use: one child per knob, every case checked in the child as above.
    NOLZSS_NO_SPEC_CURSOR: the exact stages alone.  NOLZSS_TEST_SPEC_CURSOR_FAILS: the flag is raised on every input, and
    the exact stages deliver the result."""
    env = dict(os.environ, **{knob: "1"})
    r = subprocess.run([sys.executable, "-c", CHILD, mode], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    lines = [x for x in r.stdout.splitlines() if x.startswith("RAN ")]
    assert r.returncode == 0 and lines, r.stdout[-2000:] + r.stderr[-4000:]
    ran = json.loads(lines[-1][4:])
    assert len(ran) >= 2 * len(S.CASES) and all(p == ("exact" if mode == "exact" else "failed_over") for p, _ in ran)
