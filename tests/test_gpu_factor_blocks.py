"""The factor look-ups over rank blocks (nolzss_amd/csrc/rank_blocks.hpp: SA and LCP of 16 ranks in one line, written by
the candidate kernel, read by factor_block_kernel) against the CPU: per text
  (a) native.debug_position_factors -- the record of EVERY position, through the block look-up in plain mode -- against
      length = the oracle's L*, ref = the leftmost occurrence by brute force (a literal is (i, 1, i));
  (b) native.factorize_array against the oracle's factors.
The texts (tests/rank_block_cases.py) are the smallest at which the blocks can go wrong: lengths around 16, 32, 48, 256
and the candidate kernel's tile (n % 16 in {0, 1, 15}, the block that holds lcp[n], the block behind the last tile); runs
and short periods (the interval is the whole array: both sides leave three blocks and the pyramids take over); one 12-mer
planted 3, 14, 18, 40 and 100 times; two copies of a text; the benchmark generator at 2^16 bases.

The planted 12-mer on the true suffix array (asserted below): 3 occurrences -- the interval and its two stops lie in ONE
block; 14 and 18 -- they straddle TWO; 40 -- they span THREE; 100 -- they exceed three (seven or more) and the pyramids
take the rest."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle_lib as oracle
import rank_block_cases as rb

TEXTS = rb.make_texts()
PLANT_BLOCKS = {3: (1, 1), 14: (2, 2), 18: (2, 2), 40: (3, 3), 100: (4, 99)}  # count -> blocks of the 12-mer's interval


def same(got, exp) -> bool:
    return len(got) == len(exp) and all(np.array_equal(got[f], exp[f]) for f in rb.FIELDS)


@functools.lru_cache(maxsize=None)
def expected(name):
    """(records of every position, the oracle's factors), computed once per text"""
    t = TEXTS[name]
    return rb.expected_positions(t), oracle.factors_array(t)


@functools.lru_cache(maxsize=None)
def big():
    t = rb.big_text()
    sample = rb.big_sample(len(t))
    return t, sample, rb.expected_positions(t, sample), oracle.factors_array(t)


def test_planted_intervals_are_what_the_cases_say():
    """No GPU: the 12-mer's interval on the true suffix array touches the number of blocks the module docstring states,
    and the factors of the planted texts fall in every class: interval in one block, in two, in three, wider."""
    classes = set()
    for count, (least, most) in PLANT_BLOCKS.items():
        t = TEXTS[f"plant{count}"]
        assert t.count(rb.PLANT.encode()) == count
        sa, isa, lcp = rb.true_arrays(t)
        lo, hi = rb.interval(lcp, int(isa[t.find(rb.PLANT.encode())]), len(rb.PLANT))
        assert hi - lo + 1 == count
        assert least <= rb.blocks_touched(lo, hi) <= most, (count, lo, hi)
        _, blocks, _, covered = rb.census(t, oracle.factors_array(t))
        classes |= set(np.minimum(blocks, 4).tolist())
        assert covered.min() == 0 and covered.max() == 1, count  # some factors go to the pyramids, some do not
    assert classes == {1, 2, 3, 4}


@pytest.fixture(scope="module")
def native():
    from nolzss_amd import _noLZSS
    assert _noLZSS.device_count() >= 1, "no MI355X visible"
    return _noLZSS


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(TEXTS))
def test_every_position_and_the_factors(native, name):
    t = TEXTS[name]
    every, factors = expected(name)
    got = native.debug_position_factors(t)
    assert len(got) == len(t)
    for f in rb.FIELDS:
        bad = np.flatnonzero(got[f] != every[f])
        assert len(bad) == 0, (name, f, len(bad), bad[:8].tolist(), got[f][bad[:8]].tolist(), every[f][bad[:8]].tolist())
    assert same(native.factorize_array(t), factors), name


@pytest.mark.gpu
def test_benchmark_generator_64k(native):
    t, sample, every, factors = big()
    got = native.debug_position_factors(t)[sample]
    for f in rb.FIELDS:
        bad = np.flatnonzero(got[f] != every[f])
        assert len(bad) == 0, (f, len(bad), sample[bad[:8]].tolist())
    assert same(native.factorize_array(t), factors)


CHILD = r'''
import sys
import numpy as np
sys.path.insert(0, "tests")
import oracle_lib as oracle
import rank_block_cases as rb
from nolzss_amd import _noLZSS as native
mode, out = sys.argv[1], sys.argv[2]
if mode == "pending":
    texts = rb.make_texts()
    names = ["random16", "random49", "random257", "random1024", "run300", "period5", "plant40", "plant100", "copies_1pct"]
    for name in names:
        t = texts[name]
        exp = oracle.factors_array(t)
        got = native.factorize_array(t)
        assert len(got) == len(exp) and all(np.array_equal(got[f], exp[f]) for f in rb.FIELDS), name
        every = rb.expected_positions(t)
        pos = native.debug_position_factors(t)
        assert all(np.array_equal(pos[f], every[f]) for f in rb.FIELDS), name
    print("ok", len(names))
else:
    got = native.factorize_array(rb.big_text())
    np.save(out, np.stack([got[f] for f in rb.FIELDS]))
    print("ok", len(got))
'''


def _child(mode, out, **env):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", CHILD, mode, str(out)], cwd=root, env=dict(os.environ, NOLZSS_TRACE="1", **env),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
    return r.stderr


@pytest.mark.gpu
def test_blocks_after_the_pending_lcp_rerun(tmp_path):
    """NOLZSS_TEST_INJECT_PENDING leaves one LCP entry undecided: the safety net changes lcp[] and the candidate stage
    runs a second time -- the blocks must hold the final lcp[].  Records of every position and factors against the
    CPU, in a child process (the knob is read once per process); the trace says that the blocks were read."""
    err = _child("pending", tmp_path / "unused.npy", NOLZSS_TEST_INJECT_PENDING="1")
    assert "factor look-ups: rank blocks" in err and "factor look-ups: sa[] and lcp[]" not in err, err[-2000:]


@pytest.mark.gpu
def test_knob_switches_the_blocks_off(native, tmp_path):
    """NOLZSS_NO_RANK_BLOCKS=1: no blocks, the look-ups read sa[] and lcp[] -- and the records equal the default run's."""
    out = tmp_path / "records.npy"
    err = _child("knob", out, NOLZSS_NO_RANK_BLOCKS="1")
    assert "factor look-ups: sa[] and lcp[]" in err and "factor look-ups: rank blocks" not in err, err[-2000:]
    t, _, _, factors = big()
    off = np.load(out)
    got = native.factorize_array(t)
    for k, f in enumerate(rb.FIELDS):
        assert np.array_equal(off[k], got[f]), f
    assert same(got, factors)
