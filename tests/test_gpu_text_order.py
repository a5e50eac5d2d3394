"""The permutation that brings the L* codes into text order and delivers the inverse suffix array (bucketed_scatter,
two-value form): the packed look-back partition against the histogram form it replaced (NOLZSS_TEXT_ORDER_HIST), each
in a child process of its own, and against the oracle once.  The path needs more than 2^24 symbols and a suffix array
that the direct rounds finish (the inverse suffix array is then left to this permutation); every case asserts that it
ran, from the NOLZSS_TRACE lines.  (A text with a copy long enough to escape without the knob -- L* of 2^20 or more at
these sizes -- is finished by the pair runs, not the direct rounds, and never reaches this permutation: the escape is
exercised through NOLZSS_TEXT_ORDER_ESC instead.)"""
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import gen
import oracle_lib as oracle

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent

CHILD = r"""
import sys
import numpy as np
sys.path[:0] = [sys.argv[1], sys.argv[1] + "/tests"]
import gen
from nolzss_amd import _noLZSS as native
kind, n, out = sys.argv[2], int(sys.argv[3]), sys.argv[4]
t = gen.random_dna(n) if kind == "random" else gen.repeat_dna(n)
native.set_device(0)
d = native.debug_arrays(t)
np.savez(out, isa=d["isa"], lstar=d["lstar"])
"""

RANDOM_N = (1 << 25) + 12345
PACKED = "text order: packed look-back partition"
DIRECT = "suffix array finished by the direct rounds"


def run(tmp_path, kind, n, **env):
    out = tmp_path / f"{kind}_{len(list(tmp_path.iterdir()))}.npz"
    e = dict(os.environ, NOLZSS_TRACE="1", **env)
    r = subprocess.run([sys.executable, "-c", CHILD, str(ROOT), kind, str(n), str(out)], env=e, capture_output=True,
                       text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-4000:]
    d = np.load(out)
    return d["isa"], d["lstar"], r.stderr


def escaped(stderr):
    line = next(s for s in stderr.splitlines() if PACKED in s)
    return int(line.split(PACKED + ", ")[1].split()[0]), line


def same_as_hist_form(tmp_path, kind, n, **env):
    isa, lstar, err = run(tmp_path, kind, n, **env)
    assert DIRECT in err and PACKED in err, err[-4000:]
    isa0, lstar0, err0 = run(tmp_path, kind, n, NOLZSS_TEXT_ORDER_HIST="1")
    assert PACKED not in err0
    assert np.array_equal(isa, isa0), "inverse suffix array"
    assert np.array_equal(lstar, lstar0), "L*"
    return err, lstar0


def test_random_dna(tmp_path):
    err, _ = same_as_hist_form(tmp_path, "random", RANDOM_N)
    assert "overflow" not in escaped(err)[1]


def test_repeat_dna(tmp_path):
    err, _ = same_as_hist_form(tmp_path, "repeat", 1 << 26)
    assert "overflow" not in escaped(err)[1]


def test_many_exceptions(tmp_path):
    # the threshold at which at most n / 256 final L* values reach it: the codes before the far and exact searches
    # are never larger, so the list (n / 64 entries) cannot overflow, and plenty of codes escape
    n = 1 << 26
    _, lstar0, _ = run(tmp_path, "repeat", n, NOLZSS_TEXT_ORDER_HIST="1")
    v = np.sort(lstar0)
    thr = int(v[n - n // 256]) + 1
    isa, lstar, err = run(tmp_path, "repeat", n, NOLZSS_TEXT_ORDER_ESC=str(thr))
    assert DIRECT in err and PACKED in err
    cnt, line = escaped(err)
    assert "overflow" not in line and cnt >= 10000, line
    isa0, _, _ = run(tmp_path, "repeat", n, NOLZSS_TEXT_ORDER_HIST="1")
    assert np.array_equal(isa, isa0)
    assert np.array_equal(lstar, lstar0)


def test_exception_list_overflow(tmp_path):
    err, _ = same_as_hist_form(tmp_path, "random", RANDOM_N, NOLZSS_TEXT_ORDER_ESC="1")
    assert "list overflow, histogram form instead" in escaped(err)[1]


def test_against_oracle(tmp_path):
    n = (1 << 24) + 4097
    isa, lstar, err = run(tmp_path, "random", n)
    assert DIRECT in err and PACKED in err
    t = gen.random_dna(n)
    sa = oracle.suffix_array(t)
    ref = np.empty(n, dtype=np.int64)
    ref[sa] = np.arange(n)
    assert np.array_equal(isa.astype(np.int64), ref), "inverse suffix array"
    ln, _ = oracle.lpnf_all(t)
    got = lstar.astype(np.int64)
    assert np.array_equal(np.where(got == 0, 1, got), ln.astype(np.int64)), "L*"
