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
def copies(n):
    # four copies of one random text that differ from each other at every 2000th base: groups of four suffixes tied
    # up to 2000 bases deep, half of them beyond the 1024 bases of the direct round
    L = n // 4
    y = gen.random_dna(L, 17)
    bases = np.frombuffer(b"ACGT", dtype=np.uint8)
    at = np.arange(1000, L, 2000)
    parts = [y]
    for c in (1, 2, 3):
        z = y.copy()
        z[at] = bases[(np.searchsorted(bases, y[at]) + c) % 4]
        parts.append(z)
    return np.concatenate(parts + [y[:n - 4 * L]])
t = gen.random_dna(n) if kind == "random" else copies(n) if kind == "copies" else gen.repeat_dna(n)
native.set_device(0)
if sys.argv[5:] == ["sa"]:
    native.profile_enable(True)
d = native.debug_arrays(t)
if sys.argv[5:] == ["sa"]:  # the suffix array too, and (launches, bytes) of the stages that name a form
    rep = native.profile_report()
    stages = np.array([rep.get(k, (0, 0.0, 0.0))[::2] for k in ("window_scatter", "bucket_scatter")], dtype=np.float64)
    np.savez(out, isa=d["isa"], lstar=d["lstar"], sa=d["sa"], stages=stages)
else:
    np.savez(out, isa=d["isa"], lstar=d["lstar"])
"""

RANDOM_N = (1 << 25) + 12345
PACKED = "text order: packed look-back partition"
DIRECT = "suffix array finished by the direct rounds"


def run(tmp_path, kind, n, want_sa=False, **env):
    out = tmp_path / f"{kind}_{len(list(tmp_path.iterdir()))}.npz"
    e = dict(os.environ, NOLZSS_TRACE="1", **env)
    r = subprocess.run([sys.executable, "-c", CHILD, str(ROOT), kind, str(n), str(out)] + (["sa"] if want_sa else []), env=e,
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-4000:]
    d = np.load(out)
    return (d["isa"], d["lstar"], r.stderr) + ((d["sa"], d["stages"]) if want_sa else ())


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


SMALLEST_BIG = (1 << 24) + 4097  # the forms behind `big` need more than 2^24 targets: no multiple of a tile or a window


def one_value_form_against_hist_child(tmp_path, kind, **env):
    """The single-value forms of bucketed_scatter (text_order.hip) at the smallest size that takes them: the inverse
    suffix array must invert the suffix array, and L* must equal that of the NOLZSS_TEXT_ORDER_HIST=1 child, which
    sorts the same text on the default path."""
    n = SMALLEST_BIG
    isa, lstar, err, sa, stages = run(tmp_path, kind, n, want_sa=True, **env)
    assert PACKED not in err, err[-4000:]
    assert np.array_equal(isa[sa], np.arange(n, dtype=isa.dtype)), "isa[sa]"
    _, lstar0, _ = run(tmp_path, kind, n, NOLZSS_TEXT_ORDER_HIST="1")
    assert np.array_equal(lstar, lstar0), "L*"
    return err, stages


def test_window_permutation_of_one_value(tmp_path):
    """rank[] scattered although the direct rounds finish (NOLZSS_NO_DEFER_ISA): write_all_ranks and the permutation of
    the codes each carry one value over a permutation of more than 2^24 targets -- two partition passes, the second
    through radix_pass_low16 (radix_sort.hip), and the windows."""
    err, stages = one_value_form_against_hist_child(tmp_path, "random", NOLZSS_NO_DEFER_ISA="1")
    assert DIRECT not in err
    # both permutations took the windows, and of the forms that end in them only this one accounts 10 bytes per pair
    # (the two-value forms 18, the packed form 16)
    launches, nbytes = stages[0]
    assert launches >= 2 and nbytes == 10.0 * SMALLEST_BIG * launches, stages


def test_partial_scatter_of_changed_ranks(tmp_path):
    """Groups of four suffixes tied up to 2000 bases deep, left to the doubling rounds (no pair runs, no periodic pass,
    no pivot or equalising rounds): the ranks that change in a round, more than 2^22 of them but not all n, go into
    rank[] through the windowed partial scatter and the plain scatter (sa_regroup.hip, regroup)."""
    n = SMALLEST_BIG
    err, stages = one_value_form_against_hist_child(tmp_path, "copies", NOLZSS_PAIR_RUNS_AVG4="0", NOLZSS_NO_PERIODIC="1",
                                                    NOLZSS_NO_PIVOT="1", NOLZSS_NO_EQUALISE="1")
    lines = err.splitlines()
    tied = [int(s.split(":")[1].split()[0]) for s in lines if "direct round (cap" in s][-1:]
    tied += [int(s.split(":")[1].split()[-3]) for s in lines if "doubling round h=" in s]
    assert len(tied) >= 2 and tied[-1] == 0, err[-4000:]  # the doubling rounds ran and finished the suffix array
    # That a round took the form behind `big`: a tie group is the four copies of one position, and the copies differ
    # from each other at every changed base, so a round that reaches it resolves the group entirely and three of its
    # four ranks change.  The plain scatters of this run are those of the rounds (12 bytes per changed rank; nothing
    # here carries a second value, whose scatter would account 8), so their byte count checks that model (chance ties
    # of other sizes allow one in a thousand), and by it the largest round changes 3/4 of the largest drop.
    launches, nbytes = stages[1]
    changed = nbytes / 12.0
    assert 1 <= launches <= len(tied) - 1 and abs(changed - 0.75 * tied[0]) <= tied[0] / 1000, (stages, tied)
    largest = 0.75 * max(a - b for a, b in zip(tied, tied[1:]))
    assert (1 << 22) * 1.001 < largest < n, (largest, tied)
