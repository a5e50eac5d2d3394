"""The 16-bit form of the factor-length codes in text order (code16.hpp): window_unpack16_kernel, the writers behind it
(escape fix-up, far and exact kernels) through store_code, the choice from the wide-code list's count, and the cursor
kernels on 16-bit codes with a 16-bit exit.  Every case runs the text in a child process with NOLZSS_TRACE=1, asserts
from the trace that the path under test ran, and compares the inverse suffix array, L* and the factors with a
NOLZSS_NO_CODE16=1 child (32-bit codes throughout) and the factors with the oracle; both references are computed once per
text.  n = 2^24 + 4097 throughout: the packed text-order permutation, which alone writes 16-bit codes, needs more than
2^24 targets, and the size is no multiple of a cursor tile, a window or a pair of codes."""
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
N = (1 << 24) + 4097
TILE = 4096  # positions per workgroup of the cursor kernels (chain.hip: kTile)

PERIOD_UNIT = b"ACGGTCA"
# 1400 bases: the run's suffixes share their first 16 bases, a group too large for the first direct round, and the second
# one finishes such a group only where its ties are shallower than about 1 550 bases (longer runs go to the doubling rounds,
# and the path under test needs a suffix array finished by the direct rounds)
PERIOD_REPEATS = 200


def make_text(kind, n):
    if kind == "random":
        return gen.random_dna(n)
    if kind == "repeat":
        return gen.repeat_dna(n)
    if kind == "far":
        # gen.far_copy with shorter blocks: its copies of up to 20 000 bases leave ties that the doubling rounds finish,
        # and the path under test needs a suffix array finished by the direct rounds (ties up to about 7 600 bases).  Each
        # copy starts 3000 positions into a cursor tile and is 5200 bases or longer, so its factor jumps over the whole
        # of the next tile.
        rng = np.random.default_rng(5)
        t = gen.random_dna(n, 5).copy()
        for _ in range(8):
            ln = int(rng.integers(5200, 7000))
            dst = int(rng.integers(n // 2 // TILE, n // TILE - 4)) * TILE + 3000
            src = int(rng.integers(0, n // 4))
            t[dst:dst + ln] = t[src:src + ln]
        return t
    if kind == "periodic":  # a run of a 7-base unit in random DNA: the best earlier match of a position in it overlaps it
        t = gen.random_dna(n).copy()
        run = np.frombuffer(PERIOD_UNIT * PERIOD_REPEATS, dtype=np.uint8)
        at = n // 2 + 11
        t[at:at + len(run)] = run
        return t
    raise ValueError(kind)


CHILD = r"""
import sys
import numpy as np
sys.path[:0] = [sys.argv[1], sys.argv[1] + "/tests"]
import test_gpu_code16 as me
from nolzss_amd import _noLZSS as native
kind, n, out = sys.argv[2], int(sys.argv[3]), sys.argv[4]
t = me.make_text(kind, n)
native.set_device(0)
d = native.debug_arrays(t)
f = native.factorize_array(t)
np.savez(out, isa=d["isa"], lstar=d["lstar"], start=f["start"], length=f["length"], ref=f["ref"])
"""

DIRECT = "suffix array finished by the direct rounds"
PACKED = "text order: packed look-back partition"
NARROW = "code16: narrow cursor, 0 wide codes"
WIDENED = "code16: widened, "
OVERFLOW = "code16: wide-code list overflow"
FIELDS = ("isa", "lstar", "start", "length", "ref")


def run(tmp_path, kind, **env):
    out = tmp_path / f"{kind}_{len(list(tmp_path.iterdir()))}.npz"
    e = dict(os.environ, NOLZSS_TRACE="1", **env)
    r = subprocess.run([sys.executable, "-c", CHILD, str(ROOT), kind, str(N), str(out)], env=e, capture_output=True, text=True,
                       timeout=900)
    assert r.returncode == 0, r.stderr[-4000:]
    d = np.load(out)
    return {k: d[k] for k in FIELDS}, r.stderr


@pytest.fixture(scope="module")
def references(tmp_path_factory):
    """kind -> the arrays of the NOLZSS_NO_CODE16=1 child, checked against the oracle's factors (once per text)"""
    cache = {}

    def get(kind):
        if kind not in cache:
            ref, err = run(tmp_path_factory.mktemp("ref_" + kind), kind, NOLZSS_NO_CODE16="1")
            assert DIRECT in err and PACKED in err and "code16:" not in err, err[-4000:]
            exp = oracle.factors_array(make_text(kind, N).tobytes())
            assert len(exp) == len(ref["start"])
            for k in ("start", "length", "ref"):
                assert np.array_equal(ref[k], exp[k]), f"32-bit arm against the oracle: {k}"
            cache[kind] = ref
        return cache[kind]

    return get


def check(tmp_path, references, kind, form, **env):
    ref = references(kind)
    got, err = run(tmp_path, kind, **env)
    assert DIRECT in err and PACKED in err, err[-4000:]
    assert form in err, err[-4000:]
    for k in FIELDS:  # (the reference arm's factors are the oracle's: references)
        assert np.array_equal(got[k], ref[k]), k
    return err


def listed(err, marker):
    line = next(s for s in err.splitlines() if marker in s)
    return int(line.split(marker)[1].split()[0]), line


@pytest.mark.parametrize("kind", ["random", "repeat"])
def test_narrow_cursor(tmp_path, references, kind):
    check(tmp_path, references, kind, NARROW)


def test_far_copies_jump_over_tiles(tmp_path, references):
    """copies of 5200 to 7000 bases from far back: factors that jump over whole 4096-position tiles (the 16-bit exit, the
    tiles chain_mark_kernel skips), codes written by the far kernels"""
    ref = references("far")
    start, end = ref["start"].astype(np.int64), ref["start"].astype(np.int64) + ref["length"].astype(np.int64)
    assert int(((start // TILE + 2) * TILE <= end).sum()) >= 4  # factors with a whole tile between start and end
    err = check(tmp_path, references, "far", NARROW)
    far = next(s for s in err.splitlines() if "ranks to the far queue" in s)
    assert int(far.split("lpf:")[1].split()[0]) > 0, far


def test_wide_codes_from_the_far_writers(tmp_path, references):
    ref = references("far")
    wide = int((ref["lstar"] >= 1000).sum())
    assert 0 < wide <= N // 64, wide
    err = check(tmp_path, references, "far", WIDENED, NOLZSS_CODE16_MAX="1000")
    assert listed(err, WIDENED)[0] >= wide  # (a position may be listed twice)


def test_wide_codes_from_the_windows(tmp_path, references):
    ref = references("repeat")
    thr = int(np.sort(ref["lstar"])[N - N // 4096]) + 1
    wide = int((ref["lstar"] >= thr).sum())
    assert 0 < wide <= N // 64, (thr, wide)
    err = check(tmp_path, references, "repeat", WIDENED, NOLZSS_CODE16_MAX=str(thr))
    assert listed(err, WIDENED)[0] >= wide


def test_list_overflow_reruns_with_32_bit_codes(tmp_path, references):
    err = check(tmp_path, references, "random", OVERFLOW, NOLZSS_CODE16_MAX="2")
    assert NARROW not in err and WIDENED not in err


def test_saturated_bound_of_the_exact_search(tmp_path, references):
    """in the periodic run the exact search starts from a bound that was stored saturated and appends its result behind the
    bound's own entry: the larger of the two must win"""
    ref = references("periodic")
    assert ref["lstar"].max() >= len(PERIOD_UNIT) * PERIOD_REPEATS // 2 - 8
    err = check(tmp_path, references, "periodic", WIDENED, NOLZSS_CODE16_MAX="64")
    exact = next(s for s in err.splitlines() if "positions to the exact search so far" in s)
    assert int(exact.split("far queue,")[1].split()[0]) > 0, exact
