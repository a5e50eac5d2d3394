"""The 35-bit key of the round-0 sort (text.hpp, kP35Syms): plain one-segment DNA whose sub-buckets are sorted in LDS
takes the stored word [27 key bits][5-bit tag] and two LDS digits of 10 and 9 bits.  It normally starts at 2^28 bases;
child processes with NOLZSS_DNA_FAST_MIN=1 NOLZSS_LOCAL_SORT_MIN=1 NOLZSS_LOCAL_REGROUP_MIN=1 send small texts through
it -- the smallest shapes at which the new layout can go wrong -- and every text is compared record for record with
the oracle.  The trace line of every text proves which layout it took."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import gen

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MIN_KEY35 = 32  # (key16_applicable: shorter texts take the general sort)
KMER = b"ACGTTGCT"  # the 8-mer of the sub-bucket filled to just below a workgroup's capacity (18 432 pairs)


def _lcp(t: np.ndarray, p: int, q: int) -> int:
    m = min(len(t) - p, len(t) - q)
    d = np.nonzero(t[p:p + m] != t[q:q + m])[0]
    return int(d[0]) if len(d) else m


def boundary_pairs_text(n: int, seed: int):
    """random DNA with pairs of suffixes whose longest common prefix is exactly 15 .. 19 bases: two copies of a random
    block, different bases behind them -- for every length the pairs A/G and C/T (the bases differ in their high bit)
    and A/C and G/T (in the low bit only: at 17 bases that is the half base of the key).  Returns the text and the
    planted (position, position, length) triples."""
    rng = np.random.default_rng(seed)
    t = gen.random_dna(n, seed).copy()
    plants = []
    at = 64
    for length in (15, 16, 17, 18, 19):
        for a, b in (b"AG", b"CT", b"AC", b"GT"):
            block = gen.ACGT[rng.integers(0, 4, size=length)]
            p, q = at, at + 48
            t[p:p + length] = block
            t[q:q + length] = block
            t[p + length], t[q + length] = a, b
            plants.append((p, q, length))
            at += 96
    assert at + 64 < n
    return t, plants


def end_of_text_cases():
    """texts ending in a run of k A's behind random DNA, n around the smallest text of the layout and around a tile: the
    zero-padded keys of the short suffixes collide with the keys of longer runs of A elsewhere (a run of 20 in the middle
    where there is room)"""
    out = []
    for n in (32, 33, 48, 49, 4097):
        for k in (0, 1, 15, 16, 17, 18, 40):
            if k > n - 8:
                continue
            t = gen.random_dna(n - k, 100 * n + k).copy()
            if n - k >= 40:
                mid = (n - k) // 2 - 10
                t[mid:mid + 20] = ord("A")
            out.append(t.tobytes() + b"A" * k)
    return out


def full_sub_bucket_text():
    """one sub-bucket (the suffixes that start with KMER) of 18 000 .. 18 432 pairs: below the capacity of a workgroup,
    above everything the other texts reach"""
    rng = np.random.default_rng(77)
    units = 18_200
    t = gen.ACGT[rng.integers(0, 4, size=(units, 12), dtype=np.uint8)]
    t[:, :8] = np.frombuffer(KMER, dtype=np.uint8)
    return t.reshape(-1).tobytes()


def count_8mers(t: bytes):
    """suffixes per sub-bucket: 8-mers of the text, zero-padded (A) behind its end"""
    code = np.zeros(256, dtype=np.int64)
    for k, c in enumerate(b"ACGT"):
        code[c] = k
    x = code[np.frombuffer(t + b"A" * 8, dtype=np.uint8)]
    v = np.zeros(len(t), dtype=np.int64)
    for j in range(8):
        v = v * 4 + x[j:j + len(t)]
    return np.bincount(v, minlength=65536)


def kmer_code(k: bytes) -> int:
    v = 0
    for c in k:
        v = v * 4 + b"ACGT".index(c)
    return v


def build_cases():
    """every text of the test, with the CPU-side proof that it holds what it is there for"""
    cases = []
    for n, seed in ((8192, 11), (150_000, 12)):
        t, plants = boundary_pairs_text(n, seed)
        seen = set()
        for p, q, length in plants:
            assert _lcp(t, p, q) == length, (p, q, length)
            # which bit of the base behind the block decides: the key's half base sees the high bit only
            hi = (b"ACGT".index(int(t[p + length])) ^ b"ACGT".index(int(t[q + length]))) >> 1
            seen.add((length, hi))
        assert seen == {(length, hi) for length in (15, 16, 17, 18, 19) for hi in (0, 1)}
        cases.append(t.tobytes())
    cases += end_of_text_cases()
    # sub-buckets beyond a workgroup's capacity (18 432 pairs): the list and the three segmented passes
    for t, kmer in ((b"A" * 30000 + gen.random_dna(20000, 4).tobytes(), b"AAAAAAAA"), (b"ACGT" * 25000 + b"T", b"ACGTACGT")):
        assert count_8mers(t)[kmer_code(kmer)] > 18_432
        cases.append(t)
    t = full_sub_bucket_text()
    c = count_8mers(t)
    assert 18_000 <= c[kmer_code(KMER)] <= 18_432 and c.max() == c[kmer_code(KMER)], c.max()
    cases.append(t)
    sizes = [63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097, 8191, 8192, 8193, 65535, 65536, 65537]
    cases += [gen.repeat_dna(m, 40 + m % 7, lo=8, hi=512).tobytes() for m in sizes]
    cases.append(gen.repeat_dna(300_000, 5, lo=16, hi=4096).tobytes())
    assert max(len(t) for t in cases) <= 300_000
    return cases


def test_cases_hold_what_they_are_there_for():
    """(no GPU) the planted LCPs, the sub-bucket counts and the sizes, checked in numpy"""
    cases = build_cases()
    assert all(len(t) >= MIN_KEY35 for t in cases)
    assert {32, 33, 48, 49, 4097} <= {len(t) for t in cases}


@pytest.fixture(scope="module")
def expected_file(tmp_path_factory):
    """the oracle's factors of every text, computed once for all the children"""
    import oracle_lib as oracle
    arrays = {}
    for i, t in enumerate(build_cases()):
        exp = oracle.factors_array(t)
        for k in ("start", "length", "ref"):
            arrays[f"{k}{i}"] = np.asarray(exp[k]).astype(np.uint64)
    path = tmp_path_factory.mktemp("key35") / "expected.npz"
    np.savez(path, **arrays)
    return str(path)


CHILD = r'''
import sys
sys.path.insert(0, "tests")
import numpy as np
import test_gpu_key35 as T
from nolzss_amd import _noLZSS as native
exp = np.load(sys.argv[1])
cases = T.build_cases()
for i, t in enumerate(cases):
    got = native.factorize_array(t)
    assert len(got) == len(exp[f"start{i}"]), (i, len(t), len(got))
    for k in ("start", "length", "ref"):
        assert np.array_equal(np.asarray(got[k]).astype(np.uint64), exp[f"{k}{i}"]), (i, len(t), k)
print("ok", len(cases))
'''


@pytest.mark.gpu
@pytest.mark.parametrize("extra_env,line", [
    ({}, "35-bit key sort"),
    ({"NOLZSS_TEST_LOCAL_ORDER_FAILS": "1"}, "35-bit key sort"),
    ({"NOLZSS_TEST_LOCAL_LOOKBACK_FAILS": "1"}, "35-bit key sort"),
    ({"NOLZSS_NO_LOCAL_REGROUP": "1"}, "35-bit key sort"),
    ({"NOLZSS_NO_KEY35": "1"}, "16-symbol key sort"),
], ids=["default", "sub-buckets-redone", "regroup-falls-back", "regroup-kernel", "knob-off"])
def test_key35_on_small_texts(expected_file, extra_env, line):
    """The default: local_sort_kernel<2, true, true> (two wide digits and the regroup of round 0), sub-buckets beyond a
    workgroup's capacity through three segmented passes.  NOLZSS_TEST_LOCAL_ORDER_FAILS: every sub-bucket redone by those
    passes, then regroup_kernel<true, 4>.  NOLZSS_TEST_LOCAL_LOOKBACK_FAILS: the text sorted again by the plain kernel.
    NOLZSS_NO_LOCAL_REGROUP: the plain kernel and the regroup kernel from the start.  NOLZSS_NO_KEY35: the 16-base key."""
    env = dict(os.environ, NOLZSS_DNA_FAST_MIN="1", NOLZSS_LOCAL_SORT_MIN="1", NOLZSS_LOCAL_REGROUP_MIN="1", NOLZSS_TRACE="1",
               **extra_env)
    r = subprocess.run([sys.executable, "-c", CHILD, expected_file], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
    took = {}
    for m in re.finditer(r"n=(\d+): \d+ suffixes tied after the (\d+-\w+) key sort", r.stderr):
        took.setdefault(int(m.group(1)), set()).add(m.group(2) + " key sort")
    for t in build_cases():
        assert took.get(len(t)) == {line}, (len(t), took.get(len(t)))
