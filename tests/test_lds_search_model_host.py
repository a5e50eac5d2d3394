"""The model of the LDS tile searches (tests/lds_search_model.py) without a GPU: the brute force against a pure-Python
walk, the lane-group restatement of rounds B + C against the brute force, the inputs of tests/test_gpu_lds_search.py
against the mistakes they are there to see, and the refusals of the debug hook that need no device."""
import random

import numpy as np
import pytest

import lds_search_model as M
from nolzss_amd import _lib


def python_walk(sa, lcp, r, k, strand):
    """search k of rank r on a single tile (n <= 768: the whole array is in sight), step by step"""
    greater, up = M.kind(k)
    n = len(sa)
    x = 2 * strand - sa[r] if greater else sa[r]
    m, q = 0xffffffff, r
    for d in range(1, 257):
        q = r - d if up else r + d
        inside = 0 <= q < n
        edge = q + 1 if up else q
        m = min(m, lcp[edge] if 0 <= edge <= n else 0)
        v = sa[q] if inside else 0
        if (v > x) if greater else (v < x):
            return (m, sa[q]) if m else (0, M.NONE)
        if d in (4, 16) and m == 0:
            return 0, M.NONE
    return M.FAR | m, M.NONE


def test_the_brute_force_matches_a_python_walk():
    rng = random.Random(20261022)
    matches = 0
    for n_case in range(60):
        n = rng.choice([1, 2, 5, 17, 40, 200, 255])
        sa = rng.sample(range(0, 4 * n + 4), n)
        lcp = [0] + [rng.choice([0, 1, 2, 3, 3, 7]) if n_case % 2 else rng.randint(1, 9) for _ in range(n - 1)] + [0]
        strand = 2 * n + 2
        for form in (M.PLAIN, M.RC):
            length, pos = M.answers(sa, lcp, form, strand)
            for r in range(n):
                for k in range(M.searches(form)):
                    exp = python_walk(sa, lcp, r, k, strand) if form == M.PLAIN or sa[r] < strand else (0, M.NONE)
                    got = (int(length[k, r]), int(pos[k, r]) if k < 2 else exp[1])
                    assert got == exp, (n, form, r, k)
                    matches += exp[1] != M.NONE
    assert matches >= 2000


def test_reach_by_alignment():
    up, down = M.reach_of(2048, True), M.reach_of(2048, False)
    assert up[0] == 256 and down[1023] == 256                 # the ends of the tile: one block lies outside the span
    assert set(up.tolist()) == set(range(256, 273)) and set(down.tolist()) == set(range(256, 273))
    assert up[1024 + 16] == 272 and down[1007] == 272 and np.array_equal(up[:1024], up[1024:])


@pytest.fixture(scope="module")
def cases():
    return {n: M.case(n) for n in M.SIZES}


@pytest.mark.parametrize("form", [M.PLAIN, M.RC], ids=["plain", "rc"])
@pytest.mark.parametrize("n", M.SIZES)
def test_the_cases_hold_what_they_list(cases, n, form):
    c = cases[n]
    assert c.lcp[0] == 0 and c.lcp[n] == 0 and len(np.unique(c.sa)) == n
    M.check_features(c, form)


# which sizes must see which mistake (form: plain): a group of lanes needs searches that go beyond 16 steps; a partial
# minimum that takes in the stopping block shows where the target lies in the middle of its block, from 1024 ranks on
SEEN_FROM = {"later_stop": 255, "carry_dropped": 255, "wrong_lane": 255, "partial_with_stop": 1024}


@pytest.mark.parametrize("lanes", [2, 4])
@pytest.mark.parametrize("n", M.SIZES)
def test_the_cases_see_the_mistakes_of_a_lane_group(cases, n, lanes):
    c = cases[n]
    for form in (M.PLAIN, M.RC):
        walks = M.case_walks(c, form)
        exp = M.answers(c.sa, c.lcp, form, M.STRAND)
        got = M.grouped(c.sa, c.lcp, form, M.STRAND, lanes, walks=walks)
        assert np.array_equal(got[0], exp[0]) and np.array_equal(got[1], exp[1]), (n, form)   # the restatement is right
        for rule in M.WRONG_RULES:
            wrong = M.grouped(c.sa, c.lcp, form, M.STRAND, lanes, rule, walks=walks)
            seen = not (np.array_equal(wrong[0], exp[0]) and np.array_equal(wrong[1], exp[1]))
            assert seen == (n >= SEEN_FROM[rule]), (n, form, lanes, rule)


# ---- what needs no device --------------------------------------------------------------------------------------------
def test_symbol_is_exported():
    assert "nolzss_debug_lds_search" in _lib.EXPORTED_SYMBOLS and hasattr(_lib.lib, "nolzss_debug_lds_search")


def test_the_hook_refuses_bad_arguments_before_any_device_work():
    lib, bad = _lib.lib, _lib.ERR_INVALID_ARGUMENT
    sa = np.arange(10, dtype=np.uint32)
    lcp = np.array([0] + [2] * 9 + [0], dtype=np.uint32)
    length, pos = np.zeros((4, 10), dtype=np.uint32), np.zeros((2, 10), dtype=np.uint32)

    def call(sa_=sa, lcp_=lcp, n=10, form=0, poison=0, out_len=length, out_pos=pos):
        return lib.nolzss_debug_lds_search(sa_.ctypes.data if sa_ is not None else None,
                                           lcp_.ctypes.data if lcp_ is not None else None, n, form, 5, poison, 0,
                                           out_len.ctypes.data if out_len is not None else None,
                                           out_pos.ctypes.data if out_pos is not None else None)

    assert call(sa_=None) == bad and b"null" in lib.nolzss_last_error()
    assert call(lcp_=None) == bad and call(out_len=None) == bad and call(out_pos=None) == bad
    assert call(n=0) == bad and b"empty" in lib.nolzss_last_error()
    assert call(n=(1 << 31) - 2047) == bad
    assert call(form=2) == bad and call(form=-1) == bad and call(poison=1) == bad
    for broken in (np.array([1] + [2] * 9 + [0], dtype=np.uint32), np.array([0] + [2] * 9 + [3], dtype=np.uint32)):
        assert call(lcp_=broken) == bad and b"lcp[0] and lcp[n]" in lib.nolzss_last_error()
