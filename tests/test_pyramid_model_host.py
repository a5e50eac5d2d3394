"""The pyramid and nearest-suffix model (tests/pyramid_model.py) without a GPU: the model against a pure-Python brute
force, the inputs of tests/test_gpu_pyramid.py against the mistakes they are there to see, and the refusals of the two
debug hooks that need no device."""
import ctypes as C
import random

import numpy as np
import pytest

import pyramid_model as M
from nolzss_amd import _lib


# ---- the model against a brute force -------------------------------------------------------------------------------
def brute_levels(base, is_max):
    out = [list(base)]
    while len(out[-1]) > 1:
        cur = out[-1]
        out.append([(max if is_max else min)(cur[k:k + 16]) for k in range(0, len(cur), 16)])
    return out


def brute_hit(v, x, is_max):
    return v > x if is_max else v < x


def brute_left(base, r, x, is_max):
    for q in range(r, -1, -1):
        if brute_hit(base[q], x, is_max):
            return q
    return M.NONE


def brute_right(base, r, x, is_max):
    for q in range(r, len(base)):
        if brute_hit(base[q], x, is_max):
            return q
    return len(base)


def brute_search(sa, lcp, r, x, floor, up, greater, start):
    q, m = (r - start, None) if up else (r + start, None)
    while 0 <= q < len(sa) and not brute_hit(sa[q], x, greater):
        q += -1 if up else 1
    if not 0 <= q < len(sa):
        return 0, M.NONE
    m = min(lcp[q + 1:r + 1]) if up else min(lcp[r + 1:q + 1])
    return (0, M.NONE) if m == 0 or m < floor else (m, sa[q])


def test_queries_match_the_brute_force():
    rng = random.Random(20261019)
    arrays = left_none = right_none = 0
    for n_case in range(400):
        n = rng.choice([1, 2, 15, 16, 17, 31, 32, 33, 47, 48, 49]) if n_case % 2 else rng.randint(1, 600)
        is_max = bool(n_case & 1) ^ bool(n_case & 2)
        top = rng.choice([3, 3, 50, 0xffffffff])
        base = [rng.randint(0, top) for _ in range(n)]
        arr = np.array(base, dtype=np.uint32)
        lv = M.levels(arr, is_max)
        assert [len(a) for a in lv] == M.level_lengths(n) and [a.tolist() for a in lv] == brute_levels(base, is_max)
        rows, exp = [], []
        for _ in range(30):
            r, x = rng.randrange(n), rng.choice([rng.randint(0, top), 0, top, base[rng.randrange(n)]])
            a = rng.randrange(n)
            b = rng.randint(a, n - 1)
            rows += [(M.OP_LEFT, r, x), (M.OP_RIGHT, r, x), (M.OP_RANGE, a, b)]
            exp += [brute_left(base, r, x, is_max), brute_right(base, r, x, is_max),
                    (max if is_max else min)(base[a:b + 1])]
        rows.append((M.OP_RIGHT, n + rng.randrange(3), 0))
        exp.append(n)
        got = M.answers(arr, is_max, rows)
        assert got.tolist() == exp, (n, is_max)
        assert np.array_equal(M.answers_many(arr, is_max, rows), got), (n, is_max)
        arrays += 1
        left_none += exp[0::3].count(M.NONE)
        right_none += exp[1::3].count(n)
    assert arrays == 400 and left_none >= 400 and right_none >= 400   # the inputs reach both ends


def test_searches_match_the_brute_force():
    rng = random.Random(20261020)
    found = 0
    for n_case in range(300):
        n = rng.choice([1, 4, 5, 6, 40, 252, 253, 254, 300, 600])
        sa = [rng.randint(0, 4) for _ in range(n)]
        lcp = [0] + [rng.choice([1, 2, 3, 3, 3, 0]) for _ in range(n - 1)] + [0]
        if n_case % 3 == 0:     # a plateau, so that the far searches find something
            sa = [2] * n
            sa[rng.randrange(n)] = rng.choice([1, 3])
            lcp = [0] + [rng.choice([3, 4]) for _ in range(n - 1)] + [0]
        a_sa, a_lcp = np.array(sa, dtype=np.uint32), np.array(lcp, dtype=np.uint32)
        rows, exp = [], []
        for _ in range(12):
            r, x, floor = rng.randrange(n), rng.randint(0, 4), rng.randint(0, 4)
            for op in range(M.UP_LESS, M.FAR_DOWN_GREATER + 1):
                up, start = op in (0, 1, 4, 5), 253 if op >= 4 else 1
                rows.append((op, r, x, floor, 0))
                exp.append(brute_search(sa, lcp, r, x, floor, up, bool(op & 1), start))
            d = rng.randint(1, 5)
            lo = max(q for q in range(r + 1) if lcp[q] < d)
            hi = min(q for q in range(r + 1, n + 1) if lcp[q] < d) - 1
            rows += [(M.LCP_INTERVAL, r, d, 0, 0), (M.LPNF_LEFTMOST, r, d, 0, 0)]
            exp += [(lo, hi), (min(sa[lo:hi + 1]), 0)]
        got = M.near_answers(a_sa, a_lcp, rows)
        assert got.tolist() == [list(e) for e in exp], n
        found += sum(1 for e in exp if e[1] != M.NONE and e[0] != 0)
    assert found >= 3000


def test_lpnf_search_matches_the_definition():
    """on true SA / LCP the model's search is the longest previous non-overlapping factor: the longest d for which
    text[i : i + d] occurs at some j with j + d <= i"""
    import oracle_lib as oracle
    rng = random.Random(20261021)
    for n_case in range(40):
        n = rng.randint(2, 90)
        text = bytes(rng.choice(b"AC" if n_case % 2 else b"ACGT") for _ in range(n))
        if n_case % 5 == 0:
            text = (text[:rng.randint(1, 4)] * n)[:n]
        sa, isa, lcp = M.text_arrays(text)
        ln = oracle.lpnf_all(text)[0]
        for i in range(n):
            best = 0
            for d in range(1, n - i + 1):
                if any(text[j:j + d] == text[i:i + d] for j in range(0, i - d + 1)):
                    best = d
            assert M.lpnf_search(sa, lcp, int(isa[i]), i, 0, n - i) == best, (text, i)
            assert int(ln[i]) == max(best, 1), (text, i)     # (the oracle counts a literal as length 1)
            if best >= 2:
                assert M.lpnf_search(sa, lcp, int(isa[i]), i, best - 1, best + 1) == best
                assert M.lpnf_search(sa, lcp, int(isa[i]), i, 1, best - 1) == best - 1
            assert M.lpnf_search(sa, lcp, int(isa[i]), i, best, best) == best


# ---- the inputs hold what they are there for -------------------------------------------------------------------------
def rule_kwargs(name, is_max):
    kw = dict(M.WRONG_RULES[name])
    if kw.get("pad"):
        kw["pad"] = 0xffffffff if is_max else 0    # the poison that beats every entry (the GPU test runs both)
    return kw


def seen(case, name):
    """some query of the case is answered differently under the wrong rule (one query at a time: the first one ends it)"""
    kw = rule_kwargs(name, case.is_max)
    for row in np.asarray(case.queries).tolist():
        if M.answers(case.base, case.is_max, [row], **kw)[0] != M.answers(case.base, case.is_max, [row])[0]:
            return True
    return False


def unmasked_can_show(n):
    """A right walk without a hit meets an unhidden padding entry that changes its answer iff some level l >= 1 of two
    entries or more has a short last block and the base index under its first padding entry, len[l] * 16^l, is not len
    (pyramid_model.nearest_right)."""
    return any(ln >= 2 and ln % 16 and ln << (4 * l) != n for l, ln in enumerate(M.level_lengths(n)) if l >= 1)


FAMILIES = {
    # family -> (builder, {wrong rule: the lengths at which it must be seen})
    "one_hit": (M.one_hit_cases, {"nonstrict": lambda n: n >= 2}),     # (n = 1: the only entry is the hit itself)
    "no_hit": (M.no_hit_cases, {"nonstrict": lambda n: True, "unmasked": unmasked_can_show}),
    "identity": (M.identity_cases, {"nonstrict": lambda n: True}),
    "random": (M.random_cases, {"nonstrict": lambda n: True}),
    "range": (M.range_cases, {"range_a-1": lambda n: n >= 2, "range_b+1": lambda n: n >= 2,
                              "range_excl_b": lambda n: True, "unmasked_range": lambda n: True}),
}


@pytest.mark.parametrize("family", sorted(FAMILIES))
@pytest.mark.parametrize("is_max", [False, True])
def test_pyramid_inputs_see_the_wrong_rules(family, is_max):
    builder, expect = FAMILIES[family]
    for n in M.LENGTHS:
        cases = builder(n, is_max)
        assert cases and all(len(c.queries) for c in cases)
        names = {name for c in cases for name in c.applies}
        assert names == set(expect), (family, n, names)
        for name, must in expect.items():
            caught = any(seen(c, name) for c in cases if name in c.applies)
            assert caught == bool(must(n)), (family, n, name)


def test_level_inputs_see_a_missing_mask():
    for is_max in (False, True):
        pad = 0xffffffff if is_max else 0
        for n in M.LENGTHS:
            arr = M.level_cases(n, is_max)[0]
            right, wrong = M.levels(arr, is_max), M.levels(arr, is_max, pad=pad)
            differs = any(not np.array_equal(a, b) for a, b in zip(right, wrong))
            assert differs == any(ln % 16 for ln in M.level_lengths(n)[:-1]), n   # some group is short


def test_the_lengths_reach_every_level_count():
    assert [len(M.level_lengths(n)) for n in M.LENGTHS] == [1, 2, 2, 2, 3, 3, 3, 3, 3, 3, 4, 4, 4, 4, 4, 4, 5, 5, 5,
                                                            6, 6, 6, 7, 7]
    assert M.level_lengths(16 ** 5 + 1) == [16 ** 5 + 1, 16 ** 4 + 1, 16 ** 3 + 1, 257, 17, 2, 1]


def near_seen(case, name, memo=None):
    kw = rule_kwargs(name, False)
    for row in np.asarray(case.queries).tolist():
        if not np.array_equal(M.near_answers(case.sa, case.lcp, [row], memo=memo, **kw),
                              M.near_answers(case.sa, case.lcp, [row], memo=memo)):
            return True
    return False


@pytest.mark.parametrize("n", M.NEAR_N)
def test_search_inputs_see_the_wrong_rules(n):
    cases = M.near_cases(n)
    plateau = [c for c in cases if c.name.startswith("plateau")]
    assert bool(plateau) == (n >= 4) and len(cases) == len(plateau) + 1
    for name in ("nonstrict", "near", "far"):
        assert any(near_seen(c, name) for c in plateau) == (n >= 4), (n, name)
    if n >= 4:
        assert near_seen(cases[-1], "nonstrict"), n
    # the qualifying rank lies at every distance that fits, each way, and the dip is crossed
    dists = {d for d in M.NEAR_DIST if d < n}
    assert {int(c.name.split("dist=")[1].split(",")[0]) for c in plateau} == dists
    if n >= 257:
        assert any((c.lcp == M.DIP).any() for c in plateau)


def test_lpnf_search_inputs_see_a_wrong_predicate():
    import oracle_lib as oracle
    texts = M.lpnf_texts()
    assert [len(t) for t in texts.values()] == [5000, 6001, 10_000, 20_000]
    caught = {}
    for name, text in texts.items():
        memo = {}
        case, longest = M.lpnf_case(name, text, memo)
        ln = oracle.lpnf_all(text)[0]
        assert all(int(ln[i]) == max(L, 1) for i, L in longest.items()), name     # L is the oracle's (a literal: 1)
        assert len(case.queries) >= 50 and max(longest.values()) >= 16
        caught[name] = near_seen(case, "nonstrict", memo)
    # the periodic texts hold positions whose best match ends exactly where they start
    assert caught["run"] and caught["period2"] and caught["fibonacci"], caught


# ---- what needs no device --------------------------------------------------------------------------------------------
def test_symbols_are_exported():
    for name in ("nolzss_debug_pyramid", "nolzss_debug_nearest"):
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(_lib.lib, name)


def call_pyramid(base, n, queries=(), is_max=0, mode=0, level1=None, first_entry=0, flag_min=0, poison=0, nlev=True,
                 lens=True, flag=True):
    q = np.array(queries, dtype=np.uint32).reshape(-1, 3)
    res = np.zeros(max(len(q), 1), dtype=np.uint32)
    out_nlev, out_flag, out_lens = C.c_int(), C.c_uint32(), np.zeros(9, dtype=np.uint32)
    return _lib.lib.nolzss_debug_pyramid(
        base.ctypes.data if base is not None else None, n, is_max, mode,
        level1.ctypes.data if level1 is not None else None, first_entry, flag_min, poison,
        q.ctypes.data if len(q) else None, len(q), 0, C.byref(out_nlev) if nlev else None,
        out_lens.ctypes.data if lens else None, None, 0, C.byref(out_flag) if flag else None, res.ctypes.data)


def test_the_pyramid_hook_refuses_bad_arguments_before_any_device_work():
    bad = _lib.ERR_INVALID_ARGUMENT
    base = np.arange(40, dtype=np.uint32)
    assert call_pyramid(None, 40) == bad and b"null" in _lib.lib.nolzss_last_error()
    assert call_pyramid(base, 40, nlev=False) == bad and call_pyramid(base, 40, lens=False) == bad
    assert call_pyramid(base, 0) == bad and b"empty" in _lib.lib.nolzss_last_error()
    assert call_pyramid(base, 1 << 32) == bad and call_pyramid(base, (1 << 32) + 5) == bad
    assert call_pyramid(base, 40, mode=2) == bad and call_pyramid(base, 40, poison=0x55) == bad
    assert call_pyramid(base, 40, queries=[(M.OP_LEFT, 40, 1)]) == bad          # r >= len for left
    assert call_pyramid(base, 40, queries=[(M.OP_RANGE, 5, 4)]) == bad          # a > b
    assert call_pyramid(base, 40, queries=[(M.OP_RANGE, 5, 40)]) == bad         # b >= len
    assert call_pyramid(base, 40, queries=[(3, 0, 0)]) == bad                   # unknown op
    assert call_pyramid(base, 40, queries=[(M.OP_RIGHT, 0, 1), (M.OP_RANGE, 0, 40)]) == bad   # any row
    assert call_pyramid(base, 1, mode=1) == bad                                 # no level 1 to write
    assert call_pyramid(base, 40, mode=1, first_entry=4) == bad                 # level 1 has 3 entries
    assert call_pyramid(base, 40, mode=1, first_entry=2) == bad                 # level-1 entries wanted, none given
    assert call_pyramid(base, 40, is_max=1, flag_min=7) == bad                  # the flag belongs to a min pyramid
    assert call_pyramid(base, 40, flag_min=7, flag=False) == bad and call_pyramid(base, 1, flag_min=7) == bad
    lib = _lib.lib   # a null result array with queries present
    q = np.array([[M.OP_RIGHT, 0, 1]], dtype=np.uint32)
    n_out, lens = C.c_int(), np.zeros(9, dtype=np.uint32)
    assert lib.nolzss_debug_pyramid(base.ctypes.data, 40, 0, 0, None, 0, 0, 0, q.ctypes.data, 1, 0, C.byref(n_out),
                                    lens.ctypes.data, None, 0, None, None) == bad


def test_the_nearest_hook_refuses_bad_arguments_before_any_device_work():
    lib, bad = _lib.lib, _lib.ERR_INVALID_ARGUMENT
    sa = np.arange(10, dtype=np.uint32)
    lcp = np.array([0] + [2] * 9 + [0], dtype=np.uint32)
    res = np.zeros((4, 2), dtype=np.uint32)

    def call(sa_, lcp_, n, rows, poison=0, out=res):
        q = np.array(rows, dtype=np.uint32).reshape(-1, 5)
        return lib.nolzss_debug_nearest(sa_.ctypes.data if sa_ is not None else None,
                                        lcp_.ctypes.data if lcp_ is not None else None, n, poison,
                                        q.ctypes.data if len(q) else None, len(q), 0,
                                        out.ctypes.data if out is not None else None)

    ok_row = (M.UP_LESS, 3, 5, 0, 0)
    assert call(None, lcp, 10, [ok_row]) == bad and call(sa, None, 10, [ok_row]) == bad
    assert call(sa, lcp, 0, [ok_row]) == bad and b"empty" in lib.nolzss_last_error()
    assert call(sa, lcp, (1 << 32) - 1, [ok_row]) == bad
    assert call(sa, lcp, 10, [ok_row], out=None) == bad and call(sa, lcp, 10, [ok_row], poison=1) == bad
    for broken in (np.array([1] + [2] * 9 + [0], dtype=np.uint32), np.array([0] + [2] * 9 + [3], dtype=np.uint32)):
        assert call(sa, broken, 10, [ok_row]) == bad and b"lcp[0] and lcp[n]" in lib.nolzss_last_error()
    assert call(sa, lcp, 10, [(M.UP_LESS, 10, 5, 0, 0)]) == bad                 # r >= n
    assert call(sa, lcp, 10, [(11, 3, 5, 0, 0)]) == bad                         # unknown op
    assert call(sa, lcp, 10, [(M.LCP_INTERVAL, 3, 0, 0, 0)]) == bad             # d == 0
    assert call(sa, lcp, 10, [(M.LPNF_LEFTMOST, 3, 0, 0, 0)]) == bad
    assert call(sa, lcp, 10, [(M.LPNF_SEARCH, 3, 10, 0, 4)]) == bad             # i >= n
    assert call(sa, lcp, 10, [ok_row, (M.DOWN_LESS, 12, 5, 0, 0)]) == bad       # any row
