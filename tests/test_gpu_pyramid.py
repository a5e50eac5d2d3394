"""The 16-ary pyramids (pyramid.hpp, pyramid.hip) and the searches built on them (nearest.hpp), run on the device by the
debug hooks and compared by integer equality with the numpy model (tests/pyramid_model.py): levels from the three ways a
pyramid is built, the pending flag, the three queries at every height of ascent and descent, and the searches, each
with the padding behind every array poisoned with 0x00 and with 0xFF.  tests/test_pyramid_model_host.py shows that
these inputs can see the mistakes they are there for."""
import numpy as np
import pytest

import pyramid_model as M

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def native():
    from nolzss_amd import _noLZSS
    assert _noLZSS.device_count() >= 1, "no MI355X visible"
    return _noLZSS


def same(got, exp, what):
    got, exp = np.asarray(got), np.asarray(exp)
    assert got.shape == exp.shape, what
    bad = np.flatnonzero((got != exp).reshape(len(got), -1).any(axis=1))
    assert not bad.size, (what, len(bad), "first at row", int(bad[0]), got[bad[0]].tolist(), exp[bad[0]].tolist())


@pytest.mark.parametrize("n", M.LENGTHS)
def test_levels_from_every_way_of_building(native, n):
    for is_max in (False, True):
        for arr in M.level_cases(n, is_max):
            exp = M.levels(arr, is_max)
            # mode 1: the caller's own level 1 in front of first_entry.  n >> 4 leaves the short last block to
            # fill_pyramid_tail (nothing where n is a multiple of 16); (n - 1) >> 4 leaves it the last block whatever its
            # size -- a full one at a multiple of 16, as the LCP pyramid of a text of 16k + 15 symbols has it
            builds = [(0, 0)] + ([(1, n >> 4), (1, (n - 1) >> 4)] if n >= 2 else [])
            for poison in M.POISONS:
                for mode, first_entry in builds:
                    got = native.debug_pyramid(arr, is_max, mode=mode, level1=exp[1][:first_entry] if mode else None,
                                               first_entry=first_entry, poison=poison)
                    what = (n, is_max, poison, mode, first_entry)
                    assert got["nlev"] == len(exp) and got["lens"] == M.level_lengths(n), what
                    for lev, (a, b) in enumerate(zip(got["levels"], exp)):
                        same(a, b, what + (f"level {lev}",))


@pytest.mark.parametrize("n", [n for n in M.LENGTHS if n >= 2])   # (the first level's kernel sets the flag: one entry has none)
def test_pending_flag(native, n):
    flag_min = 0xfffffff0     # (kLcpPendingMin is of this kind: a code above every length)
    rng = np.random.default_rng(n)
    clear = rng.integers(0, flag_min, size=n).astype(np.uint32)
    clear[rng.integers(0, n, size=3)] = flag_min - 1
    first, last = clear.copy(), clear.copy()
    first[0] = flag_min
    last[n - 1] = flag_min     # the last index: of a short last block where n is no multiple of 16
    for poison in M.POISONS:   # 0xFF: the padding itself reads as a pending code
        for arr, exp in ((clear, 0), (first, 1), (last, 1)):
            got = native.debug_pyramid(arr, False, flag_min=flag_min, poison=poison)
            assert got["flag"] == exp == M.flag_word(arr, flag_min), (n, poison, exp)
            same(got["levels"][-1], M.levels(arr, False)[-1], (n, poison, "top level"))


@pytest.mark.parametrize("is_max", [False, True])
@pytest.mark.parametrize("n", M.LENGTHS)
def test_queries(native, n, is_max):
    sent = 0
    for case in M.pyramid_cases(n, is_max):
        exp = M.answers_many(case.base, is_max, case.queries)
        for poison in M.POISONS:
            got = native.debug_pyramid(case.base, is_max, case.queries, poison=poison, want_levels=False)
            assert got["nlev"] == len(M.level_lengths(n))
            same(got["results"], exp, (case.name, "max" if is_max else "min", poison))
            sent += len(case.queries)
    print(f"pyramid queries n={n} {'max' if is_max else 'min'}: {sent}")


@pytest.mark.parametrize("n", M.NEAR_N)
def test_searches(native, n):
    sent = 0
    for case in M.near_cases(n):
        exp = M.near_answers(case.sa, case.lcp, case.queries)
        for poison in M.POISONS:
            same(native.debug_nearest(case.sa, case.lcp, case.queries, poison=poison), exp, (case.name, poison))
            sent += len(case.queries)
    print(f"search queries n={n}: {sent}")


@pytest.fixture(scope="module")
def lpnf_texts():
    return M.lpnf_texts()


@pytest.mark.parametrize("name", ["run", "period2", "fibonacci", "repeat_dna"])
def test_lpnf_search(native, lpnf_texts, name):
    import oracle_lib as oracle
    text = lpnf_texts[name]
    memo = {}
    case, longest = M.lpnf_case(name, text, memo)
    ln = oracle.lpnf_all(text)[0]
    assert all(int(ln[i]) == max(L, 1) for i, L in longest.items())   # (the oracle counts a literal as length 1)
    exp = M.near_answers(case.sa, case.lcp, case.queries, memo=memo)
    for poison in M.POISONS:
        same(native.debug_nearest(case.sa, case.lcp, case.queries, poison=poison), exp, (name, poison))
    print(f"lpnf_search queries {name}: {2 * len(case.queries)}")


def test_refusals_come_back_as_errors(native):
    base = np.arange(100, dtype=np.uint32)
    for rows in ([(M.OP_LEFT, 100, 5)], [(M.OP_RANGE, 7, 6)], [(M.OP_RANGE, 0, 100)], [(9, 0, 0)]):
        with pytest.raises(ValueError):
            native.debug_pyramid(base, False, rows)
    with pytest.raises(ValueError):
        native.debug_pyramid(np.zeros(0, dtype=np.uint32), False)
    with pytest.raises(ValueError, match="lcp"):
        native.debug_nearest(base, np.ones(101, dtype=np.uint32), [(M.UP_LESS, 3, 5, 0, 0)])
    # nearest_right from r >= len is legal and answers len
    got = native.debug_pyramid(base, False, [(M.OP_RIGHT, 100, 50), (M.OP_RIGHT, 0xffffffff, 50), (M.OP_RIGHT, 99, 100)])
    assert got["results"].tolist() == [100, 100, 99]
