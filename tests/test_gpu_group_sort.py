"""The group-sort rounds of the suffix-array construction (group_sort.hpp: group_dir_kernel and group_sort_kernel in its
tiled, 128-, 256- and 1024-member forms, as window rounds and as pivot rounds, at 2, 4 and 8 bits per symbol) on caller
groups, through nolzss_debug_group_sort -- the launch function of the construction itself, with no regroup behind it --
against the round-level model of tests/group_sort_model.py by integer equality: sa, out_lo, lcp_list and min_depth.
tests/test_group_sort_model_host.py proves without a GPU that the model agrees with the definition of the suffix order
and what every input is there for.

The inputs (group_sort_model.CASES), at most 72 000 symbols and 69 000 list entries per call:
  size_*, sizes_*, big_*   groups of 2, 3, 63 .. 65, 127 .. 129, 255 .. 257, 1023 .. 1025 members, alone and in one list with gaps
  deep_*                   first differences at every depth from h0 to a pivot round and two symbols, every residue, both
                           halves, highest and lowest code bit; caps on, around and below h0; budgets of one and two rounds
  verydeep_*               ties that outlast 24 window rounds, in a pair and inside a triple
  tiles                    groups that start at places 0, 1, 62, 63 of a tile and cross it; a small group behind a large one
  queues, small_only       68 850 entries in groups of 65 .. 70 (shards shared by workgroups, more items than gridDim.y); no queue entry
  equalise*                lcp_mark on every other group, reduced budgets
  terms_*                  terminator tables of 2 .. 4 (kernel arguments), 5, 33 and 251 entries; every length inside the window
  mutated_*, hotspots_*    5 .. 1024 mutated copies; equal l with different symbols
  periodic, capedge        exact copies tied at the cap and out of rounds; a class that ends exactly at the cap
"""
import numpy as np
import pytest

import group_sort_model as M

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def native():
    from nolzss_amd import _noLZSS as native
    assert native.device_count() >= 1, "no MI355X visible"
    return native


def run_one(native, name, order, pivot, max_rounds, depth_cap, marked):
    """one call of the hook, everything it returns against the model; -> the model's account of what ran"""
    case = M.CASES[name]
    text, lst = M.text_of(case.text), M.listed(name, order)
    exp = M.expected(name, order, pivot, max_rounds, depth_cap, marked)
    got = native.debug_group_sort(text.data, lst.sa, lst.slot, lst.grp, case.h0, pivot, max_rounds, depth_cap,
                                  M.mark_for(name, order) if marked else None)
    where = (name, order, "pivot" if pivot else "window", max_rounds, depth_cap, marked)
    assert (got["bits"], got["terms"], got["segmented"]) == (text.bits, text.terms.size, text.segmented), where
    outside = np.ones(text.n, dtype=bool)
    outside[lst.slot] = False
    assert np.array_equal(got["sa"][outside], lst.sa[outside]), where
    for k in ("sa", "out_lo", "lcp_list"):
        bad = np.nonzero(got[k] != exp[k])[0]
        assert bad.size == 0, (where, k, bad[:8].tolist(), got[k][bad[:8]].tolist(), exp[k][bad[:8]].tolist())
    assert got["min_depth"] == exp["min_depth"], where
    return exp


@pytest.mark.parametrize("name", list(M.CASES))
def test_rounds_match_the_model(native, name):
    forms, tied, runs = {}, 0, 0
    for run in M.runs_of(name):
        exp = run_one(native, name, *run)
        for form, count in exp["forms"].items():
            key = f"{form}/{'pivot' if run[1] else 'window'}"
            forms[key] = forms.get(key, 0) + count
        tied += exp["tied"]
        runs += 1
    text = M.text_of(M.CASES[name].text)
    print(f"{name}: {runs} runs at {text.bits} bits, {text.terms.size} terminator entries; groups by form {forms}; members left tied {tied}")


def test_a_call_leaves_no_state_behind(native):
    """one case as window rounds, then as pivot rounds, then as window rounds again"""
    for name in ("sizes_w2", "terms_33"):
        for pivot in (False, True, False):
            run_one(native, name, "shuffle" if name == "sizes_w2" else "text", pivot, M.ROUNDS, M.NONE, False)


def test_bad_arguments_are_refused(native):
    text = b"ACGTACGTACGTACGTAACC"
    sa = np.arange(20, dtype=np.uint32)
    ok = dict(text=text, sa=sa, slot=[3, 4, 7, 8, 9], grp=[3, 3, 7, 7, 7], h0=0)
    got = native.debug_group_sort(**ok)
    assert sorted(got["sa"][3:5]) == [3, 4] and sorted(got["sa"][7:10]) == [7, 8, 9] and got["lcp_list"][0] == 0
    bad_sa = sa.copy()
    bad_sa[8] = 20
    bad = [
        dict(ok, text=b"", sa=sa[:0], slot=[], grp=[]),               # no text
        dict(ok, slot=list(range(21)), grp=[0] * 21),                   # more list entries than suffixes
        dict(ok, sa=bad_sa),                                            # a listed slot that holds no suffix
        dict(ok, slot=[3, 4, 7, 8, 9], grp=[3, 3, 8, 8, 8]),            # grp > slot
        dict(ok, slot=[3, 4, 18, 19, 20], grp=[3, 3, 18, 18, 18]),      # slot >= n
        dict(ok, slot=[7, 8, 9, 3, 4], grp=[7, 7, 7, 3, 3]),            # not in ascending slot order
        dict(ok, slot=[3, 4, 4, 8, 9], grp=[3, 3, 3, 8, 8]),            # a slot twice
        dict(ok, slot=[3, 5, 7, 8, 9], grp=[3, 3, 7, 7, 7]),            # a group with a hole in its slots
        dict(ok, slot=[4, 5, 7, 8, 9], grp=[3, 3, 7, 7, 7]),            # a group that does not start at its head slot
        dict(ok, slot=[3, 4, 7, 8, 9], grp=[3, 3, 7, 8, 8]),            # a listed group of one member
        dict(ok, slot=[3, 4, 7, 8, 12], grp=[3, 3, 7, 7, 12]),          # ... at the end of the list
        dict(ok, max_rounds=M.ROUNDS + 1),                              # more rounds than kGroupSortRounds
        dict(ok, sa=sa[:19]), dict(ok, grp=[3, 3, 7, 7]), dict(ok, lcp_mark=sa[:19]),   # lengths that do not fit
    ]
    for kw in bad:
        with pytest.raises(ValueError):
            native.debug_group_sort(**kw)
    from nolzss_amd._lib import lib
    t = np.frombuffer(text, dtype=np.uint8)
    slot, grp = np.array(ok["slot"], dtype=np.uint32), np.array(ok["grp"], dtype=np.uint32)
    lo, lcp, depth = np.zeros(5, dtype=np.uint32), np.zeros(5, dtype=np.uint32), np.zeros(1, dtype=np.uint32)
    work = sa.copy()
    args = [t.ctypes.data, 20, work.ctypes.data, slot.ctypes.data, grp.ctypes.data, 5, 0, 0, M.ROUNDS, M.NONE, None, 0,
            lo.ctypes.data, lcp.ctypes.data, depth.ctypes.data, None]
    assert lib.nolzss_debug_group_sort(*args) == 0
    for null_at in (0, 2, 3, 4, 12, 13, 14):
        a = list(args)
        a[null_at] = None
        assert lib.nolzss_debug_group_sort(*a) != 0, null_at
    a = list(args)
    a[1] = 0  # (refused before anything is read)
    assert lib.nolzss_debug_group_sort(*a) != 0
