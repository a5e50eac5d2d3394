"""The window rounds of group_sort.hpp in their one-trip form -- a scanning member asks for the words of its scan, of its
segment's first member and of its window at once and cuts the window out of registers; the queue kernels count places with one
position per thread; queue items are taken from a counter of the shard -- through nolzss_debug_group_sort against
tests/group_sort_model.py (unchanged) by integer equality of sa, out_lo, lcp_list and min_depth.  The inputs are built in
tests/group_sort_trips_cases.py; tests/test_group_sort_trips_host.py shows on the CPU which mistake they tell from the model.

The hook packs the text itself (the caller hands over bytes), so a test cannot own the packed buffer and cannot fill the
words behind the text with 0x00 in one run and 0xFF in the next; the suffix whose scan runs past the end of the text
(ends_case) is checked against the model with the padding pack_text writes.
"""
import numpy as np
import pytest

import group_sort_model as M
import group_sort_trips_cases as C

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def native():
    from nolzss_amd import _noLZSS as native
    assert native.device_count() >= 1, "no MI355X visible"
    return native


def check(native, built, pivot=False, max_rounds=M.ROUNDS, depth_cap=M.NONE, mark=None, where=()):
    text, lst = built.text, built.listed
    exp = M.model(text, lst, C.H0, pivot, max_rounds, depth_cap, mark)
    got = native.debug_group_sort(text.data, lst.sa, lst.slot, lst.grp, C.H0, pivot, max_rounds, depth_cap, mark)
    assert (got["bits"], got["terms"], got["segmented"]) == (text.bits, text.terms.size, text.segmented), where
    for k in ("sa", "out_lo", "lcp_list"):
        bad = np.nonzero(got[k] != exp[k])[0]
        assert bad.size == 0, (where, k, bad[:8].tolist(), got[k][bad[:8]].tolist(), exp[k][bad[:8]].tolist())
    assert got["min_depth"] == exp["min_depth"], where
    return exp, got


@pytest.mark.parametrize("size", C.SIZES)
def test_group_sizes_alone_and_next_to_small_groups(native, size):
    for with_small in (False, True):
        exp, _ = check(native, C.sizes_case(size, with_small), where=(size, with_small))
        assert exp["forms"][M.form_of(size)] == 1 and exp["tied"] == 0  # (they split into singletons, most in the first round)


@pytest.mark.parametrize("first", list(C.FIRST))
@pytest.mark.parametrize("k", (3, 66))
def test_first_difference_in_the_scan_and_the_next_in_the_window(native, first, k):
    for second in C.SECOND:
        for max_rounds in (2, 3, M.ROUNDS):
            check(native, C.diff_case(first, second, k), max_rounds=max_rounds, where=(first, second, k, max_rounds))


def test_first_difference_256_threads(native):
    for first, second in (("word8_stop", 64), ("word7_last_bit", 63)):
        for max_rounds in (2, M.ROUNDS):
            check(native, C.diff_case(first, second, 130), max_rounds=max_rounds, where=(first, second, max_rounds))


@pytest.mark.parametrize("k", (8, 70, 140))
def test_ends_inside_the_scan_the_window_and_past_the_text(native, k):
    built = C.ends_case(k)
    for max_rounds in (2, 3, M.ROUNDS):
        exp, _ = check(native, built, max_rounds=max_rounds, where=(k, max_rounds))
    assert exp["tied"] == 0


@pytest.mark.parametrize("k", (70, 130))
def test_equal_members_give_up(native, k):
    for max_rounds in (1, 2, M.ROUNDS):
        exp, _ = check(native, C.equal_case(k), max_rounds=max_rounds, where=(k, max_rounds))
        assert exp["tied"] > 0 and exp["min_depth"] != M.NONE


def test_more_items_in_a_shard_than_workgroups_twice(native):
    built = C.many_items_case()
    exp, a = check(native, built)
    assert exp["forms"]["m128"] >= 300
    _, b = check(native, built)
    for k in ("sa", "out_lo", "lcp_list"):
        assert np.array_equal(a[k], b[k]), k
    assert a["min_depth"] == b["min_depth"]


def test_the_ladder_in_pivot_rounds_and_in_the_equalising_round(native):
    built = C.ladder_case()
    check(native, built, pivot=True, where="pivot")
    exp, _ = check(native, built, mark=C.mark_of(built), max_rounds=3, where="marked")
    assert sum(exp["forms"].values()) == len(C.SIZES)  # (every other group is taken)
