"""What the inputs of tests/group_sort_trips_cases.py are there for, shown without a GPU: each of three mistakes that the
one-trip form of the window rounds (group_sort.hpp) could make gives another answer than tests/group_sort_model.py on them.
The mistakes are put into the model from outside (the model file stays as it is):
  * a window cut one word early: the window of a segment that scanned starts one 64-bit word in front of the scan's result;
  * a scan that stops at word 7 instead of word 8;
  * a clamp that changes a compared word: the last word of the text reads as the word in front of it.
Also: the model's answer on these inputs is the suffix order (Text.compare), and the situations the inputs are named
after do occur in them.
"""
import numpy as np
import pytest

import group_sort_model as M
import group_sort_trips_cases as C

KEYS = ("sa", "out_lo", "lcp_list", "min_depth")


def run(built, max_rounds=M.ROUNDS, text=None):
    return M.model(text or built.text, built.listed, C.H0, False, max_rounds, M.NONE, None)


def differs(a, b):
    return any(not np.array_equal(a[k], b[k]) for k in KEYS)


def early_window(monkeypatch):
    """scans report one word less (not in front of their start): the minimum, and so the window, moves with them"""
    real = M._first_diff
    monkeypatch.setattr(M, "_first_diff", lambda codes, pa, pb, start, end: np.maximum(start, real(codes, pa, pb, start, end) - C.PER))


def clamped(text):
    """the same text whose last word reads as the word in front of it"""
    other = M.Text(text.data)
    other.codes = text.codes.copy()
    other.codes[text.n - C.PER:text.n] = text.codes[text.n - 2 * C.PER:text.n - C.PER]
    return other


@pytest.mark.parametrize("k", (3, 66))
@pytest.mark.parametrize("second", C.SECOND)
@pytest.mark.parametrize("first", list(C.FIRST))
def test_the_model_sorts_the_difference_cases(first, second, k):
    built = C.diff_case(first, second, k)
    text, lst = built.text, built.listed
    got = run(built)
    assert got["tied"] == 0 and got["min_depth"] == M.NONE
    order = got["sa"][lst.slot]
    for a, b, lcp in zip(order[:-1], order[1:], got["lcp_list"][1:]):
        sign, exact = text.compare(int(a), int(b))
        assert sign < 0 and exact == lcp, (a, b, exact, lcp)
    # the earliest difference stands where the case says, and nothing differs in front of it
    members = np.sort(lst.sa[lst.slot].astype(np.int64))
    lcps = [text.lcp(int(members[0]), int(x)) for x in members[1:]]
    assert min(lcps) == C.FIRST[first] and sorted(lcps)[1] == C.FIRST[first] + second


@pytest.mark.parametrize("k", (3, 66))
@pytest.mark.parametrize("first", list(C.FIRST))
def test_a_window_cut_one_word_early_is_told(monkeypatch, first, k):
    """the member that differs 63 symbols into the window leaves in the second round; one word early it stays tied"""
    built = C.diff_case(first, 63, k)
    good = run(built, 2)
    early_window(monkeypatch)
    assert differs(good, run(built, 2)), (first, k)


@pytest.mark.parametrize("k", (3, 66))
@pytest.mark.parametrize("first", ("word7_last_bit", "word8_stop"))
def test_a_scan_that_stops_at_word_7_is_told(monkeypatch, first, k):
    built = C.diff_case(first, 63, k)
    good = run(built, 2)
    monkeypatch.setattr(M, "SCAN_WORDS", 7)
    assert differs(good, run(built, 2)), (first, k)


def test_word_0_does_not_tell_the_scan_length(monkeypatch):
    """(what the two cases above are needed for: a difference in word 0 gives the same answer with seven words)"""
    built = C.diff_case("word0", 63, 3)
    good = run(built, 2)
    monkeypatch.setattr(M, "SCAN_WORDS", 7)
    assert not differs(good, run(built, 2))


@pytest.mark.parametrize("k", (8, 70, 140))
def test_a_clamp_that_changes_a_compared_word_is_told(k):
    built = C.ends_case(k)
    text = built.text
    last = int(np.sort(built.listed.sa[built.listed.slot])[-1])
    assert text.lim[last] == 98 and last + 98 == text.n  # the scan from 78 would read 236 symbols past the end
    for max_rounds in (2, M.ROUNDS):
        assert differs(run(built, max_rounds), run(built, max_rounds, clamped(text))), (k, max_rounds)


@pytest.mark.parametrize("k", (8, 70, 140))
def test_the_ends_case_holds_what_it_is_named_after(k):
    built = C.ends_case(k)
    text, lst = built.text, built.listed
    lims = np.sort(text.lim[lst.sa[lst.slot]])
    # the depth of the second round is 98 (the end of the text): one member ends on the window's first symbol, one inside
    # the window [98, 162) at 128, two at 138 with different terminators, one inside the scanned words behind it
    assert lims[0] == 98 and 128 in lims and (lims == 138).sum() == 2 and 178 in lims
    twins = lst.sa[lst.slot][text.lim[lst.sa[lst.slot]] == 138]
    assert text.term[twins[0]] != text.term[twins[1]]
    got = run(built)
    assert got["tied"] == 0
    order = got["sa"][lst.slot]
    for a, b, lcp in zip(order[:-1], order[1:], got["lcp_list"][1:]):
        sign, exact = text.compare(int(a), int(b))
        assert sign < 0 and exact == lcp


def test_sizes_and_queue_cases_are_what_they_say():
    for size in C.SIZES:
        for with_small in (False, True):
            lst = C.sizes_case(size, with_small).listed
            sizes = np.unique(lst.grp, return_counts=True)[1]
            assert size in sizes and (len(sizes) == 1) == (not with_small)
    built = C.many_items_case()
    sizes = np.unique(built.listed.grp, return_counts=True)[1]
    assert (sizes == 65).all() and sizes.size >= 300
    blocks = -(-built.listed.slot.size // 256)
    assert blocks < 256 and sizes.size > 2 * blocks  # more items per shard than the two workgroups a shard has here
    for k in (70, 130):
        for max_rounds in (1, 2, M.ROUNDS):
            got = run(C.equal_case(k), max_rounds)
            assert got["tied"] > 0 and got["rounds"] == max_rounds
