"""What the inputs of tests/test_gpu_group_sort.py are there for, shown without a GPU (tests/group_sort_model.py):

  * the round-level model (b) against the definition (a) on every case and run: whatever the rounds did, positions in
    different classes are in true suffix order, every decided LCP is the true one, every class left tied agrees on at least
    min_depth symbols, every taken group's output is a permutation of its input, tied classes keep their input order;
  * guaranteed progress: window rounds separate every pair that differs within max_rounds windows behind h0, and the pivot
    rounds finish the collections of mutated copies within their budget, in about log2 k rounds;
  * for every named mistake a named case whose expected output changes when the mistake is switched on in the model;
  * the edges the issue lists are really in the inputs (residues, halves, code bits, tile places, queue loads, window tags);
  * the builder refuses groups that do not agree on h0 symbols.
"""
import functools
import math

import numpy as np
import pytest

import group_sort_model as M


def classes_of(got, e0, e1):
    """first positions of the classes of the taken group on list positions [e0, e1)"""
    lcp = got["lcp_list"]
    return [e for e in range(e0, e1) if e == e0 or lcp[e] != M.PENDING]


def check_sound(text, lst, h0, got, pivot, max_rounds, full_sort_budget=4000):
    """(b) against (a) for one run; -> taken groups"""
    slot, grp = lst.slot.astype(np.int64), lst.grp.astype(np.int64)
    m = slot.size
    first = np.nonzero(np.concatenate([[True], grp[1:] != grp[:-1]]))[0]
    ends = np.concatenate([first[1:], [m]])
    outside = np.ones(text.n, dtype=bool)
    outside[slot] = False
    assert np.array_equal(got["sa"][outside], lst.sa[outside])
    min_depth, taken = got["min_depth"], 0
    for e0, e1 in zip(first, ends):
        before, after = lst.sa[slot[e0:e1]].astype(np.int64), got["sa"][slot[e0:e1]].astype(np.int64)
        if got["lcp_list"][e0] == M.PENDING:  # not taken: in place, one group
            assert np.array_equal(before, after) and not got["out_lo"][e0:e1].any()
            assert (got["lcp_list"][e0:e1] == M.PENDING).all()
            continue
        taken += 1
        assert got["lcp_list"][e0] == 0
        assert np.array_equal(np.sort(before), np.sort(after))
        place = {int(p): k for k, p in enumerate(before)}
        starts = classes_of(got, e0, e1)
        cls_of = np.searchsorted(starts, np.arange(e0, e1), side="right") - 1
        assert np.array_equal(got["out_lo"][e0:e1], np.array(starts)[cls_of] - e0)
        # neighbours: a boundary is decided as the definition decides it; inside a class the input order is kept
        agree = {}
        for e in range(e0 + 1, e1):
            a, b = int(after[e - 1 - e0]), int(after[e - e0])
            sign, lcp = text.compare(a, b)
            if got["lcp_list"][e] != M.PENDING:
                assert sign < 0 and lcp == got["lcp_list"][e], (e, a, b, sign, lcp, got["lcp_list"][e])
            else:
                assert place[a] < place[b], "a tied class does not keep its input order"
                agree[cls_of[e - e0]] = min(agree.get(cls_of[e - e0], 1 << 40), lcp)
        # a class left tied agrees on more symbols than either boundary beside it decides -- with the ordered neighbours
        # that puts EVERY member of a class in front of every member of the next one -- and on at least min_depth
        for c, depth in agree.items():
            assert min_depth != M.NONE and depth >= min_depth, (c, depth, min_depth)
            flank = [got["lcp_list"][starts[k]] for k in (c, c + 1) if 0 < k < len(starts)]
            assert all(f < depth for f in flank)
            if not pivot:  # every window of two words separates what differs inside it
                assert depth >= h0 + max_rounds * 2 * text.per
        if e1 - e0 >= 3 and e1 - e0 <= full_sort_budget:  # the same by a full sort with the definition, while the budget lasts
            full_sort_budget -= e1 - e0
            truth = sorted(after.tolist(), key=functools.cmp_to_key(lambda a, b: text.compare(a, b)[0]))
            rank = {p: k for k, p in enumerate(truth)}
            r = np.array([rank[int(p)] for p in after])
            for k in range(1, len(starts)):
                assert r[:starts[k] - e0].max() < r[starts[k] - e0:].min()
    return taken


@pytest.mark.parametrize("name", list(M.CASES))
def test_model_agrees_with_the_definition(name):
    case = M.CASES[name]
    text = M.text_of(case.text)
    for order, pivot, max_rounds, depth_cap, marked in M.runs_of(name):
        got = M.expected(name, order, pivot, max_rounds, depth_cap, marked)
        taken = check_sound(text, M.listed(name, order), case.h0, got, pivot, max_rounds)
        assert taken == sum(got["forms"].values())
        if marked:
            assert 0 < taken < len(M.chosen_groups(name))


def test_every_form_mode_and_width_is_reached():
    seen = {}
    for name, case in M.CASES.items():
        for order, pivot, max_rounds, depth_cap, marked in M.runs_of(name):
            got = M.expected(name, order, pivot, max_rounds, depth_cap, marked)
            for form, count in got["forms"].items():
                key = (form, pivot, M.text_of(case.text).bits)
                seen[key] = seen.get(key, 0) + count
    for form in ("tiled", "m128", "m256", "m1024"):
        for pivot in (False, True):
            for bits in (2, 4, 8):
                assert seen.get((form, pivot, bits), 0) > 0, (form, pivot, bits)
    print(sorted(seen.items()))


@pytest.mark.parametrize("k", [5, 17, 65, 300, 1024])
def test_pivot_rounds_finish_mutated_copies(k):
    name = f"mutated_{k}"
    for order in M.ORDERS:
        got = M.expected(name, order, True, M.ROUNDS, M.NONE, False)
        assert got["tied"] == 0 and got["min_depth"] == M.NONE
        assert got["rounds"] <= 2 * math.ceil(math.log2(k)) + 2 <= M.ROUNDS, got["rounds"]


def test_exact_copies_stay_tied_at_the_cap():
    got = M.expected("periodic", "shuffle", True, M.ROUNDS, 14 + 1000, False)
    assert got["tied"] >= 100 and got["min_depth"] == 14 + 1000
    got = M.expected("periodic", "shuffle", True, 3, 14 + 5000, False)  # out of rounds below the cap
    assert got["tied"] >= 100 and 14 + M.PIVOT_WORDS * 32 <= got["min_depth"] <= 14 + 3 * M.PIVOT_WORDS * 32


NAMED = {  # mistake -> (case, order, pivot, max_rounds, depth_cap - h0, marked)
    "mask_more": ("terms_251", "text", False, 24, None, False),
    "mask_fewer": ("terms_251", "text", False, 24, None, False),
    "no_tt": ("terms_251", "text", False, 24, None, False),
    "no_term_index": ("terms_3", "text", False, 24, None, False),
    "lcp_no_valid": ("terms_251", "text", False, 24, None, False),
    "no_second_word": ("deep_w2", "text", False, 24, None, False),
    "scan_no_limit": ("terms_5", "text", False, 24, None, False),
    "scan_no_stop": ("deep_w2", "text", False, 2, None, False),
    "unstable": ("deep_w2", "text", False, 1, None, False),
    "above_ascending": ("mutated_17", "text", True, 24, None, False),
    "no_sym_tiebreak": ("hotspots_w8", "text", True, 24, None, False),
    "lcp_wrong_neighbour": ("mutated_17", "text", True, 24, None, False),
    "cap_gt": ("capedge", "text", True, 24, 7, False),
    "take_1025": ("size_1025_w2", "text", False, 24, None, False),
    "mark_at_g": ("equalise", "text", False, 3, None, True),
    "no_capped_depth": ("periodic", "text", True, 24, 1000, False),
}


@pytest.mark.parametrize("bug", M.BUGS)
def test_every_named_mistake_changes_a_named_case(bug):
    name, order, pivot, max_rounds, cap, marked = NAMED[bug]
    case = M.CASES[name]
    run = (order, pivot, max_rounds, M.NONE if cap is None else case.h0 + cap)
    assert run + (marked,) in set(M.runs_of(name)), "not a run of the GPU test"
    good, bad = M.expected(name, *run, marked), M.expected(name, *run, marked, bug=bug)
    assert any(not np.array_equal(good[k], bad[k]) for k in ("sa", "out_lo", "lcp_list", "min_depth")), bug


def test_capedge_is_the_class_that_ends_at_the_cap():
    """x and y leave the pivot at cap - 1 with the same symbol and x ends at the cap: one class, tied at the cap"""
    got = M.expected("capedge", "text", True, 24, 14 + 7, False)
    assert got["out_lo"].tolist() == [0, 1, 1] and got["min_depth"] == 21 and got["lcp_list"].tolist() == [0, 20, M.PENDING]


@pytest.mark.parametrize("bits", [2, 4, 8])
def test_deep_case_has_every_depth_residue_half_and_code_bit(bits):
    name = f"deep_w{bits}"
    text, h0, per = M.text_of(f"deep:{bits}"), M.H0[bits], 64 // bits
    assert text.bits == bits and not text.segmented
    depths, residues, halves, xors = set(), set(), set(), set()
    for g in M.chosen_groups(name):
        for a, b in zip(g[:-1], g[1:]):
            d = text.lcp(int(a), int(b))
            depths.add(d - h0)
            for p in (int(a), int(b)):
                residues.add((p + d) % per)
                halves.add((p + d) * bits % 64 // 32)
            xors.add(int(text.codes[a + d]) ^ int(text.codes[b + d]))
    assert depths >= set(range(0, M.PIVOT_WORDS * per + 3))  # window, scan and pivot-round edges, one to either side
    assert residues == set(range(per)) and halves == {0, 1}
    assert {1, 1 << (bits - 1)} <= xors
    reach = h0 + 2 * (M.SCAN_WORDS + 2) * per  # two rounds of scan and window: ties beyond stay
    assert max(depths) + h0 > reach and M.expected(name, "text", False, 2, M.NONE, False)["tied"] > 0
    caps = {c - h0 for _, pv, rounds, c, _ in M.runs_of(name) if pv and c != M.NONE and rounds == M.ROUNDS}
    assert any(c <= 0 for c in caps) and any(c % per for c in caps if c > 0) and any(c % per == 0 for c in caps if c > 0)
    assert all({c - 1, c, c + 1} <= depths for c in caps if c > 0)


def test_verydeep_outlasts_24_rounds():
    for bits in (2, 8):
        text, h0 = M.text_of(f"verydeep:{bits}"), M.H0[bits]
        got = M.expected(f"verydeep_w{bits}", "text", False, M.ROUNDS, M.NONE, False)
        sizes = sorted(len(g) for g in M.chosen_groups(f"verydeep_w{bits}"))
        assert sizes == [2, 2, 2, 3, 3, 3]
        assert text.lcp(0, 8200 + 1 + 150 + 1) > h0 + M.ROUNDS * (M.SCAN_WORDS + 2) * text.per
        assert got["tied"] == 12 and got["rounds"] == M.ROUNDS and got["min_depth"] != M.NONE  # the triples lose one member each


def test_tiles_case_places():
    lst = M.listed("tiles", "text")
    first = np.nonzero(np.concatenate([[True], lst.grp[1:] != lst.grp[:-1]]))[0]
    size = np.diff(np.concatenate([first, [lst.slot.size]]))
    crossing = {int(f % 64) for f, s in zip(first, size) if s <= 64 and f % 64 + s > 64}
    assert crossing >= {1, 62, 63} and 0 in first % 64
    assert any(a > 64 and b <= 64 for a, b in zip(size[:-1], size[1:]))  # a small group right behind a large one
    assert lst.slot.size % 64 != 0 and lst.slot.size - (lst.slot.size // 64) * 64 < 128


def test_queue_case_loads():
    lst = M.listed("queues", "text")
    m = lst.slot.size
    blocks = -(-m // 256)
    assert blocks > 256 and m <= 80000  # several workgroups of group_dir_kernel per shard
    last = np.nonzero(np.concatenate([lst.grp[1:] != lst.grp[:-1], [True]]))[0]
    per_shard = np.bincount((last // 256) % 256, minlength=256)
    grid_y = min(64, max(1, -(-m // (256 * 64))))
    assert per_shard.max() > grid_y  # a shard holds more items than gridDim.y
    assert not [g for g in M.chosen_groups("small_only") if len(g) > 64]


def test_terminator_cases():
    for count in (2, 3, 4, 5, 33, 251):
        text = M.text_of(f"terms:{count}")
        assert text.segmented and text.bits == 2 and text.terms.size == count
    text, h0 = M.text_of("terms:251"), 14
    members = np.concatenate(M.chosen_groups("terms_251"))
    assert set(np.minimum(text.lim[members] - h0, 64).tolist()) == set(range(65))  # every length inside the window, 0 = ends at h0
    assert (members >= text.n - 9 * 32).any()  # the padded reads behind the text
    same = ends_on_zero = 0
    for name in ("terms_3", "terms_5", "terms_251"):
        t = M.text_of(M.CASES[name].text)
        for g in M.chosen_groups(name):
            for a, b in zip(g[:-1], g[1:]):
                lcp = t.lcp(int(a), int(b))
                same += lcp == t.lim[a] == t.lim[b]
                short, long_ = (a, b) if t.lim[a] < t.lim[b] else (b, a)
                ends_on_zero += lcp == t.lim[short] < t.lim[long_] and t.codes[long_ + lcp] == 0
    assert same >= 2 and ends_on_zero >= 2


def test_builder_refuses_bad_groups():
    text = M.text_of("sizes:2")
    good = M.chosen_groups("size_3_w2")
    M.lay_out(text, 14, good)
    other = M.chosen_groups("size_2_w2")[0]
    with pytest.raises(ValueError):
        M.lay_out(text, 14, [np.concatenate([good[0], other])])  # two groups as one: no agreement on h0 symbols
    with pytest.raises(ValueError):
        M.lay_out(text, 40, [good[0]])  # ... nor on more symbols than head and digits are long
    with pytest.raises(ValueError):
        M.lay_out(text, 14, [good[0][:1]])
    with pytest.raises(ValueError):
        M.lay_out(text, 14, [np.array([text.n - 3, text.n - 2])])  # members that end in front of h0
    with pytest.raises(ValueError):
        M.lay_out(text, 14, [good[0], good[0]])
