"""What the inputs of tests/test_gpu_direct_round.py are there for, shown without a GPU (tests/direct_round_model.py):

  * the round-level model (b) against the definition (a) on every case and run: every boundary the model declares decided
    has the order and the LCP of Text.compare, every class it leaves tied agrees on the depth its tile reports (and so on
    min_depth[0]), every group it calls untouched comes back unchanged, the new list is exactly the members that are
    still tied, in slot order, each with the head slot of its class;
  * the union of the branches the model reports over the cases holds every branch of the kernel, and the sizes, tile
    places, list lengths, pair counts and busy-lane counts the issue lists are really in the inputs;
  * for every named mistake the cases whose expected output changes when the mistake is switched on in the model.
"""
import numpy as np
import pytest

import direct_round_model as D

PENDING_MIN = D.PENDING - 64   # kLcpPendingMin


def runs():
    return [(name, order, flags) for name in D.CASES for order, flags in D.runs_of(name)]


def check_sound(text, lst, h0, cap, got):
    slot, grp = lst.slot.astype(np.int64), lst.grp.astype(np.int64)
    m, n = slot.size, text.n
    before = D.lcp_before(n)
    first = np.nonzero(np.concatenate([[True], grp[1:] != grp[:-1]]))[0] if m else np.zeros(0, dtype=np.int64)
    ends = np.concatenate([first[1:], [m]]).astype(np.int64)
    outside = np.ones(n, dtype=bool)
    outside[slot] = False
    assert np.array_equal(got["sa"][outside], lst.sa[outside])
    assert np.array_equal(got["lcp"][outside], before[outside]) and (got["rank_by_slot"][outside] == D.FILL).all()
    tied_slots, tied_heads = [], []
    depths = []
    assert set(got["groups"]) == set(grp[first].tolist())
    for e0, e1 in zip(first, ends):
        head = int(grp[e0])
        s0, s1 = head, head + int(e1 - e0)
        inp, after = lst.sa[s0:s1].astype(np.int64), got["sa"][s0:s1].astype(np.int64)
        assert got["lcp"][s0] == before[s0], "the head entry of a group is left alone"
        if got["groups"][head] == "untouched":  # in place, one group, everybody goes on
            assert np.array_equal(inp, after) and np.array_equal(got["lcp"][s0:s1], before[s0:s1])
            assert (got["rank_by_slot"][s0:s1] == head + 1).all()
            tied_slots += range(s0, s1)
            tied_heads += [head] * (s1 - s0)
            continue
        assert np.array_equal(np.sort(inp), np.sort(after))
        place = {int(p): k for k, p in enumerate(inp)}
        depth = got["depth"][head]
        assert h0 < depth < cap + D.window(text.bits)
        cls_head = s0
        members = [s0]
        for s in range(s0 + 1, s1 + 1):
            if s < s1 and got["lcp"][s] == D.COMPARED:  # no boundary: the class goes on, in input order
                a, b = int(after[s - 1 - s0]), int(after[s - s0])
                assert text.lcp(a, b) >= depth, (s, a, b, text.lcp(a, b), depth)
                assert place[a] < place[b], "a tied class does not keep its input order"
                members.append(s)
                continue
            # the class [cls_head, s) is complete
            assert (got["rank_by_slot"][cls_head:s] == cls_head + 1).all()
            if len(members) > 1:
                tied_slots += members
                tied_heads += [cls_head] * len(members)
                depths.append(depth)
            if s < s1:
                a, b = int(after[s - 1 - s0]), int(after[s - s0])
                sign, lcp = text.compare(a, b)
                assert got["lcp"][s] < PENDING_MIN
                assert sign < 0 and lcp == got["lcp"][s], (s, a, b, sign, lcp, got["lcp"][s])
                assert lcp < depth
                cls_head, members = s, [s]
    assert got["new_m"] == len(tied_slots)
    assert got["new_slot"].tolist() == tied_slots and got["new_grp"].tolist() == tied_heads
    assert got["min_depth"][0] == (min(depths) if depths else D.NONE)
    untouched = [h for h, v in got["groups"].items() if v == "untouched"]
    assert got["min_depth"][1] == (h0 if untouched else D.NONE)


@pytest.mark.parametrize("name", list(D.CASES))
def test_model_agrees_with_the_definition(name):
    c = D.CASES[name]
    text, groups = D.made(name)
    assert len(groups) > 0, "a case that lists nothing"
    for order, flags in D.runs_of(name):
        check_sound(text, D.listed(name, order), c.h0, c.cap, D.expected(name, order, bool(flags & D.NO_STRAGGLERS)))


def test_every_branch_size_place_and_count_is_reached():
    seen, sizes, places, lengths, pairs, busy = set(), {}, set(), set(), set(), set()
    for name, order, flags in runs():
        got = D.expected(name, order, bool(flags & D.NO_STRAGGLERS))
        seen |= D.branches_of(got)
        lst = D.listed(name, order)
        lengths.add(lst.slot.size)
        first = np.nonzero(np.concatenate([[True], lst.grp[1:] != lst.grp[:-1]]))[0]
        size = np.diff(np.concatenate([first, [lst.slot.size]]))
        for f, s in zip(first, size):
            sizes.setdefault(int(s), set()).add(D.CASES[name].bits)
            places.add(int(f % D.TILE))
        for br in got["tiles"]:
            pairs.add(br["pairs"])
            busy |= set(br["busy"])
    assert seen == set(D.BRANCHES), set(D.BRANCHES) - seen
    for s in D.SIZES:
        assert sizes.get(s) == {2, 4, 8}, s
    assert places >= {0, 1, 190, 191} and lengths >= {2, 191, 192, 193}
    assert {D.PAIR_CAP, D.PAIR_CAP + 1} <= pairs and {32, 33, 64, 65} <= busy
    assert max(lengths) > 64 * D.TILE and all(k <= 13000 for k in lengths)
    assert all(D.made(name)[0].n <= 40000 for name in D.CASES)


def test_the_edges_the_cases_are_named_for():
    # a group alone at tile places 190 and 191 that runs into the span; the 64-member group that ends on thread 254
    for name, place, size in (("tile_190_1", 190, 3), ("tile_191_64", 191, 64), ("tile_191_58", 191, 58), ("tile_190_19", 190, 19)):
        lst = D.listed(name, "text")
        first = np.nonzero(np.concatenate([[True], lst.grp[1:] != lst.grp[:-1]]))[0]
        size_of = dict(zip(first.tolist(), np.diff(np.concatenate([first, [lst.slot.size]])).tolist()))
        assert size_of[place] == size
    assert 193 in np.nonzero(np.diff(D.listed("tile_190_1", "text").grp))[0] + 1  # a group at place 1 of the second tile
    # a 300-member group over three tiles: tile 1 starts no group, all its 192 main threads stay, its span is not reported
    for order in ("text", "shuffle"):
        got = D.expected("group_300_three_tiles", order)
        assert len(got["tiles"]) == 3 and (got["tiles"][1]["starts"], got["tiles"][1]["stays"], got["tiles"][1]["pairs"]) == (0, 192, 0)
        assert got["tiles"][0]["stays"] == 92 and got["tiles"][2]["stays"] == 16 and got["tiles"][2]["handled"] == 5
        assert got["new_slot"].tolist()[:300] == list(range(100, 400))
        assert changed("group_300_three_tiles", order, 0, "span_owner")
    # a group of 58 from place 191 that IS handled: the pair list, the fetch and the epilogue run on threads up to 248
    for order in ("text", "shuffle"):
        got, lst = D.expected("tile_191_58_handled", order), D.listed("tile_191_58_handled", order)
        assert got["groups"][int(lst.grp[191])] == "handled" and got["tiles"][0]["last handled thread"] == 248
        assert got["tiles"][0]["span-crossing"] == 1 and got["tiles"][0]["pairs"] == 1653
    # bail-out: 64 busy lanes after the second window go on, 65 stop at h0 + 2 windows; 32 go to the straggler loop, 33 stay
    for bits in (2, 8):
        h0, W = D.H0[bits], D.window(bits)
        b32, b33, b64, b65 = (D.expected(f"busy_{k}_w{bits}", "text") for k in (32, 33, 64, 65))
        assert b32["tiles"][0]["busy"] == [32] and b32["tiles"][0]["straggler trips"] == 1
        assert b33["tiles"][0]["busy"] == [33, 33, 0] and not b33["tiles"][0]["straggler trips"]
        assert b64["tiles"][0]["busy"] == [64, 64, 0] and not b64["tiles"][0]["bail-out"] and b64["new_m"] == 0
        assert b65["tiles"][0]["busy"] == [65, 65] and b65["tiles"][0]["bail-out"] and b65["new_m"] == 130
        assert b65["min_depth"][0] == h0 + 2 * W
    # the straggler loop: trips of four and of two windows; more than 64 members on 32 lanes
    got = D.expected("stragglers_32", "text")
    assert got["tiles"][0]["straggler trips"] == 2 and got["tiles"][0]["tied-at-cap"] and got["min_depth"][0] == 16 + 7 * 128
    for k in (1, 2):  # one and two tied pairs, decided in window 1, 4 (first trip), 5 and in the partial last trip
        trips = [D.expected(f"stragglers_{k}_win{win}", "text")["tiles"][0]["straggler trips"] for win in (1, 4, 5, 6)]
        assert trips == [1, 1, 2, 2]
        for win in (1, 4, 5, 6):
            got, ns = D.expected(f"stragglers_{k}_win{win}", "text"), D.expected(f"stragglers_{k}_win{win}", "text", True)
            assert got["new_m"] == 0 and ns["tiles"][0]["busy"] == [k] * win + [0]
    got = D.expected("straggler_overflow", "text")
    assert got["tiles"][0]["busy"] == [32] and got["tiles"][0]["pairs"] == 318 and got["tiles"][0]["straggler-overflow"]
    assert got["new_m"] == 66 and got["min_depth"][0] == 16 + 128
    assert D.expected("straggler_overflow", "text", True)["new_m"] == 0   # NO_STRAGGLERS: the rounds finish them
    # a window that would start behind the end of the text is not fetched -- and never compared (the model asserts it)
    for name in ("ends_in_window_1_text_end_w2", "ends_in_window_1_text_end_w8"):
        br = D.expected(name, "text")["tiles"][0]
        assert br["guard-skipped window"] >= 3 and br["terminator-decided"] >= 1
    assert D.expected("ends_in_window_2_terminator", "text")["tiles"][0]["terminator-decided"] >= 1
    # the pair cap: 1664 pairs are all handled, with 1665 the last group stays; a group of 59 stays alone
    assert D.expected("paircap_1664", "text")["new_m"] == 0 and D.expected("paircap_19s", "text")["new_m"] == 0
    for name in ("paircap_1665", "paircap_19s_more"):
        got = D.expected(name, "text")
        assert got["new_m"] == 2 and got["min_depth"][1] == 16 and got["tiles"][0]["overflow-rest"] == 1
    got = D.expected("prefix_59_rest", "text")
    assert (got["tiles"][0]["overflow-prefix"], got["tiles"][0]["overflow-rest"]) == (2, 4)
    assert D.expected("first_59", "text")["tiles"][0]["overflow-prefix"] == 0
    # min_depth[2]: tiles 0 and 64 count their 70 untouched members each, tiles 1 and 63 hold as many and do not count
    got = D.expected("untouched_counter", "text")
    assert len(got["tiles"]) == 65 and [k for k, br in enumerate(got["tiles"]) if br["large"]] == [0, 1, 63, 64]
    assert got["min_depth"][2] == 140 and got["new_m"] >= 280


@pytest.mark.parametrize("bits", [2, 4, 8])
def test_deep_cases_have_every_offset_residue_half_and_code_bit(bits):
    h0, W, per = D.H0[bits], D.window(bits), 64 // bits
    seen, xors = set(), set()
    in_triple = set()
    for name in D.CASES:
        if not name.startswith(f"deep_w{bits}_"):
            continue
        text, groups = D.made(name)
        for g in groups:
            for a, b in zip(g[:-1], g[1:]):
                d = text.lcp(int(a), int(b))
                for p in (int(a), int(b)):
                    seen.add((d - h0, p % per))
                    if len(g) == 3:
                        in_triple.add((d - h0, p % per))
                if d - h0 < W:
                    xors.add(int(text.codes[a + d]) ^ int(text.codes[b + d]))
    want = {(o, r) for o in range(W + 2) for r in range(per)}  # every symbol of the window and one behind it, every residue
    assert want <= seen and {(o, r) for o in range(W // 2) for r in range(per)} <= in_triple
    assert {1, 1 << (bits - 1)} <= xors
    # the edges of windows and caps
    text, groups = D.made(f"edges_w{bits}")
    depths = {text.lcp(int(g[0]), int(g[1])) - h0 for g in groups} | {text.lcp(int(g[-2]), int(g[-1])) - h0 for g in groups}
    for cap in (D.CASES[f"edges_w{bits}"].cap, D.CASES[f"edges_past_cap_w{bits}"].cap):
        assert {0, W - 1, W, cap - h0 - 1, cap - h0, cap - h0 + 1} <= depths
    assert (D.CASES[f"edges_w{bits}"].cap - h0) % W == 0 and (D.CASES[f"edges_past_cap_w{bits}"].cap - h0) % W != 0


def test_terminator_cases():
    W = D.window(2)
    for count in (1, 2, 3, 4, 5, 33, 251):
        text, groups = D.made(f"terms_{count}")
        assert text.bits == 2 and text.terms.size == count and text.segmented == (count > 1)
    text, groups = D.made("terms_251")
    members = np.concatenate(groups)
    assert set(np.minimum(text.lim[members] - 16, W).tolist()) == set(range(W + 1))  # every length inside the window, 0 = ends at h0
    same = nearer = 0
    for g in groups:
        for a, b in zip(g[:-1], g[1:]):
            lcp = text.lcp(int(a), int(b))
            same += lcp == text.lim[a] == text.lim[b]
            nearer += lcp == min(text.lim[a], text.lim[b]) and text.lim[a] != text.lim[b]
    assert same >= 2 and nearer >= 2


def changed(name, order, flags, bug):
    ns = bool(flags & D.NO_STRAGGLERS)
    good, bad = D.expected(name, order, ns), D.expected(name, order, ns, bug=bug)
    return (good["new_m"] != bad["new_m"] or good["min_depth"] != bad["min_depth"] or
            any(not np.array_equal(good[k], bad[k]) for k in ("sa", "lcp", "rank_by_slot", "new_slot", "new_grp")))


@pytest.mark.parametrize("bug", D.BUGS)
def test_every_named_mistake_changes_a_case(bug):
    small = [r for r in runs() if D.listed(r[0], r[1]).slot.size <= 3000]
    hit = [r for r in small if changed(*r, bug)]
    print(f"{bug}: {len(hit)} of {len(small)} runs change, e.g. {sorted({r[0] for r in hit})[:8]}")
    assert hit, bug


def test_builder_refuses_bad_groups():
    text, groups = D.made("size_3_w2")
    D.lay_out(text, 16, groups)
    other = D.made("size_3_w2")[0]
    with pytest.raises(ValueError):
        D.lay_out(text, 40, groups)                                   # no agreement on that many symbols
    with pytest.raises(ValueError):
        D.lay_out(text, 16, [groups[0][:1]])
    with pytest.raises(ValueError):
        D.lay_out(text, 16, [np.array([other.n - 3, other.n - 2])])   # members that end in front of h0
