"""The first direct round of the suffix-array construction (sa_direct.hip: group_refine_kernel at 2, 4 and 8 bits per
symbol and the compaction of what it leaves tied) on caller groups, through nolzss_debug_direct_round -- the launch
function of the construction itself, the only launch site of the kernel -- against the round-level model of
tests/direct_round_model.py by integer equality: sa, lcp and rank_by_slot over all n entries (what the round must not
touch included), the next active list and its length, and the three min_depth words.
tests/test_direct_round_model_host.py proves without a GPU that the model agrees with the definition of the suffix order,
that every branch of the kernel is reached and what every input is there for.

The inputs (direct_round_model.CASES), at most 40 000 symbols and 12 500 list entries per call:
  size_*, sizes_*          groups of 2, 3, 18, 19, 58, 59, 63 .. 66, 128 and 300 members, alone and in one list with gaps, in
                           text order, reversed and shuffled; h0 16 and 17 at 2 bits, 8 at 4 bits, 4 at 8 bits
  m_*, tile_*, group_*     lists of 2, 191, 192 and 193 entries; groups at tile places 0, 1, 190 and 191 that run into the
                           span, a 64-member group from place 191 and a handled group of 58 that ends on thread 248; 65, 128
                           and 300 members with small groups behind them, the 300 over three tiles
  paircap_*, prefix_59_rest, first_59, overflow_no_large
                           tiles that need exactly 1664 pairs and one more; a handled prefix in front of a group of 59 and
                           small groups that must stay; nothing handled; an overflow with no large group
  deep_*, edges_*          a first difference at every symbol of a window and one behind it, at every residue of the start
                           position modulo a word, lowest and highest code bit, in pairs and inside triples; differences
                           around the window edges and around a cap that is and is not a multiple of the window
  busy_*                   32 / 33 busy lanes after the first window (straggler loop or not), 64 / 65 after the second
                           (goes on or bails out with the ties at h0 + 2 windows)
  stragglers_*, ends_*     1 and 2 tied pairs (once per window), 32 tied pairs and nine triples decided in windows 1, 4, 5, in the partial last trip, or
                           tied at the cap; a shorter member that ends inside a straggler window or on its edge, at the end
                           of the text and at a terminator; windows that would start behind the end of the text
  tied_classes*            several classes of one group tied at the cap
  straggler_overflow*      66 tied members on 32 busy lanes
  terms_*, terms_gs_*      terminator tables of 1, 2 .. 4, 5, 33 and 251 entries; every length inside the window; the
                           texts of the group-sort model's terminator_text as they are
  mutated_*, periodic_*    5 .. 64 mutated and exact copies
  untouched_counter        65 tiles with groups of 70 in tiles 0, 1, 63 and 64
Every case runs with flags 0; those that name it also with NO_STRAGGLERS (against a model run of its own) and with TIMED
(which must equal the untimed result in every output).
"""
import numpy as np
import pytest

import direct_round_model as D

pytestmark = pytest.mark.gpu

OUTPUTS = ("sa", "lcp", "rank_by_slot", "new_slot", "new_grp")


@pytest.fixture(scope="module")
def native():
    from nolzss_amd import _noLZSS as native
    assert native.device_count() >= 1, "no MI355X visible"
    return native


def call(native, name, order, flags):
    c = D.CASES[name]
    text, lst = D.made(name)[0], D.listed(name, order)
    return native.debug_direct_round(text.data, lst.sa, lst.slot, lst.grp, c.h0, c.cap, flags, D.lcp_before(text.n), D.FILL)


def run_one(native, name, order, flags, with_ranks=True):
    """one call of the hook, everything it returns against the model; -> (the model's account of what ran, the results)"""
    text = D.made(name)[0]
    exp = D.expected(name, order, bool(flags & D.NO_STRAGGLERS))
    got = call(native, name, order, flags | (D.WITH_RANKS if with_ranks else 0))
    where = (name, order, flags)
    assert (got["bits"], got["terms"], got["segmented"]) == (text.bits, text.terms.size, text.segmented), where
    print(f"{where}: new_m {got['new_m']} (model {exp['new_m']}), min_depth {got['min_depth']} (model {exp['min_depth']})")
    assert got["new_m"] == exp["new_m"], where
    for k in OUTPUTS:
        want = exp[k] if with_ranks or k != "rank_by_slot" else np.full(text.n, D.FILL, dtype=np.uint32)
        bad = np.nonzero(got[k] != want)[0]
        assert bad.size == 0, (where, k, bad[:8].tolist(), got[k][bad[:8]].tolist(), want[bad[:8]].tolist())
    assert got["min_depth"] == exp["min_depth"], where
    return exp, got


@pytest.mark.parametrize("name", list(D.CASES))
def test_round_matches_the_model(native, name):
    branches, tied, runs, plain = set(), 0, 0, {}
    for order, flags in D.runs_of(name):
        exp, got = run_one(native, name, order, flags)
        if flags == 0:
            plain[order] = got
        if flags & D.TIMED:  # the timed instantiation: the same results as the untimed one, in every output
            assert got["new_m"] == plain[order]["new_m"] and got["min_depth"] == plain[order]["min_depth"]
            assert all(np.array_equal(got[k], plain[order][k]) for k in OUTPUTS), (name, order, "timed differs from untimed")
        branches |= D.branches_of(exp)
        tied += exp["new_m"]
        runs += 1
    text = D.made(name)[0]
    print(f"{name}: {runs} runs at {text.bits} bits, {text.terms.size} terminator entries; branches {sorted(branches)}; members left tied {tied}")


def test_timed_runs_cover_every_width():
    timed = [D.CASES[name].bits for name in D.CASES for _, flags in D.runs_of(name) if flags & D.TIMED]
    assert all(timed.count(bits) >= 2 for bits in (2, 4, 8))


def test_without_ranks_nothing_is_written_to_them(native):
    for name in ("sizes_h17", "tied_classes"):
        run_one(native, name, "shuffle", 0, with_ranks=False)


def test_a_call_leaves_no_state_behind(native):
    """one case three times, with a different case (another width, another cap, the other loop) in between"""
    first = run_one(native, "stragglers_32", "text", 0)[1]
    run_one(native, "busy_65_w8", "text", D.NO_STRAGGLERS)
    second = run_one(native, "stragglers_32", "text", 0)[1]
    run_one(native, "straggler_overflow_w4", "reversed", 0)
    third = run_one(native, "stragglers_32", "text", 0)[1]
    for other in (second, third):
        assert all(np.array_equal(first[k], other[k]) for k in OUTPUTS) and first["min_depth"] == other["min_depth"]


def test_bad_arguments_are_refused(native):
    text = b"ACGTACGTACGTACGTAACC"
    sa = np.arange(20, dtype=np.uint32)
    ok = dict(text=text, sa=sa, slot=[3, 4, 7, 8, 9], grp=[3, 3, 7, 7, 7], h0=0, cap=128)
    got = native.debug_direct_round(**ok)
    assert sorted(got["sa"][3:5]) == [3, 4] and sorted(got["sa"][7:10]) == [7, 8, 9] and got["new_m"] == 0
    assert got["sa"].tolist() == [0, 1, 2, 4, 3, 5, 6, 8, 9, 7] + list(range(10, 20))   # A.. < T..; A.. < C.. < T..
    many = native.debug_direct_round(text, sa, list(range(3, 12)), [3] * 9, 0, 128)   # a group of any size >= 2
    assert sorted(many["sa"][3:12]) == list(range(3, 12))
    bad_sa = sa.copy()
    bad_sa[8] = 20
    bad = [
        dict(ok, text=b"", sa=sa[:0], slot=[], grp=[]),               # no text
        dict(ok, slot=list(range(21)), grp=[0] * 21),                   # more list entries than suffixes
        dict(ok, sa=bad_sa),                                            # a listed slot that holds no suffix
        dict(ok, h0=12, cap=140),                                       # ... or one of fewer than h0 symbols (sa[9] + 12 > 20)
        dict(ok, slot=[3, 4, 7, 8, 9], grp=[3, 3, 8, 8, 8]),            # grp > slot
        dict(ok, slot=[3, 4, 18, 19, 20], grp=[3, 3, 18, 18, 18]),      # slot >= n
        dict(ok, slot=[7, 8, 9, 3, 4], grp=[7, 7, 7, 3, 3]),            # not in ascending slot order
        dict(ok, slot=[3, 4, 4, 8, 9], grp=[3, 3, 3, 8, 8]),            # a slot twice
        dict(ok, slot=[3, 5, 7, 8, 9], grp=[3, 3, 7, 7, 7]),            # a group with a hole in its slots
        dict(ok, slot=[4, 5, 7, 8, 9], grp=[3, 3, 7, 7, 7]),            # a group that does not start at its head slot
        dict(ok, slot=[3, 4, 7, 8, 9], grp=[3, 3, 7, 8, 8]),            # a listed group of one member
        dict(ok, slot=[3, 4, 7, 8, 12], grp=[3, 3, 7, 7, 12]),          # ... at the end of the list
        dict(ok, cap=0), dict(ok, h0=5, cap=5), dict(ok, h0=5, cap=4),  # cap <= h0
        dict(ok, cap=1025),                                             # more than 32 words of text
        dict(ok, flags=8),                                              # an unknown flag
        dict(ok, sa=sa[:19]), dict(ok, grp=[3, 3, 7, 7]), dict(ok, lcp_in=sa[:19]),   # lengths that do not fit
    ]
    for kw in bad:
        with pytest.raises(ValueError):
            native.debug_direct_round(**kw)
    assert native.debug_direct_round(**dict(ok, cap=1024))["new_m"] == 0   # 32 words at 2 bits
    wide = bytes(range(32, 72)) * 2   # 8 bits per symbol: 32 words are 256 symbols
    sa80 = np.arange(80, dtype=np.uint32)
    assert native.debug_direct_round(wide, sa80, [0, 1], [0, 0], 0, 256)["sa"][:2].tolist() == [0, 1]
    with pytest.raises(ValueError):
        native.debug_direct_round(wide, sa80, [0, 1], [0, 0], 0, 257)
    from nolzss_amd._lib import lib
    t = np.frombuffer(text, dtype=np.uint8)
    slot, grp = np.array(ok["slot"], dtype=np.uint32), np.array(ok["grp"], dtype=np.uint32)
    lcp_in, lcp, rank = np.zeros(20, dtype=np.uint32), np.zeros(20, dtype=np.uint32), np.zeros(20, dtype=np.uint32)
    new_slot, new_grp = np.zeros(5, dtype=np.uint32), np.zeros(5, dtype=np.uint32)
    new_m, depth = np.zeros(1, dtype=np.uint32), np.zeros(3, dtype=np.uint32)
    work = sa.copy()
    args = [t.ctypes.data, 20, work.ctypes.data, slot.ctypes.data, grp.ctypes.data, 5, 0, 128, 0, lcp_in.ctypes.data, 0, 0,
            lcp.ctypes.data, rank.ctypes.data, new_slot.ctypes.data, new_grp.ctypes.data, new_m.ctypes.data,
            depth.ctypes.data, None]
    assert lib.nolzss_debug_direct_round(*args) == 0
    for null_at in (0, 2, 3, 4, 9, 12, 13, 14, 15, 16, 17):
        a = list(args)
        a[null_at] = None
        assert lib.nolzss_debug_direct_round(*a) != 0, null_at
    a = list(args)
    a[1] = 0  # (refused before anything is read)
    assert lib.nolzss_debug_direct_round(*a) != 0
