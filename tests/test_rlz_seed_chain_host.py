"""CPU tests (no GPU) of the colinear seed chains of the relative-LZ index: the model the GPU tests compare with
(tests/rlz_seed_chain_model.py) against the definitions it rests on, what its generators are good for, the batch planner's
cut at 2^24 targets, the exports, and the refusals the library decides before any device work."""
import ctypes as C
import random

import numpy as np
import pytest

import rlz_locate_model as lm
import rlz_model as model
import rlz_seed_chain_model as cm
from nolzss_amd import _lib
from nolzss_amd import _noLZSS as native

PAIRS = [(1 << 33, 1 << 33), (1000, 50), (100, 10), (30, 0)]


def clouds():
    """200 seeded clouds, sizes around and beyond the look-back, each with one of the parameter pairs"""
    for seed in range(200):
        rng = random.Random(seed)
        yield cm.cloud(rng, rng.choice([1, 2, 40, 63, 64, 65, 70, 100, 129, 200, 300])), rng.choice(PAIRS)


# ---- the recurrence --------------------------------------------------------------------------------------------------
def test_the_look_back_equals_the_unbounded_recurrence_up_to_65_anchors():
    checked = 0
    for group, pair in clouds():
        if len(group) <= 65:
            assert cm.recurrence(group, *pair) == cm.recurrence(group, *pair, lookback=None)
            checked += 1
    for size in range(1, 66):  # every size once more
        group = cm.cloud(random.Random(9000 + size), size)
        assert cm.recurrence(group, 1000, 50) == cm.recurrence(group, 1000, 50, lookback=None)
    assert checked >= 50


def test_the_clouds_can_tell_the_rules_apart():
    """a prototype gave 17 and 113 of 200; what matters is that neither is 0"""
    lookback = ties = 0
    for group, pair in clouds():
        base = cm.recurrence(group, *pair)
        lookback += base != cm.recurrence(group, *pair, lookback=None)
        ties += base[1] != cm.recurrence(group, *pair, farthest=True)[1]
    assert lookback >= 1 and ties >= 1
    for group, _ in clouds():  # the generator keeps its promises
        assert group == sorted(group) and len({(y, q) for y, q, _ in group}) == len(group)
        assert all(1 <= L <= 30 for _, _, L in group)


# ---- every reported chain --------------------------------------------------------------------------------------------
def chains_of(res):
    for c in range(len(res["target"])):
        lo, hi = int(res["anchor_offsets"][c]), int(res["anchor_offsets"][c + 1])
        rec = {k: res[k][c].item() for k in cm.CHAIN_FIELDS}
        yield rec, [(int(res["anchor_t_start"][a]), int(res["anchor_position"][a]), int(res["anchor_length"][a]))
                    for a in range(lo, hi)]


def check_chains(refs, targets, res, max_gap, bandwidth, min_score):
    B, starts = cm.block_length(refs), lm.record_starts(refs)
    seen = set()
    for rec, anch in chains_of(res):
        key = (rec["target"], rec["is_rc"], rec["record"])
        assert key not in seen and (not seen or max(seen) < key)  # one per group, ascending
        seen.add(key)
        assert len(anch) == rec["num_anchors"] >= 1
        t, r = bytes(targets[rec["target"]]).upper(), bytes(refs[rec["record"]]).upper()
        ys = []
        for q, x, L in anch:  # every anchor is a genuine match inside its record
            piece = t[q:q + L]
            at = x - starts[rec["record"]]
            assert len(piece) == L and 0 <= at and at + L <= len(r)
            assert r[at:at + L] == (model.revcomp(piece) if rec["is_rc"] else piece)
            ys.append(2 * B - x - L + 1 if rec["is_rc"] else x)
        score = anch[0][2]
        for k in range(1, len(anch)):
            dq, dy = anch[k][0] - anch[k - 1][0], ys[k] - ys[k - 1]
            assert dq >= 1 and dy >= 1 and max(dq, dy) <= max_gap and abs(dq - dy) <= bandwidth
            score += min(anch[k][2], dq, dy) - abs(dq - dy)
        assert score == rec["score"] >= min_score
        assert (rec["t_start"], rec["t_end"]) == (anch[0][0], anch[-1][0] + anch[-1][2])
        assert (rec["r_start"], rec["r_end"]) == (min(x for _, x, _ in anch), max(x + L for _, x, L in anch))
    for t in {k[0] for k in seen}:  # one primary per target: the first of the largest score
        mine = [(rec["score"], rec["primary"]) for rec, _ in chains_of(res) if rec["target"] == t]
        assert sum(p for _, p in mine) == 1 and mine[[s for s, _ in mine].index(max(s for s, _ in mine))][1]


@pytest.mark.parametrize("seed", [1000, 1001, 1002])
def test_planted_targets_are_placed_where_they_were_cut(seed):
    refs, targets, truth = cm.planted(random.Random(seed))
    res = cm.expected(refs, targets, True, **cm.MAPPING)
    check_chains(refs, targets, res, cm.MAPPING["max_gap"], cm.MAPPING["bandwidth"], cm.MAPPING["min_score"])
    starts = lm.record_starts(refs)
    for j, (record, is_rc, lo, hi) in enumerate(truth):
        sel = np.flatnonzero((res["target"] == j) & res["primary"])
        assert len(sel) == 1
        c = sel[0]
        assert (res["record"][c], res["is_rc"][c]) == (record, bool(is_rc))
        assert starts[record] + lo <= res["r_start"][c] < res["r_end"][c] <= starts[record] + hi
        assert res["record_offset"][c] == res["r_start"][c] - starts[record]


def test_chains_of_the_ring_case_and_of_small_alphabets_are_sound():
    refs, target = cm.ring_case(random.Random(2000))
    for t in (target, model.revcomp(target)):
        check_chains(refs, [t], cm.expected(refs, [t], True, **cm.RING), cm.RING["max_gap"], cm.RING["bandwidth"],
                     cm.RING["min_score"])
    import rlz_seeds_model as sm
    for case in range(12):
        rng = random.Random(4100 + case)
        refs = lm.case(rng)
        targets = sm.targets(rng, refs, rng.randint(1, 6))
        for p in (dict(min_length=1, max_hits=0, max_gap=1 << 33, bandwidth=1 << 33, min_score=0),
                  dict(min_length=3, max_hits=4, max_gap=12, bandwidth=2, min_score=4)):
            check_chains(refs, targets, cm.expected(refs, targets, case % 3 != 0, **p), p["max_gap"], p["bandwidth"],
                         p["min_score"])


def test_the_extents_are_not_those_of_the_end_anchors():
    """diagonals that differ: the last anchor of a chain need not reach the furthest, on either strand"""
    group = [(100, 0, 30), (110, 12, 8)]  # (y, q, L): dq = 12, dy = 10, the link is worth min(8, 12, 10) - 2
    (c,) = cm.chains([(0, 0) + a for a in group], 1000, 1, 100, 50)["chains"]
    assert (c["num_anchors"], c["score"], c["r_start"], c["r_end"], c["t_end"]) == (2, 36, 100, 130, 20)
    (c,) = cm.chains([(0, 1) + a for a in group], 1000, 1, 100, 50)["chains"]  # group 1 of m = 1: the reverse strand
    assert (c["is_rc"], c["r_start"], c["r_end"]) == (1, 2001 - 100 - 30, 2001 - 100)
    assert c["r_start"] < 2001 - 110 - 8  # the last anchor starts further in


# ---- what needs no device --------------------------------------------------------------------------------------------
def test_the_planner_cuts_at_the_target_limit():
    from nolzss_amd.genomics import rlz
    assert rlz.MAX_CHAIN_TARGETS == 1 << 24
    assert rlz.plan_index_batches([0] * 10, 5, max_targets=4) == [(0, 4), (4, 8), (8, 10)]
    assert rlz.plan_index_batches([3, 3, 3, 3, 3], 5, batch_bases=6, max_targets=4) == [(0, 2), (2, 4), (4, 5)]
    assert rlz.plan_index_batches([1] * 5, 5, max_targets=5) == [(0, 5)] == rlz.plan_index_batches([1] * 5, 5)
    n = (1 << 24) + 3  # the real limit, on empty targets
    assert rlz.plan_index_batches(np.zeros(n, dtype=np.int64).tolist(), 5, max_targets=rlz.MAX_CHAIN_TARGETS) == \
        [(0, 1 << 24), (1 << 24, n)]


def test_symbols_layouts_and_exports():
    for name in ("nolzss_rlz_index_seed_chains", "nolzss_free_rlz_seed_chains_result", "nolzss_debug_rlz_seed_chain"):
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(_lib.lib, name)
    assert native.CHAIN_DTYPE.itemsize == 64 and native.CHAIN_ANCHOR_DTYPE.itemsize == 24
    assert native.CHAIN_DTYPE.names == ("target", "t_start", "t_end", "r_start", "r_end", "score", "record", "is_rc",
                                        "num_anchors", "primary")
    assert native.CHAIN_ANCHOR_DTYPE.names == ("t_start", "position", "length")
    assert C.sizeof(_lib.RlzChainParams) == 40 and C.sizeof(_lib.RlzSeedChainsResult) == 7 * C.sizeof(C.c_void_p)
    import noLZSS.genomics.rlz as shim
    from nolzss_amd.genomics import rlz
    for name in ("CHAIN_DTYPE", "CHAIN_ANCHOR_DTYPE"):
        assert name in rlz.__all__ and name in shim.__all__
        assert getattr(shim, name) is getattr(rlz, name) is getattr(native, name)


def test_refusals_before_any_device_work():
    lib, bad = _lib.lib, _lib.ERR_INVALID_ARGUMENT
    pt, ln = (C.c_char_p * 1)(b"ACGT"), (C.c_size_t * 1)(4)
    params, res = _lib.RlzChainParams(10, 8, 1000, 50, 20), _lib.RlzSeedChainsResult()
    assert lib.nolzss_rlz_index_seed_chains(None, pt, ln, 1, C.byref(params), None) == bad
    assert b"output pointer is null" in lib.nolzss_last_error()
    res.num_chains = 7
    assert lib.nolzss_rlz_index_seed_chains(None, pt, ln, 1, C.byref(params), C.byref(res)) == bad
    assert b"handle is null" in lib.nolzss_last_error() and res.num_chains == 0 and not res.anchor_offsets
    # the next two are decided before the handle is read: a block of zero bytes stands in for one
    stand_in = C.create_string_buffer(4096)
    assert lib.nolzss_rlz_index_seed_chains(stand_in, pt, ln, 1, None, C.byref(res)) == bad
    assert b"params is null" in lib.nolzss_last_error()
    k = (1 << 24) + 1  # empty targets: neither array is read
    ptrs, lens = np.zeros(k, dtype=np.uintp), np.zeros(k, dtype=np.uintp)
    assert lib.nolzss_rlz_index_seed_chains(stand_in, ptrs.ctypes.data_as(C.POINTER(C.c_char_p)),
                                            lens.ctypes.data_as(C.POINTER(C.c_size_t)), k, C.byref(params), C.byref(res)) == bad
    assert b"at most 2^24 targets" in lib.nolzss_last_error() and not res.chains and not res.anchor_offsets
    lib.nolzss_free_rlz_seed_chains_result(None)
    lib.nolzss_free_rlz_seed_chains_result(C.byref(res))
    assert res.num_chains == 0 and res.num_anchors == 0


def test_negative_and_oversized_arguments_raise_before_the_library_is_called():
    for name in ("min_length", "max_hits", "max_gap", "bandwidth", "min_score"):
        args = dict(min_length=1, max_hits=1, max_gap=1, bandwidth=1, min_score=1)
        with pytest.raises(ValueError, match=name):
            native._chain_params(**dict(args, **{name: -1}))
        with pytest.raises(ValueError, match=name):
            native._chain_params(**dict(args, **{name: 1 << 64}))
    p = native._chain_params(15, 64, 1 << 33, 500, 40)
    assert (p.min_length, p.max_hits, p.max_gap, p.bandwidth, p.min_score) == (15, 64, 1 << 33, 500, 40)


def test_the_debug_hook_refuses_bad_anchors_before_any_launch():
    good = [(0, 0, 5, 1, 3), (0, 0, 9, 4, 2), (0, 1, 2, 0, 1), (1, 0, 0, 0, 1)]

    def run(anch, B=1 << 20, m=2):
        cols = [np.array([a[k] for a in anch], dtype=np.uint32) for k in range(5)]
        return native.debug_rlz_seed_chain(*cols, B, m, 100, 10)

    for anch, text in (([good[1], good[0]], "do not ascend"), ([good[0], (0, 0, 5, 0, 3)], "do not ascend"),
                       ([good[0], good[0]], "twice"), ([good[2], good[0]], "do not ascend"),
                       ([(0, 0, 5, 1, 0)], "length of 0"), ([(0, 4, 5, 1, 1)], "group"), ([(1 << 24, 0, 5, 1, 1)], "target"),
                       ([(0, 0, 5, (1 << 31) - 1, 1)], "2\\^31"), ([(0, 2, (1 << 21) + 1, 0, 1)], "reverse-strand")):
        with pytest.raises(ValueError, match=text):
            run(anch)
    with pytest.raises(ValueError, match="records"):
        run(good, m=0)
    with pytest.raises(ValueError, match="records"):
        run(good, m=129)
