"""Colinear seed chains on the relative-LZ index, on the device (rlz_seed_chain.hip, rlz_index_seeds_api.hip).  Every
case compares RlzIndex.seed_chains with tests/rlz_seed_chain_model.expected -- the seeds of rlz_seeds_model, the
recurrence in plain Python integers -- by integer equality of every field of every chain and anchor."""
import random
import threading

import numpy as np
import pytest

import rlz_locate_model as lm
import rlz_model as model
import rlz_seed_chain_model as cm
import rlz_seeds_model as sm

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rlz():
    from nolzss_amd import _noLZSS
    assert _noLZSS.device_count() >= 1, "no MI355X visible"
    from nolzss_amd.genomics import rlz
    return rlz


def same(got, exp):
    assert sorted(got) == sorted(exp)
    for key, e in exp.items():
        assert got[key].dtype == e.dtype, key
        if not np.array_equal(got[key], e):
            raise AssertionError(f"{key} differs: {len(got[key])} entries {got[key][:16]} != {len(e)} entries {e[:16]}")


def check_query(ix, refs, targets, with_rc, **params):
    got = ix.seed_chains(targets, **params)
    same(got, cm.expected(refs, targets, with_rc, **params))
    return got


def primary(got, target=0):
    sel = np.flatnonzero((got["target"] == target) & got["primary"])
    assert len(sel) == 1
    return {k: got[k][sel[0]].item() for k in cm.CHAIN_FIELDS}


def other(*bases):
    return bytes([next(c for c in b"ACGT" if c not in bases)])


# ---- 1. hand cases ---------------------------------------------------------------------------------------------------
R1 = b"ACGGTCATTGCAAGCTTAGGCATCGA"
R2 = b"TTGACCGGTAAGGCCTTTAGACCA"
HAND = dict(min_length=5, max_hits=0, max_gap=100, bandwidth=10, min_score=0)


@pytest.mark.parametrize("with_rc", [True, False])
def test_hand_cases(rlz, with_rc):
    refs = [R1, R2]
    with rlz.RlzIndex.build(refs, with_rc=with_rc) as ix:
        got = check_query(ix, refs, [R1], with_rc, **HAND)  # a whole record: one chain of one anchor
        assert len(got["target"]) == 1 and got["anchor_offsets"].tolist() == [0, 1]
        assert primary(got) == dict(target=0, record=0, is_rc=False, score=len(R1), t_start=0, t_end=len(R1), r_start=0,
                                    r_end=len(R1), num_anchors=1, primary=True)
        got = check_query(ix, refs, [model.revcomp(R2)], with_rc, **HAND)
        if with_rc:
            assert primary(got) == dict(target=0, record=1, is_rc=True, score=len(R2), t_start=0, t_end=len(R2),
                                        r_start=len(R1) + 1, r_end=len(R1) + 1 + len(R2), num_anchors=1, primary=True)
            assert got["record_offset"][got["primary"]].tolist() == [0]
        else:
            assert int(got["score"].max(initial=0)) < len(R2)
        # one substitution: two anchors on one diagonal, the second one worth all its 13 bases
        got = check_query(ix, refs, [R1[:12] + other(R1[12]) + R1[13:]], with_rc, **HAND)
        p = primary(got)
        assert (p["num_anchors"], p["score"], p["t_start"], p["t_end"], p["r_start"], p["r_end"]) == (2, 12 + 13, 0, 26, 0, 26)
        # one inserted base: dq = 13, dy = 12: the second anchor is worth min(14, 13, 12) - 1
        inserted = R1[:12] + other(R1[11], R1[12]) + R1[12:]
        got = check_query(ix, refs, [inserted], with_rc, **HAND)
        p = primary(got)
        assert (p["num_anchors"], p["score"], p["t_end"], p["r_end"]) == (2, 12 + 12 - 1, 27, 26)
        # bandwidth 0 splits it: the better half is reported
        got = check_query(ix, refs, [inserted], with_rc, **dict(HAND, bandwidth=0))
        p = primary(got)
        assert (p["num_anchors"], p["score"], p["t_start"], p["r_start"]) == (1, 14, 13, 12)
        # pieces of two records: two chains, the longer one primary
        got = check_query(ix, refs, [R1[2:20] + R2[3:15]], with_rc, **HAND)
        assert got["record"].tolist() == [0, 1] and got["primary"].tolist() == [True, False]
        assert got["score"].tolist()[0] >= 18 > got["score"].tolist()[1] >= 12
        # min_score above everything
        got = check_query(ix, refs, [R1, R2[3:15]], with_rc, **dict(HAND, min_score=1000))
        assert len(got["target"]) == 0 and got["anchor_offsets"].tolist() == [0] and len(got["anchor_length"]) == 0
        # empty targets between others; lower case; no target
        got = check_query(ix, refs, [R1[:9], b"", R2[3:11].lower(), b"", b"", R1[-8:]], with_rc, **HAND)
        assert got["target"].tolist() == [0, 2, 5] and got["primary"].all()
        same(ix.seed_chains([R1.lower()], **HAND), cm.expected(refs, [R1], with_rc, **HAND))
        for none in ([], [b"", b""]):
            got = ix.seed_chains(none)
            assert got["anchor_offsets"].tolist() == [0] and len(got["target"]) == 0 and got["primary"].dtype == bool


# ---- 2. seeded end to end --------------------------------------------------------------------------------------------
SETS = [dict(min_length=1, max_hits=0, max_gap=1 << 33, bandwidth=1 << 33, min_score=0),
        dict(min_length=3, max_hits=4, max_gap=12, bandwidth=2, min_score=4),
        dict(min_length=2, max_hits=0, max_gap=40, bandwidth=0, min_score=1)]


@pytest.mark.parametrize("part", range(4))
def test_seeded_cases(rlz, part):
    """small alphabets: many hits per seed, interleaved groups"""
    chains = 0
    for case in range(10 * part, 10 * part + 10):
        rng = random.Random(4100 + case)
        refs = lm.case(rng)
        targets = sm.targets(rng, refs, rng.randint(1, 6))
        with_rc = case % 3 != 0
        with rlz.RlzIndex.build(refs, with_rc=with_rc) as ix:
            for params in SETS:
                chains += len(check_query(ix, refs, targets, with_rc, **params)["target"])
    assert chains >= 30


def test_planted_targets_with_the_mapping_parameters(rlz):
    refs, targets, truth = cm.planted(random.Random(1000))
    starts = lm.record_starts(refs)
    with rlz.RlzIndex.build(refs) as ix:
        got = check_query(ix, refs, targets, True, **cm.MAPPING)
    for j, (record, is_rc, lo, hi) in enumerate(truth):
        p = primary(got, j)
        assert (p["record"], p["is_rc"]) == (record, bool(is_rc))
        assert starts[record] + lo <= p["r_start"] < p["r_end"] <= starts[record] + hi


# ---- 3. groups longer than the ring ----------------------------------------------------------------------------------
@pytest.mark.parametrize("reverse", [False, True])
def test_a_group_wraps_the_ring_twice(rlz, reverse):
    refs, target = cm.ring_case(random.Random(2000))
    if reverse:
        target = model.revcomp(target)
    anch = cm.anchors(refs, [target], True, cm.RING["min_length"], cm.RING["max_hits"])
    assert max(end - first for _, first, end in cm.groups_of(anch)) > 128
    with rlz.RlzIndex.build(refs) as ix:
        got = check_query(ix, refs, [target], True, **cm.RING)
    p = primary(got)
    assert (p["record"], p["is_rc"]) == (0, reverse) and p["num_anchors"] > 20


# ---- 4. transport: chunks, batches, threads --------------------------------------------------------------------------
def test_chunks_and_batches_change_nothing(rlz, monkeypatch):
    refs, targets, _ = cm.planted(random.Random(1001), count=9)
    targets.insert(4, b"")
    exp = cm.expected(refs, targets, True, **cm.MAPPING)
    assert len(exp["target"]) >= 9 and len(exp["anchor_length"]) >= 40
    with rlz.RlzIndex.build(refs) as ix:
        same(ix.seed_chains(targets, **cm.MAPPING), exp)
        monkeypatch.setenv("NOLZSS_RLZ_LOCATE_CHUNK", "3")  # the knob is read on every call
        same(ix.seed_chains(targets, **cm.MAPPING), exp)
        monkeypatch.delenv("NOLZSS_RLZ_LOCATE_CHUNK")
        same(ix.seed_chains(targets, batch_bases=500, **cm.MAPPING), exp)
        monkeypatch.setattr(rlz, "MAX_CHAIN_TARGETS", 2)  # the cut at 2^24 targets, brought within reach
        same(ix.seed_chains(targets, **cm.MAPPING), exp)


def _profiled(fn):
    from nolzss_amd import _noLZSS as native
    native.profile_enable(True)
    try:
        native.profile_reset()
        out = fn()
        return out, native.profile_report()
    finally:
        native.profile_enable(False)
        native.profile_reset()


def _launches(report, *names):
    return [report[name][0] if name in report else 0 for name in names]


def test_the_batch_is_searched_again_when_the_arena_grows_for_the_hits(rlz):
    """an open leaves the arena empty: the first query reserves for the batch, learns the number of hits, reserves again
    -- the slab is replaced -- and searches the batch a second time in it, before the hits are expanded and chained once;
    the next call finds room"""
    from nolzss_amd import _noLZSS as native
    refs, targets, _ = cm.planted(random.Random(1001), count=9)
    targets.insert(4, b"")
    exp = cm.expected(refs, targets, True, **cm.MAPPING)
    front, back = ("rlz_index_search", "rlz_seed_flags", "rlz_seed_intervals"), ("rlz_seed_hits", "rlz_chain_recurrence")
    with rlz.RlzIndex.build(refs) as ix:
        native.debug_trim_arenas()
        first, report = _profiled(lambda: ix.seed_chains(targets, **cm.MAPPING))
        assert report["rlz_index_search"][0] >= 2  # (at least one regrow: else this test is not on the path)
        assert _launches(report, *front) == [2, 2, 2] and _launches(report, *back) == [1, 1]
        again, report = _profiled(lambda: ix.seed_chains(targets, **cm.MAPPING))
        assert _launches(report, *front) == [1, 1, 1] and _launches(report, *back) == [1, 1]
        same(first, exp)
        same(again, exp)


def test_two_threads_query_one_handle(rlz):
    refs, targets, _ = cm.planted(random.Random(1002), count=12)
    batches = [targets[:6], targets[6:]]
    exp = [cm.expected(refs, b, True, **cm.MAPPING) for b in batches]
    out, errors = [[None] * 4, [None] * 4], []
    with rlz.RlzIndex.build(refs) as ix:
        def work(t):
            try:
                for rep in range(4):
                    out[t][rep] = ix.seed_chains(batches[t], **cm.MAPPING)
            except Exception as e:  # noqa: BLE001
                errors.append(e)

        threads = [threading.Thread(target=work, args=(t,)) for t in range(2)]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
    assert not errors, errors
    for t in range(2):
        for got in out[t]:
            same(got, exp[t])


def test_negative_arguments(rlz):
    with rlz.RlzIndex.build([R1]) as ix:
        for name in ("min_length", "max_hits", "max_gap", "bandwidth", "min_score"):
            with pytest.raises(ValueError, match=name):
                ix.seed_chains([R1], **{name: -1})


def test_what_a_seed_query_refuses_is_refused_alike(rlz):
    with rlz.RlzIndex.build([R1, R2]) as ix:
        with pytest.raises(RuntimeError, match="Invalid nucleotide 'N' found in sequence 4"):
            ix.seed_chains([b"ACG", b"", b"ACNT"])
        same(ix.seed_chains([R1], **HAND), cm.expected([R1, R2], [R1], True, **HAND))  # (the handle is still good)
    with pytest.raises(ValueError, match="closed"):
        ix.seed_chains([R1])


def test_a_hit_total_beyond_the_pipeline_leaves_an_empty_result_and_the_status(rlz):
    """the total is summed on the device in 64 bits: this one is beyond 2^32"""
    import ctypes as C

    from nolzss_amd import _lib
    from nolzss_amd import _noLZSS as native
    ref = np.frombuffer(b"ACGT", dtype=np.uint8)[np.random.default_rng(41).integers(0, 4, 1 << 16)].tobytes()
    per = len(lm.brute_locate([ref], b"A", True))
    q = (1 << 32) // per + 2
    assert q < 200_000 and q * per > 1 << 32 > rlz.MAX_TEXT
    loose = dict(min_length=1, max_hits=0, max_gap=10, bandwidth=10, min_score=0)
    with rlz.RlzIndex.build(ref) as ix:
        with pytest.raises(ValueError, match=rf"seeds would report {q * per} hits.*max_hits.*min_length"):
            ix.seed_chains([b"A"] * q, **loose)
        res, params = _lib.RlzSeedChainsResult(), native._chain_params(1, 0, 10, 10, 0)
        rc = _lib.lib.nolzss_rlz_index_seed_chains(ix._live()._handle(), *native._seq_args([b"A"] * q, "target"),
                                                   C.byref(params), C.byref(res))
        assert rc == _lib.ERR_INVALID_ARGUMENT and res.num_chains == 0 and not res.chains and not res.anchor_offsets
        _lib.lib.nolzss_free_rlz_seed_chains_result(C.byref(res))
        got = ix.seed_chains([b"A"] * q, **dict(loose, max_hits=per - 1))  # every seed capped: no anchor at all
        assert len(got["target"]) == 0 and got["anchor_offsets"].tolist() == [0]
        got = ix.seed_chains([b"A"] * 3, **loose)  # every group holds anchors of one q: chains of one anchor
        assert got["target"].tolist() == [0, 0, 1, 1, 2, 2] and got["score"].tolist() == [1] * 6
        assert got["primary"].tolist() == [True, False] * 3
