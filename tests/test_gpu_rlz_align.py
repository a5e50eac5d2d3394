"""Base-level alignments of the seed chains on the relative-LZ index, on the device (rlz_align.hip,
rlz_index_seeds_api.hip).  RlzIndex.align is compared with tests/rlz_align_model.expected -- driven from the chains
RlzIndex.seed_chains returns at the same parameters -- by integer equality of every record, offset and op; replay
rebuilds every aligned stretch."""
import random

import numpy as np
import pytest

import rlz_align_model as am

pytestmark = pytest.mark.gpu

PLANTED_SEED = 7  # tests/test_rlz_align_host.py asserts the conditions on the planted reads for the model alone
CHAIN = {k: v for k, v in am.DEFAULTS.items() if k not in ("band", "max_flank")}
CHAIN_FIELDS = ("target", "record", "is_rc", "score", "primary")


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


def check_query(ix, refs, targets, **params):
    """align against the model driven from seed_chains at the same parameters; the invariants of every alignment"""
    params = dict(am.DEFAULTS, **params)
    chain = {k: params[k] for k in CHAIN}
    chains = ix.seed_chains(targets, **chain)
    got = ix.align(targets, **params)
    for key in CHAIN_FIELDS:
        assert np.array_equal(got[key], chains[key]), key
    same(got, am.expected(refs, targets, chains, params["band"], params["max_flank"]))
    block = b"\x01".join(bytes(r).upper() for r in refs)
    for c in range(len(got["target"])):
        ops = got["ops"][int(got["op_offsets"][c]):int(got["op_offsets"][c + 1])]
        n, code = ops >> 4, ops & 15
        t0, t1, r0, r1 = (int(got[k][c]) for k in ("t_start", "t_end", "r_start", "r_end"))
        assert t1 - t0 == int(n[(code == am.EQ) | (code == am.X) | (code == am.I)].sum())
        assert r1 - r0 == int(n[(code == am.EQ) | (code == am.X) | (code == am.D)].sum())
        assert int(got["edit_distance"][c]) == int(n[code != am.EQ].sum()) and int(got["columns"][c]) == int(n.sum())
        assert not (code[1:] == code[:-1]).any() and len(ops) == int(got["num_ops"][c]) >= 1
        target = bytes(targets[int(got["target"][c])]).upper()
        rebuilt, cost = am.replay(ops, target, block, t0, t1, r0, r1, bool(got["is_rc"][c]))
        assert rebuilt == target[t0:t1] and cost == int(got["edit_distance"][c])
    return got, chains


@pytest.fixture(scope="module")
def planted(rlz):
    refs, targets, truth = am.planted(random.Random(PLANTED_SEED))
    with rlz.RlzIndex.build(refs) as ix:
        got, chains = check_query(ix, refs, targets)
        yield ix, refs, targets, truth, got, chains


def test_reads_and_contigs_align_as_the_model_does(planted):
    ix, refs, targets, truth, got, chains = planted
    assert len(got["target"]) >= len(targets) and got["is_rc"].any() and not got["is_rc"].all()
    code = got["ops"] & 15
    assert all((code == c).any() for c in (am.I, am.D, am.EQ, am.X))
    assert ((got["ops"] >> 4)[(code == am.I) | (code == am.D)] == 20).any()  # the contigs' indel of 20 bases


def test_every_planted_read_is_recovered_end_to_end(planted):
    """a condition, not a measurement: the seed is chosen so that the model alone meets it (the host test asserts that)"""
    ix, refs, targets, truth, got, chains = planted
    assert am.DEFAULTS["max_flank"] >= 150
    for j, (record, is_rc, edits) in enumerate(truth):
        sel = np.flatnonzero((got["target"] == j) & got["primary"])
        assert len(sel) == 1, j
        c = sel[0]
        assert (int(got["record"][c]), bool(got["is_rc"][c])) == (record, is_rc), j
        assert int(got["t_start"][c]) == 0 and int(got["t_end"][c]) == len(targets[j]), j
        assert int(got["edit_distance"][c]) <= edits, j


def test_chunks_and_batches_change_nothing(planted, rlz, monkeypatch):
    ix, refs, targets, truth, got, chains = planted
    subset = targets[:40] + targets[-2:]
    exp = ix.align(subset)
    assert len(exp["ops"]) >= 100
    for chunk in ("1", "3", "7"):
        monkeypatch.setenv("NOLZSS_RLZ_LOCATE_CHUNK", chunk)  # the knob is read on every call
        same(ix.align(subset), exp)
    monkeypatch.delenv("NOLZSS_RLZ_LOCATE_CHUNK")
    same(ix.align(subset, batch_bases=700), exp)
    monkeypatch.setattr(rlz, "MAX_CHAIN_TARGETS", 5)  # the cut at 2^24 targets, brought within reach
    same(ix.align(subset), exp)


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


def test_the_batch_is_searched_again_when_the_arena_grows_for_the_hits_and_for_the_jobs(planted):
    """with the arena empty, the first call reserves for the batch, learns the number of hits, reserves again -- the slab
    is replaced -- and searches the batch a second time; it chains and plans, learns the DP rows and column slots,
    reserves a third time and searches, chains and plans once more before the one DP; the next call finds room"""
    from nolzss_amd import _noLZSS as native
    ix, refs, targets, truth, got, chains = planted  # (the fixture compared got with the model)
    front, back = ("rlz_index_search", "rlz_seed_flags", "rlz_seed_intervals"), ("rlz_seed_hits", "rlz_chain_recurrence")
    plan, dp = ("rlz_align_plan", "rlz_align_sizes"), ("rlz_align_dp",)
    native.debug_trim_arenas()
    first, report = _profiled(lambda: ix.align(targets))
    assert report["rlz_index_search"][0] >= 2  # (at least one regrow: else this test is not on the path)
    assert _launches(report, *front) == [3, 3, 3] and _launches(report, *back) == [2, 2]
    assert _launches(report, *plan) == [2, 2] and _launches(report, *dp) == [1]
    again, report = _profiled(lambda: ix.align(targets))
    assert _launches(report, *front) == [1, 1, 1] and _launches(report, *back) == [1, 1]
    assert _launches(report, *plan) == [1, 1] and _launches(report, *dp) == [1]
    same(first, got)
    same(again, got)


def test_max_flank_zero_clips_every_flank(planted):
    ix, refs, targets, truth, got, chains = planted
    subset = targets[:30] + targets[-1:]
    clipped, chains = check_query(ix, refs, subset, max_flank=0)
    assert np.array_equal(clipped["t_start"], chains["t_start"]) and np.array_equal(clipped["t_end"], chains["t_end"])
    assert (clipped["t_end"] - clipped["t_start"] < 150).any()
    # and a flank one base longer than max_flank is clipped while the others are kept
    check_query(ix, refs, subset, max_flank=20)


def test_a_read_hanging_over_a_records_end_is_clipped_there(planted):
    ix, refs, targets, truth, got, chains = planted
    rng = random.Random(5)
    starts = np.cumsum([0] + [len(r) + 1 for r in refs[:-1]])
    over_end = refs[1][-100:] + am.random_dna(rng, 30)
    over_start = am.random_dna(rng, 30) + refs[2][:100]
    near_end = refs[0][-100:-10] + am.random_dna(rng, 12)  # ten bases of room for twelve: inside the band, aligned
    got, _ = check_query(ix, refs, [over_end, am.revcomp(over_end), over_start, near_end])
    p = {int(t): c for c, t in enumerate(got["target"]) if got["primary"][c]}
    assert (int(got["t_start"][p[0]]), int(got["t_end"][p[0]])) == (0, 100)
    assert int(got["r_end"][p[0]]) == starts[1] + len(refs[1]) and int(got["record"][p[0]]) == 1
    assert bool(got["is_rc"][p[1]]) and (int(got["t_start"][p[1]]), int(got["t_end"][p[1]])) == (30, 130)
    assert int(got["r_end"][p[1]]) == starts[1] + len(refs[1])
    assert (int(got["t_start"][p[2]]), int(got["t_end"][p[2]])) == (30, 130) and int(got["r_start"][p[2]]) == starts[2]
    assert (int(got["t_start"][p[3]]), int(got["t_end"][p[3]])) == (0, 102) and int(got["r_end"][p[3]]) <= len(refs[0])


def test_an_index_without_reverse_complement_aligns_forward_only(rlz):
    refs, targets, truth = am.planted(random.Random(PLANTED_SEED), reads=24, contigs=1)
    with rlz.RlzIndex.build(refs, with_rc=False) as ix:
        got, _ = check_query(ix, refs, targets)
        assert len(got["target"]) >= 8 and not got["is_rc"].any()
        for j, (record, is_rc, edits) in enumerate(truth):
            if not is_rc:
                sel = np.flatnonzero((got["target"] == j) & got["primary"])
                assert len(sel) == 1 and int(got["record"][sel[0]]) == record


def test_small_alphabets_and_other_bands(rlz):
    """many chains per target, overlapping anchors (the trim), gaps without a base on one side, and the widest job"""
    rng = random.Random(77)
    refs = [bytes(rng.choice(b"AC") for _ in range(300)), bytes(rng.choice(b"ACG") for _ in range(260))]
    targets = []
    for _ in range(12):
        r = rng.choice(refs)
        lo = rng.randrange(0, len(r) - 120)
        piece, _ = am.mutate(rng, r[lo:lo + 120], 3)
        targets.append(piece if rng.random() < 0.5 else am.revcomp(piece))
    targets += [b"", b"ACGT", refs[0].lower()]
    with rlz.RlzIndex.build(refs) as ix:
        total = 0
        for params in (dict(min_length=6, max_hits=0, max_gap=60, bandwidth=31, min_score=10, band=16, max_flank=64),
                       dict(min_length=4, max_hits=8, max_gap=30, bandwidth=3, min_score=8, band=30, max_flank=10),
                       dict(min_length=8, max_hits=0, max_gap=200, bandwidth=63, min_score=12, band=0, max_flank=300)):
            total += len(check_query(ix, refs, targets, **params)[0]["target"])
        assert total >= 30
        for none in ([], [b"", b""]):
            got = ix.align(none)
            assert got["op_offsets"].tolist() == [0] and len(got["target"]) == 0 and got["primary"].dtype == bool
            assert got["ops"].dtype == np.uint32 and got["num_ops"].dtype == np.uint32
        with pytest.raises(ValueError, match="64 diagonals"):
            ix.align(targets, bandwidth=32, band=16)
        with pytest.raises(RuntimeError, match="Invalid nucleotide 'N' found in sequence 3"):
            ix.align([b"ACG", b"ACNT"])
        check_query(ix, refs, targets[:3])  # (the handle is still good)
