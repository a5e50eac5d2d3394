"""The seed-chain stages from the group heads to the chain records, on the device and on arbitrary anchors
(rlz_seed_chain.hip: rlz_seed_chain_run, through nolzss_debug_rlz_seed_chain).  The anchor clouds of
tests/rlz_seed_chain_model.py -- most points near a few diagonals, the rest uniform -- reach what real seeds rarely do:
groups around the width of the ring (63 .. 129), candidates that tie, candidates just beyond the look-back.  f, pred,
the chain records, the offsets and the anchors are compared with the model by integer equality."""
import random

import numpy as np
import pytest

import rlz_seed_chain_model as cm

pytestmark = pytest.mark.gpu

B, M = 1 << 20, 2  # the block and its records: x = 2 B - y - L + 1 in the groups 2 and 3
PAIRS = [(1 << 33, 1 << 33), (1000, 50), (100, 10), (30, 0)]


@pytest.fixture(scope="module")
def native():
    from nolzss_amd import _noLZSS
    assert _noLZSS.device_count() >= 1, "no MI355X visible"
    return _noLZSS


def run(native, anch, max_gap, bandwidth, min_score=0):
    cols = [np.array([a[k] for a in anch], dtype=np.uint32) for k in range(5)]
    return native.debug_rlz_seed_chain(*cols, B, M, max_gap, bandwidth, min_score)


def same(got, anch, max_gap, bandwidth, min_score=0):
    exp = cm.chains(anch, B, M, max_gap, bandwidth, min_score)
    assert got["f"].tolist() == exp["f"]
    assert got["pred"].tolist() == exp["pred"]
    assert got["anchor_offsets"].tolist() == exp["anchor_offsets"]
    assert len(got["chains"]) == len(exp["chains"])
    for name in cm.CHAIN_FIELDS:
        assert got["chains"][name].tolist() == [r[name] for r in exp["chains"]], name
    triples = list(zip(got["anchors"]["t_start"].tolist(), got["anchors"]["position"].tolist(),
                       got["anchors"]["length"].tolist()))
    assert triples == exp["anchors"]
    return exp


@pytest.mark.parametrize("pair", PAIRS)
@pytest.mark.parametrize("size", [1, 2, 63, 64, 65, 127, 128, 129, 200, 300])
def test_one_size_of_group_on_both_strands(native, size, pair):
    rng = random.Random(size * 1000 + PAIRS.index(pair))
    anch = cm.cloud_anchors(rng, [size] * 4)  # a forward and a reverse group of each of two records
    exp = same(run(native, anch, *pair), anch, *pair)
    assert len(exp["chains"]) == 4


def test_the_cases_can_tell_the_rules_apart():
    """what the kernel can get wrong shows in these clouds: the look-back, and which of equal candidates wins"""
    lookback = ties = 0
    for size in (65, 127, 128, 129, 200, 300):
        for k, pair in enumerate(PAIRS):
            anch = cm.cloud_anchors(random.Random(size * 1000 + k), [size] * 4)
            base = cm.chains(anch, B, M, *pair)
            lookback += base["f"] != cm.chains(anch, B, M, *pair, lookback=None)["f"]
            ties += base["pred"] != cm.chains(anch, B, M, *pair, farthest=True)["pred"]
    assert lookback >= 1 and ties >= 1


def test_many_small_groups_among_large_ones(native):
    rng = random.Random(77)
    sizes = [rng.randint(1, 3) for _ in range(2000)]
    for at, size in ((0, 150), (1000, 257), (1999, 70)):  # the first and the last group are large ones
        sizes[at] = size
    anch = cm.cloud_anchors(rng, sizes)
    exp = same(run(native, anch, 1000, 50), anch, 1000, 50)
    assert len(exp["chains"]) == 2000
    exp = same(run(native, anch, 1000, 50, min_score=25), anch, 1000, 50, min_score=25)  # most groups are dropped
    assert 3 <= len(exp["chains"]) < 1500


def test_min_score_above_everything(native):
    anch = cm.cloud_anchors(random.Random(5), [40, 3])
    got = run(native, anch, 1000, 50, min_score=1 << 40)
    assert len(got["chains"]) == 0 and got["anchor_offsets"].tolist() == [0] and len(got["anchors"]) == 0
    assert got["f"].tolist() == cm.chains(anch, B, M, 1000, 50)["f"]
    got = run(native, [], 1000, 50)
    assert len(got["chains"]) == 0 and got["anchor_offsets"].tolist() == [0] and len(got["f"]) == 0


def test_refusals_before_launch(native):
    good = [(0, 0, 5, 1, 3), (0, 0, 9, 4, 2), (0, 1, 2, 0, 1), (1, 0, 0, 0, 1)]
    same(run(native, good, 100, 10), good, 100, 10)
    for bad in ([good[1], good[0]] + good[2:],                 # y descends inside a group
                [good[0], (0, 0, 5, 0, 3)] + good[2:],         # q descends at one y
                [good[0], good[0]] + good[2:],                 # (y, q) twice
                [good[2], good[0]],                            # the groups descend
                [good[3], good[0]],                            # the targets descend
                [(0, 0, 5, 1, 0)],                             # a length of 0
                [(0, 4, 5, 1, 1)],                             # a group beyond 2 m
                [(1 << 24, 0, 5, 1, 1)],                       # a target beyond 2^24
                [(0, 0, 5, (1 << 31) - 1, 1)],                 # q + length reaches 2^31
                [(0, 2, 2 * B + 1, 0, 1)]):                    # a reverse-strand anchor in front of the block
        with pytest.raises(ValueError):
            run(native, bad, 100, 10)
