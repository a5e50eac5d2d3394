"""Left-normalised pileups, insertion alleles and the consensus of read batches on the relative-LZ index, on the device
(rlz_pileup.hip, rlz_consensus.hip, rlz_pileup_api.hip).  counts, insertions and consensus are compared with
tests/rlz_consensus_model.py over what RlzIndex.align returns, by integer and byte equality; the consensus of the
planted sample is the sample, and every read aligns to it without an edit."""
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import rlz_align_model as am
import rlz_consensus_model as km
import rlz_pileup_model as pm

pytestmark = pytest.mark.gpu

PLANTED_SEED = 7
SAMPLE_SEEDS = (3, 11)  # tests/test_rlz_consensus_host.py asserts the condition on these samples for the models alone
RULES = ((1, 0, 1), (2, 1, 2), (3, 9, 10))


@pytest.fixture(scope="module")
def rlz():
    from nolzss_amd import _noLZSS
    assert _noLZSS.device_count() >= 1, "no MI355X visible"
    from nolzss_amd.genomics import rlz
    return rlz


def model(refs, targets, aligned, primary_only, normalize):
    """-> (block, record starts, counters, allele table) of the model over an align result"""
    block = b"\x01".join(bytes(r).upper() for r in refs)
    counts, events = km.walk(block, pm.records(aligned), aligned["ops"], aligned["op_offsets"], targets, primary_only, normalize)
    return block, [int(s) for s in np.cumsum([0] + [len(r) + 1 for r in refs[:-1]])], counts, km.alleles(events)


def rows(found):
    return [tuple(int(v) for v in rec.tolist()[:8]) + (tuple(int(w) for w in rec["bases"]),) for rec in found]


def same_everything(pile, refs, targets, aligned, primary_only, normalize, rlz):
    """counts, insertions under three rules and the consensus in four settings against the model -> (counts, table)"""
    block, starts, counts, table = model(refs, targets, aligned, primary_only, normalize)
    got = pile.counts()
    assert got.dtype == np.uint32 and np.array_equal(got, counts), np.argwhere(got != counts)[:5].tolist()
    for rule in RULES:
        found = pile.insertions(rule[0], rule[1:])
        assert found.dtype == rlz.INSERTION_DTYPE and rows(found) == km.insertions(table, counts, starts, *rule), rule
    for min_depth, fraction, low in ((1, (1, 2), "reference"), (3, (2, 3), "N"), (1, (0, 1), "N"), (2, (1, 1), "reference")):
        exp = km.consensus(counts, table, block, min_depth, fraction[0], fraction[1], int(low == "N"))
        cons = pile.consensus(min_depth, fraction, low, return_map=True)
        assert cons["records"] == exp["records"] and cons["starts"].tolist() == exp["starts"], (min_depth, fraction, low)
        assert {name: cons[name] for name in km.STATS} == {name: exp[name] for name in km.STATS}
        assert "starts" not in pile.consensus(min_depth, fraction, low)
    return counts, table


@pytest.mark.parametrize("seed", SAMPLE_SEEDS)
def test_the_consensus_of_the_planted_sample_is_the_sample(rlz, seed):
    ref, reads, substitutions, sample = km.planted_sample_with_truth(random.Random(seed))
    with rlz.RlzIndex.build([ref]) as ix:
        aligned = ix.align(reads)
        with ix.pileup(normalize_indels=True) as pile, ix.pileup() as plain:
            info = pile.add(reads)
            assert plain.add(reads) == info  # (the four keys, and the flag changes none of them)
            counts, table = same_everything(pile, [ref], reads, aligned, True, True, rlz)
            cons = pile.consensus()
            assert cons["records"] == [sample]
            assert (cons["substitutions"], cons["deleted"], cons["insertions"], cons["inserted_bases"]) == (5, 3, 1, 2)
            summary = pile.info
            assert summary["normalize_indels"] is True and summary["insertion_events"] == int(counts[:, pm.INS].sum()) > 0
            assert summary["log_bytes"] >= 24 * summary["insertion_events"] and summary["device_bytes"] == plain.info["device_bytes"]
            # flags 0 beside it: the counters of the pileup as it was, the alleles of the un-normalised walk
            assert plain.info["normalize_indels"] is False
            old, old_table = same_everything(plain, [ref], reads, aligned, True, False, rlz)
            assert np.array_equal(old, pm.pileup(len(ref), pm.records(aligned), aligned["ops"], aligned["op_offsets"], reads, ref, True))
            every = plain.insertions(1, (0, 1))
            per_position = {}
            for rec in every:
                per_position[int(rec["position"])] = per_position.get(int(rec["position"]), 0) + int(rec["count"])
            assert per_position == {int(p): int(old[p, pm.INS]) for p in np.flatnonzero(old[:, pm.INS])}
            assert (every["ins_total"] == old[every["position"].astype(np.int64), pm.INS]).all()
            if seed == 3:
                assert plain.consensus()["records"] != [sample]  # why the flag exists
    with rlz.RlzIndex.build(cons["records"]) as polished:  # the loop closes: every read lies in the consensus, unedited
        again = polished.align(reads)
        best = again["primary"].astype(bool)
        assert sorted(again["target"][best].tolist()) == list(range(len(reads)))
        assert not again["edit_distance"][best].any() and ((again["t_end"] - again["t_start"])[best] == 100).all()


@pytest.fixture(scope="module")
def planted(rlz):
    refs, targets, _ = am.planted(random.Random(PLANTED_SEED))
    with rlz.RlzIndex.build(refs) as ix:
        yield ix, refs, targets, ix.align(targets)


@pytest.mark.parametrize("primary_only", (False, True))
def test_the_multi_record_set_equals_the_model(planted, rlz, primary_only):
    ix, refs, targets, aligned = planted
    for normalize in (True, False):
        with ix.pileup(primary_only=primary_only, normalize_indels=normalize) as pile:
            pile.add(targets)
            counts, table = same_everything(pile, refs, targets, aligned, primary_only, normalize, rlz)
            assert len(table) > 0 and len(pile.consensus()["records"]) == len(refs)


def test_chunked_downloads_change_nothing(planted, rlz, monkeypatch):
    ix, refs, targets, aligned = planted
    with ix.pileup(normalize_indels=True) as pile:
        pile.add(targets)
        whole = {rule: pile.insertions(rule[0], rule[1:]) for rule in RULES}
        cons = pile.consensus(return_map=True)
        assert len(whole[RULES[0]]) >= 8
        for chunk in ("1", "3", "7"):
            monkeypatch.setenv("NOLZSS_RLZ_LOCATE_CHUNK", chunk)  # the knob is read on every call
            for rule in RULES:
                assert np.array_equal(pile.insertions(rule[0], rule[1:]), whole[rule]), (chunk, rule)
            got = pile.consensus(return_map=True)  # the text and the map come down `chunk` entries at a time
            assert got["records"] == cons["records"] and np.array_equal(got["starts"], cons["starts"])
            assert {name: got[name] for name in km.STATS} == {name: cons[name] for name in km.STATS}
        monkeypatch.delenv("NOLZSS_RLZ_LOCATE_CHUNK")


CHILD = r'''
import random, sys
sys.path.insert(0, "tests")
import numpy as np
import rlz_align_model as am
from nolzss_amd.genomics import rlz
refs, targets, _ = am.planted(random.Random(7))
chunked = sys.argv[1] == "chunks"
with rlz.RlzIndex.build(refs) as ix, ix.pileup(normalize_indels=True) as halves, ix.pileup(normalize_indels=True) as once:
    assert halves.info["log_bytes"] == 0 and halves.info["insertion_events"] == 0
    half = len(targets) // 2
    halves.add(targets[:half])
    mid = halves.info
    halves.add(targets[half:], batch_bases=5000)
    once.add(targets)
    end, one = halves.info, once.info
    assert 0 < mid["insertion_events"] < end["insertion_events"] == one["insertion_events"]
    assert 24 * mid["insertion_events"] <= mid["log_bytes"] < end["log_bytes"] and end["log_bytes"] >= 24 * end["insertion_events"]
    assert np.array_equal(halves.counts(), once.counts())
    assert np.array_equal(halves.insertions(1, (0, 1)), once.insertions(1, (0, 1)))
    a, b = halves.consensus(return_map=True), once.consensus(return_map=True)
    assert a["records"] == b["records"] and np.array_equal(a["starts"], b["starts"])
    print("ok", end["insertion_events"], len(once.insertions(1, (0, 1))), mid["log_bytes"], end["log_bytes"])
'''


@pytest.mark.parametrize("knob", ("log", "chunks"))
def test_a_log_that_grows_from_one_event_in_a_child_process(rlz, knob):
    """NOLZSS_RLZ_PILEUP_LOG_EVENTS=1 for a whole process: the log grows with every batch that holds an insertion; adds in
    halves and in batches equal one add.  Once more with every download one entry at a time."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, NOLZSS_RLZ_PILEUP_LOG_EVENTS="1")
    if knob == "chunks":
        env["NOLZSS_RLZ_LOCATE_CHUNK"] = "3"
    r = subprocess.run([sys.executable, "-c", CHILD, knob], cwd=root, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("ok "), r.stdout[-2000:] + r.stderr[-4000:]
    events, alleles = (int(v) for v in r.stdout.split()[1:3])
    assert events >= alleles >= 8


def test_a_refused_add_leaves_counters_and_log_as_they_were(planted):
    ix, refs, targets, aligned = planted
    with ix.pileup(normalize_indels=True) as pile:
        pile.add(targets[:30])
        before, info = pile.counts(), pile.info
        alleles, cons = pile.insertions(1, (0, 1)), pile.consensus()
        assert info["insertion_events"] > 0
        with pytest.raises(RuntimeError, match="Invalid nucleotide 'N' found in sequence 4"):
            pile.add([targets[40], b"ACNT"])
        assert pile.info == info
        assert np.array_equal(pile.counts(), before) and np.array_equal(pile.insertions(1, (0, 1)), alleles)
        assert pile.consensus() == cons
        assert pile.add([b"", b""]) == dict(alignments=0, ops=0, columns=0, targets=32)
        assert pile.info["insertion_events"] == info["insertion_events"] and pile.info["log_bytes"] == info["log_bytes"]


def test_the_index_answers_align_as_before_beside_such_a_pileup_and_after_it(planted):
    ix, refs, targets, aligned = planted
    subset = targets[:25] + targets[-1:]
    before = ix.align(subset)
    pile = ix.pileup(normalize_indels=True)
    pile.add(subset)
    pile.insertions()
    pile.consensus(return_map=True)
    beside = ix.align(subset)
    pile.close()
    pile.close()
    after = ix.align(subset)
    for got in (beside, after):
        assert sorted(got) == sorted(before) and all(np.array_equal(got[k], before[k]) for k in before)
    for call in (pile.insertions, pile.consensus):
        with pytest.raises(ValueError, match="the pileup is closed"):
            call()
