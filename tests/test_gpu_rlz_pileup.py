"""Pileup counts and variant sites of read batches on the relative-LZ index, on the device (rlz_pileup.hip,
rlz_pileup_api.hip).  RlzPileup.counts is compared with tests/rlz_pileup_model.pileup -- over the all-CPU expectation
(seed-chain model, then rlz_align_model.expected) and over what RlzIndex.align returns -- by integer equality of every
counter, RlzPileup.variants with the model's variants over the same counters."""
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import rlz_align_model as am
import rlz_pileup_model as pm
import rlz_seed_chain_model as cm

pytestmark = pytest.mark.gpu

PLANTED_SEED = 7  # the set of tests/test_gpu_rlz_align.py
SAMPLE_SEED = 3   # tests/test_rlz_pileup_host.py asserts the condition on the sample for the model alone
RULES = ((1, 0, 1), (2, 1, 2), (3, 9, 10))


@pytest.fixture(scope="module")
def rlz():
    from nolzss_amd import _noLZSS
    assert _noLZSS.device_count() >= 1, "no MI355X visible"
    from nolzss_amd.genomics import rlz
    return rlz


def model_counts(refs, targets, aligned, primary_only):
    block = b"\x01".join(bytes(r).upper() for r in refs)
    return pm.pileup(len(block), pm.records(aligned), aligned["ops"], aligned["op_offsets"], targets, block, primary_only)


def same_counts(got, exp):
    assert got.shape == exp.shape and got.dtype == np.uint32
    if not np.array_equal(got, exp):
        p, ch = np.argwhere(got != exp)[0]
        raise AssertionError(f"position {p} channel {pm.CHANNELS[ch]}: {got[p].tolist()} != {exp[p].tolist()} "
                             f"({int((got != exp).sum())} counters differ)")


def same_variants(got, counts, refs, rule, rlz):
    block = b"\x01".join(bytes(r).upper() for r in refs)
    starts = np.cumsum([0] + [len(r) + 1 for r in refs[:-1]])
    exp = pm.variants(counts, block, starts, *rule)
    assert got.dtype == rlz.VARIANT_DTYPE and got.dtype.names == pm.VARIANT_FIELDS
    assert [tuple(int(v) for v in row) for row in got.tolist()] == exp, rule
    return exp


@pytest.fixture(scope="module")
def planted(rlz):
    """the index, the set, the all-CPU expectation of its alignments and the model's counters for both settings"""
    refs, targets, _ = am.planted(random.Random(PLANTED_SEED))
    params = dict(am.DEFAULTS)
    band, max_flank = params.pop("band"), params.pop("max_flank")
    cpu = am.expected(refs, targets, cm.expected(refs, targets, True, **params), band, max_flank)
    exp = {flag: model_counts(refs, targets, cpu, flag) for flag in (False, True)}
    with rlz.RlzIndex.build(refs) as ix:
        yield ix, refs, targets, exp


def test_counts_equal_the_model_over_the_cpu_expectation_and_over_align(planted):
    ix, refs, targets, exp = planted
    aligned = ix.align(targets)
    for flag in (False, True):
        with ix.pileup(primary_only=flag) as pile:
            info = pile.add(targets)
            got = pile.counts()
            same_counts(got, exp[flag])
            same_counts(got, model_counts(refs, targets, aligned, flag))
            kept = aligned["primary"] | (not flag)
            assert info == dict(alignments=int(kept.sum()), ops=int(aligned["num_ops"][kept].sum()),
                                columns=int(aligned["columns"][kept].sum()), targets=len(targets))
            summary = pile.info
            assert summary["block_length"] == len(got) and summary["targets"] == len(targets) and summary["adds"] == 1
            assert summary["device_bytes"] >= 44 * len(got) and summary["primary_only"] == flag and summary["dirty"] == 0
            assert summary["band"] == 16 and summary["bandwidth"] == 31
    assert got[:, pm.REV].any() and got[:, pm.DEL].any() and got[:, pm.INS].any()
    assert not got[[len(refs[0]), len(refs[0]) + 1 + len(refs[1])]].any()  # the separators


def test_alignments_that_are_not_primary_count_only_when_asked(rlz):
    """a record repeated inside the block: every read has a second placement, which primary_only skips; two reads hang
    over a record's end and are clipped there (BREAK)"""
    rng = random.Random(23)
    core = am.random_dna(rng, 400)
    refs = [am.random_dna(rng, 100) + core + am.random_dna(rng, 80), am.random_dna(rng, 60) + core[:350] + am.random_dna(rng, 90)]
    targets = []
    for j in range(40):
        lo = rng.randrange(0, 250)
        piece, _ = am.mutate(rng, core[lo:lo + 100], rng.randrange(0, 3))
        targets.append(am.revcomp(piece) if j % 2 else piece)
    over_end = refs[0][-100:] + am.random_dna(rng, 30)
    targets += [over_end, am.revcomp(over_end)]
    with rlz.RlzIndex.build(refs) as ix:
        aligned = ix.align(targets)
        assert aligned["primary"].any() and not aligned["primary"].all()
        assert (aligned["t_end"] - aligned["t_start"] == 100)[-2:].all()
        counts = {}
        for flag in (False, True):
            with ix.pileup(primary_only=flag) as pile:
                pile.add(targets)
                counts[flag] = pile.counts()
                same_counts(counts[flag], model_counts(refs, targets, aligned, flag))
        assert counts[True].sum() < counts[False].sum()
        end = len(refs[0]) - 1  # both clipped reads end at the record's last base, in block orientation
        assert counts[True][end, pm.BREAK] == 2 and counts[True][:, pm.BREAK].sum() == 2


def test_adds_in_halves_ranges_and_chunks_change_nothing(planted, monkeypatch):
    ix, refs, targets, exp = planted
    B, half = len(exp[True]), len(targets) // 2
    with ix.pileup() as pile:
        first = pile.add(targets[:half])
        assert pile.info["dirty"] == 1
        second = pile.add(targets[half:], batch_bases=5000)  # (several batches inside one add)
        assert first["targets"] == half and second["targets"] == len(targets) and pile.info["adds"] >= 3
        whole = pile.counts()
        same_counts(whole, exp[True])
        assert pile.info["dirty"] == 0
        r0, r1 = len(refs[0]), len(refs[0]) + 1 + len(refs[1])
        ranges = ((0, 0), (17, 18), (1500, r0 + 200), (r0 - 3, r0 + 4), (r0 + 1, r1), (r1 + 700, B), (0, B))
        for lo, hi in ranges:
            same_counts(pile.counts(lo, hi), whole[lo:hi])
        found = {rule: pile.variants(rule[0], rule[1:]) for rule in RULES}
        assert len(found[RULES[0]]) > len(found[RULES[1]]) >= len(found[RULES[2]]) and len(found[RULES[0]]) >= 100
        for chunk in ("1", "3", "7"):
            monkeypatch.setenv("NOLZSS_RLZ_LOCATE_CHUNK", chunk)  # the knob is read on every call
            for lo, hi in ranges[:4] + ((r1 + 700, r1 + 760),):
                same_counts(pile.counts(lo, hi), whole[lo:hi])
            for rule in RULES[1:] if chunk == "1" else RULES:
                assert np.array_equal(pile.variants(rule[0], rule[1:]), found[rule]), (chunk, rule)
        monkeypatch.delenv("NOLZSS_RLZ_LOCATE_CHUNK")
        with pytest.raises(ValueError, match="block length"):
            pile.counts(0, B + 1)
        with pytest.raises(ValueError, match="start <= end"):
            pile.counts(5, 4)


CHILD = r'''
import random, sys
sys.path.insert(0, "tests")
import numpy as np
import rlz_align_model as am, rlz_pileup_model as pm
from nolzss_amd.genomics import rlz
refs, targets, _ = am.planted(random.Random(7), reads=24, contigs=1)
block = b"\x01".join(refs)
starts = np.cumsum([0] + [len(r) + 1 for r in refs[:-1]])
with rlz.RlzIndex.build(refs) as ix, ix.pileup() as halves, ix.pileup() as once:
    aligned = ix.align(targets)
    exp = pm.pileup(len(block), pm.records(aligned), aligned["ops"], aligned["op_offsets"], targets, block, True)
    halves.add(targets[:12])
    halves.add(targets[12:])
    once.add(targets)
    for pile in (halves, once):
        whole = pile.counts()
        assert np.array_equal(whole, exp)
        for lo, hi in ((0, 0), (1500, 1501), (2990, 3040), (len(block) - 5, len(block))):
            assert np.array_equal(pile.counts(lo, hi), exp[lo:hi]), (lo, hi)
        for rule in ((1, 0, 1), (2, 1, 2), (3, 9, 10)):
            got = pile.variants(rule[0], rule[1:])
            assert [tuple(int(v) for v in row) for row in got.tolist()] == pm.variants(exp, block, starts, *rule), rule
    print("ok", int(exp.sum()), len(once.variants(1, (0, 1))))
'''


@pytest.mark.parametrize("chunk", (1, 3, 7))
def test_chunked_downloads_in_a_child_process(rlz, chunk):
    """NOLZSS_RLZ_LOCATE_CHUNK set for a whole process: two adds of the halves and one add of all equal the model, the
    whole table coming down `chunk` positions, and the variants `chunk` records, at a time"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", CHILD], cwd=root, env=dict(os.environ, NOLZSS_RLZ_LOCATE_CHUNK=str(chunk)),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("ok "), r.stdout[-2000:] + r.stderr[-4000:]
    total, found = (int(v) for v in r.stdout.split()[1:3])
    assert total >= 5000 and found >= 10  # (24 reads of about 150 bases and a contig of 2000: some 5600 columns)


def test_variants_equal_the_model_over_the_same_counts(planted, rlz):
    ix, refs, targets, exp = planted
    with ix.pileup(primary_only=False) as pile:
        assert len(pile.variants(1, (0, 1))) == 0  # nothing added yet
        pile.add(targets)
        counts = pile.counts()
        sizes = [len(same_variants(pile.variants(rule[0], rule[1:]), counts, refs, rule, rlz)) for rule in RULES]
        assert sizes[0] >= 100 and sizes[0] > sizes[1] >= sizes[2]
        got = pile.variants(1, (0, 1))
        assert set(got["record"].tolist()) == {0, 1, 2} and set(got["allele"].tolist()) == {0, 1, 2, 3, 4, 5}
        assert np.array_equal(got["depth"], counts[got["position"].astype(np.int64), :5].sum(axis=1))


def test_a_refused_add_leaves_the_counts_as_they_were(planted):
    ix, refs, targets, exp = planted
    with ix.pileup() as pile:
        pile.add(targets[:30])
        before, info = pile.counts(), pile.info
        with pytest.raises(RuntimeError, match="Invalid nucleotide 'N' found in sequence 4"):
            pile.add([targets[40], b"ACNT"])  # align refuses this batch in the same words
        with pytest.raises(RuntimeError, match="Invalid nucleotide 'N' found in sequence 4"):
            ix.align([targets[40], b"ACNT"])
        assert pile.info == info
        same_counts(pile.counts(), before)
        assert pile.add([])["targets"] == 30 and pile.add([b"", b""]) == dict(alignments=0, ops=0, columns=0, targets=32)
        same_counts(pile.counts(), before)
        assert pile.info["adds"] == 1  # neither reached the device


def test_the_planted_substitutions_are_the_base_alleles_reported(rlz):
    """a condition, not a measurement: the seed is chosen so that the model alone meets it (the host test asserts that)"""
    ref, reads, substitutions = pm.planted_sample(random.Random(SAMPLE_SEED))
    with rlz.RlzIndex.build([ref]) as ix, ix.pileup() as pile:
        info = pile.add(reads)
        assert info["alignments"] >= len(reads) - 5 and info["targets"] == len(reads)
        counts = pile.counts()
        same_counts(counts, model_counts([ref], reads, ix.align(reads), True))
        found = pile.variants(3, (1, 2))
        same_variants(found, counts, [ref], (3, 1, 2), rlz)
        bases = found[found["allele"] < 4]
        assert list(zip(bases["position"].tolist(), bases["allele"].tolist())) == substitutions
        assert (bases["ref_base"] == [pm.CODE[ref[p]] for p, _ in substitutions]).all() and (bases["rev"] > 0).all()


def test_the_index_answers_align_as_before_beside_a_pileup_and_after_it(planted, rlz):
    ix, refs, targets, exp = planted
    subset = targets[:25] + targets[-1:]
    before = ix.align(subset)
    pile = ix.pileup()
    pile.add(subset)
    beside = ix.align(subset)
    pile.close()
    pile.close()
    after = ix.align(subset)
    for got in (beside, after):
        assert sorted(got) == sorted(before) and all(np.array_equal(got[k], before[k]) for k in before)
    with pytest.raises(ValueError, match="the pileup is closed"):
        pile.counts()
    with rlz.RlzIndex.build([refs[0][:500]]) as other:
        orphan = other.pileup()
    with pytest.raises(ValueError, match="the index is closed"):
        orphan.add(subset)
    orphan.close()
