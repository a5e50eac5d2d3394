"""A cohort of samples on the relative-LZ index, end to end on the device (rlz_cohort.hip, rlz_cohort_api.hip): reads of
the planted cohort go through normalised pileups into the cohort; the calls of every sample equal the model's over the
pileup's own counters, the four counts satisfy their identities with the consensus, distances, sites and the alignment
equal the model over those calls, and the differences are the planted ones."""
import random

import numpy as np
import pytest

import rlz_cohort_model as hm

pytestmark = pytest.mark.gpu

COHORT_SEEDS = (1, 2)  # tests/test_rlz_cohort_host.py asserts the condition on these cohorts for the models alone
RULES = ((1, (1, 2)), (1, (0, 1)), (3, (9, 10)))


@pytest.fixture(scope="module")
def rlz():
    from nolzss_amd import _noLZSS
    assert _noLZSS.device_count() >= 1, "no MI355X visible"
    from nolzss_amd.genomics import rlz
    return rlz


def site_rows(found):
    return [(int(r["position"]), int(r["record_offset"]), int(r["record"]), int(r["present"]), tuple(int(v) for v in r["counts"]),
             int(r["reference"])) for r in found]


@pytest.fixture(scope="module", params=COHORT_SEEDS)
def piled(rlz, request):
    """the planted cohort of one seed with one normalised pileup per sample, the reads added"""
    cohort = hm.planted_cohort(random.Random(request.param))
    ix = rlz.RlzIndex.build([cohort["reference"]])
    piles = []
    for reads in cohort["reads"]:
        pile = ix.pileup(normalize_indels=True)
        pile.add(reads)
        piles.append(pile)
    yield ix, cohort, piles
    for pile in piles:
        pile.close()
    ix.close()


@pytest.mark.parametrize("rule", RULES)
def test_calls_and_counts_under_three_rules(piled, rule):
    ix, cohort, piles = piled
    ref = cohort["reference"]
    min_depth, fraction = rule
    with ix.cohort() as co:
        for s, pile in enumerate(piles):
            before = pile.counts()
            info = co.add(pile, id=f"iso-{s}", min_depth=min_depth, min_fraction=fraction)
            after = pile.counts()
            assert np.array_equal(before, after)  # the add changes no counter
            raw = hm.raw_calls_from_counts(after, ref, min_depth, *fraction)
            assert info == dict(hm.infos(raw, ref), sample=s)
            assert co.calls(s) == co.calls(f"iso-{s}") == hm.letters(raw)
            cons = pile.consensus(min_depth, fraction)
            assert info["called"] == cons["called"] - cons["deleted"] and info["deleted"] == cons["deleted"]
            assert info["differs"] == cons["substitutions"] and info["low"] == cons["low_positions"]
        assert co.ids == [f"iso-{s}" for s in range(len(piles))]
        assert [dict(i) for i in co.samples()] == [dict(hm.infos(hm.raw_calls_from_counts(p.counts(), ref, min_depth, *fraction), ref),
                                                        sample=s, id=f"iso-{s}") for s, p in enumerate(piles)]


def test_distances_sites_and_the_alignment_of_the_planted_cohort(piled, rlz):
    ix, cohort, piles = piled
    ref, n = cohort["reference"], len(piles)
    with ix.cohort() as co:
        for pile in piles:
            co.add(pile)
        calls = [hm.calls_from_counts(pile.counts(), ref, 1, 1, 2) for pile in piles]
        assert [co.calls(s) for s in range(n)] == calls
        diff, comp = hm.distances(calls)
        got = co.distances()
        assert got["differences"].tolist() == diff and got["compared"].tolist() == comp
        assert got["differences"].tolist() == cohort["differences"]  # the planted truth
        assert got["called"].tolist() == [comp[s][s] for s in range(n)]
        (del_sample, del_at, del_len), (gap_sample, gap_lo, gap_hi) = cohort["deletion"], cohort["gap"]
        assert got["to_reference"].tolist() == [sum(1 for p in cohort["snps"][s] if not (s == gap_sample and gap_lo <= p < gap_hi))
                                                for s in range(n)]
        for min_present, with_reference in ((None, True), (None, False), (0, True), (n - 1, True), (n + 1, True)):
            found = co.sites(min_present, with_reference)
            assert found.dtype == rlz.COHORT_SITE_DTYPE
            assert site_rows(found) == hm.sites(calls, ref, [0], n if min_present is None else min_present, with_reference)
        planted = sorted({p for snps in cohort["snps"] for p in snps})
        positions, letters = co.alignment()  # the core-SNP alignment
        assert positions.tolist() == [p for p in planted if not gap_lo <= p < gap_hi]
        assert [bytes(row) for row in letters] == hm.columns(calls, positions.tolist())
        assert [bytes(row) for row in letters] == hm.columns(cohort["truth"], positions.tolist())
        visible = [p for p in planted if any(p in cohort["snps"][s] and not (s == gap_sample and gap_lo <= p < gap_hi) for s in range(n))]
        every, shown = co.alignment(min_present=0)  # every planted position a read shows, the stretch without reads included
        assert every.tolist() == visible and [bytes(row) for row in shown] == hm.columns(calls, visible)
        hidden = [p for p in planted if p not in visible]  # the private SNP of the sample without reads there: nobody sees it
        assert hidden and all(gap_lo <= p < gap_hi for p in hidden)
        assert [bytes(row) for row in co.alignment(hidden)[1]] == [b"N" * len(hidden) if s == gap_sample else bytes(ref[p] for p in hidden)
                                                                  for s in range(n)]
        there, cols = co.alignment(range(del_at - 2, del_at + del_len + 2))
        assert bytes(cols[del_sample]) == calls[del_sample][del_at - 2:del_at + del_len + 2] and there.tolist() == list(range(del_at - 2, del_at + del_len + 2))
        assert calls[del_sample].count(b"N") == del_len  # (the deletion lies at its leftmost place: inside a repeat, left of del_at)


def test_foreign_and_closed_handles_are_refused_and_align_answers_as_before(piled, rlz):
    ix, cohort, piles = piled
    reads = cohort["reads"][0][:25]
    before = ix.align(reads)
    co = ix.cohort()
    co.add(piles[0])
    with rlz.RlzIndex.build([cohort["sequences"][2]]) as other, other.pileup(normalize_indels=True) as foreign:
        foreign.add(reads)
        with pytest.raises(ValueError, match="not open over the index of this cohort"):
            co.add(foreign)
        with other.cohort() as theirs, pytest.raises(ValueError, match="not open over the index of this cohort"):
            theirs.add(piles[0])
    closed = ix.pileup()
    closed.close()
    with pytest.raises(ValueError, match="the pileup is closed"):
        co.add(closed)
    assert co.info["samples"] == 1 and len(co) == 1
    co.distances()
    beside = ix.align(reads)
    co.close()
    co.close()
    after = ix.align(reads)
    for got in (beside, after):
        assert sorted(got) == sorted(before) and all(np.array_equal(got[k], before[k]) for k in before)
    for call in (co.distances, co.sites, co.alignment, lambda: co.add(piles[0]), lambda: co.calls(0)):
        with pytest.raises(ValueError, match="the cohort is closed"):
            call()
