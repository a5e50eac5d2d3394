"""The inputs of tests/test_gpu_rc_positions.py hold what those tests claim to cover -- asserted from the oracle alone,
without a GPU, so that a later edit of the case list cannot quietly empty the coverage (tests/rc_positions.py)."""
import numpy as np
import pytest

import gen
import rc_positions as rp


def _on_chain(e, positions):
    return np.isin(positions, e.chain(0))


@pytest.mark.parametrize("name, least", [("family_300_joined", 400), ("copies_40_of_1500", 1), ("period_300_x40", 1)])
def test_explicit_node_rule_is_reached_off_the_chain_only(name, least):
    """positions whose forward factor is shorter than plain L* (d_u in rc_fallback_kernel) exist -- and the greedy chain
    from 0 visits none of them, which is why only the every-position test checks that rule"""
    e = rp.expected(name)
    quirks = rp.quirk_positions(e)
    assert len(quirks) >= least
    assert not _on_chain(e, quirks).any()
    # where the reverse complement wins, the oracle's answer does not show the forward candidate: the chain positions
    # that take the exact search are few, so the rule is evaluated there directly
    exact = rp.exact_search_positions(e)
    for i in exact[_on_chain(e, exact)]:
        assert not rp.quirk_at(e, int(i)), i


def test_reverse_complement_positions():
    e = rp.expected("AT_x3000")
    rc = rp.rc_chosen_positions(e)
    assert len(rc) >= 1000 and not _on_chain(e, rc).any()
    assert len(rp.rc_chosen_positions(rp.expected("far_copy_150k"))) >= 30_000


@pytest.mark.parametrize("name", rp.PERIODIC + rp.PERIODIC_IN_TILES)
def test_periodic_texts_take_the_exact_search_nearly_everywhere(name):
    e = rp.expected(name)
    assert len(rp.exact_search_positions(e)) >= 0.9 * e.N
    if name in rp.PERIODIC_IN_TILES:  # no rank finds its work list full: the tile kernel queues them itself
        assert rp.overflowing_wavefronts(e) == 0


@pytest.mark.parametrize("name", ["A_x6000", "copies_40_of_1500", "family_300_joined", "family_120_sequences",
                                  "period_300_x40"])
def test_work_lists_overflow(name):
    """more than kListCap = 128 ranks of one wavefront still searching after four steps (rc.hip): those ranks restart
    from global memory"""
    assert rp.overflowing_wavefronts(rp.expected(name)) >= 1


def test_work_lists_do_not_overflow_on_random_bases():
    e = rp.Expected([gen.random_dna(100_000, 21).tobytes()])
    assert rp.overflowing_wavefronts(e) == 0


def test_case_list_is_what_the_gpu_tests_name():
    assert len(rp.cases_single()) == 16 and len(rp.cases_multi()) == 3
    assert len(rp.cases_sizes()) == len(rp.TILE_SIZES) + len(rp.RUN_SIZES) == 29
    e = rp.expected("family_120_sequences")
    assert len(e.sent) == 240 and not e.byte_order  # sentinels above 'A': the device's order is not the byte order
    assert rp.expected("family_9_sequences").byte_order and rp.expected("tiny_sequences_x4").byte_order
    for name, seqs in rp.all_cases().items():
        assert sum(len(s) for s in seqs) <= 200_000, name
