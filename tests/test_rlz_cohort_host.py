"""The model of the cohort (tests/rlz_cohort_model.py) against calls, matrices and sites written out by hand, the
condition of the end-to-end test on the all-CPU path, and everything the new entry points decide before any device
work.  No GPU."""
import ctypes as C
import functools
import os
import random
import re
import subprocess
import sys

import numpy as np
import pytest

import rlz_align_model as am
import rlz_cohort_model as hm
import rlz_consensus_model as km
import rlz_pileup_model as pm
import rlz_seed_chain_model as cm
from nolzss_amd import _lib
from nolzss_amd import _noLZSS as native
from nolzss_amd._noLZSS import COHORT_SITE_DTYPE, COHORT_MAX_SAMPLES  # (the feature: none without it)

COHORT_SEEDS = (1, 2)  # tests/test_gpu_rlz_cohort.py runs the same cohorts on the device
NEW_SYMBOLS = ("nolzss_rlz_cohort_open", "nolzss_rlz_cohort_add_pileup", "nolzss_rlz_cohort_add_calls", "nolzss_rlz_cohort_info",
               "nolzss_rlz_cohort_samples", "nolzss_rlz_cohort_distances", "nolzss_free_rlz_cohort_distances_result",
               "nolzss_rlz_cohort_sites", "nolzss_free_rlz_cohort_sites_result", "nolzss_rlz_cohort_columns",
               "nolzss_rlz_cohort_calls", "nolzss_rlz_cohort_close")


def row(a=0, c=0, g=0, t=0, dele=0, ins=0, rev=0, brk=0):
    return [a, c, g, t, dele, ins, rev, brk]


def test_calls_from_counts_by_hand():
    block = b"ACG\x01TTA"
    counts = np.array([row(a=3),            # the block's base
                       row(c=2, t=2),       # a tie: the block's base wins
                       row(a=2, t=2),       # a tie without the block's base: the smallest channel
                       row(a=9),            # a separator: no call whatever was counted
                       row(t=1, dele=2),    # DEL is the plurality
                       row(),               # no depth
                       row(a=2, c=1, g=1)], dtype=np.uint32)
    assert hm.raw_calls_from_counts(counts, block, 1, 1, 2) == b"ACA.-nA"
    assert hm.calls_from_counts(counts, block, 1, 1, 2) == b"ACANNNA"
    assert hm.raw_calls_from_counts(counts, block, 3, 1, 2) == b"ACA.-nA"
    assert hm.raw_calls_from_counts(counts, block, 4, 0, 1) == b"nCA.nnA"  # (depth 3 < 4; the fraction plays no part)
    assert hm.raw_calls_from_counts(counts, block, 1, 3, 4) == b"Ann.nnn"  # (2 of 3 and 2 of 4 stay below 3 / 4)
    assert hm.infos(b"ACA.-nA", block) == dict(called=4, low=1, deleted=1, differs=1)
    # what the consensus model says of the same counters: the identities of nolzss_rlz_cohort_add_pileup
    for min_depth, num, den in ((1, 1, 2), (3, 1, 2), (4, 0, 1), (1, 3, 4)):
        cons = km.consensus(counts, [], block, min_depth, num, den, 0)
        mine = hm.infos(hm.raw_calls_from_counts(counts, block, min_depth, num, den), block)
        assert mine == dict(called=cons["called"] - cons["deleted"], low=cons["low_positions"], deleted=cons["deleted"],
                            differs=cons["substitutions"])


def test_calls_from_bytes_by_hand():
    block = b"ACG\x01TTA"
    assert hm.raw_calls_from_bytes(b"acgtN-\x00", block) == b"ACG.nnn"
    assert hm.raw_calls_from_bytes(b"TTTTTTT", block) == b"TTT.TTT"
    assert hm.calls_from_bytes(b"acgtN-\x00", block) == b"ACGNNNN"
    assert hm.infos(b"TTT.TTT", block) == dict(called=6, low=0, deleted=0, differs=4)
    assert hm.infos(b"ACG.nnn", block) == dict(called=3, low=3, deleted=0, differs=0)
    with pytest.raises(AssertionError):
        hm.raw_calls_from_bytes(b"AC", block)


def test_distances_sites_and_columns_by_hand():
    block = b"AAAA\x01CCCC"
    calls = [b"AAAANCCCC",
             b"ATNANCCGC",
             b"NTNTNNNGN"]
    diff, comp = hm.distances(calls)
    assert diff == [[0, 2, 3], [2, 0, 1], [3, 1, 0]]
    assert comp == [[8, 7, 3], [7, 7, 3], [3, 3, 3]]
    starts = hm.record_starts(block)
    assert starts == [0, 5]
    #                 position, offset, record, present, counts, reference
    assert hm.sites(calls, block, starts, 0, True) == [(1, 1, 0, 3, (1, 0, 0, 2), 0), (3, 3, 0, 3, (2, 0, 0, 1), 0),
                                                       (7, 2, 1, 3, (0, 1, 2, 0), 1)]
    assert hm.sites(calls, block, starts, 3, True) == hm.sites(calls, block, starts, 0, True)
    assert hm.sites(calls, block, starts, 4, True) == []
    # samples 1 and 2 alone agree on T and G where the block has A and C: sites only with the reference
    assert [r[0] for r in hm.sites(calls[1:], block, starts, 0, True)] == [1, 3, 7]
    assert [r[0] for r in hm.sites(calls[1:], block, starts, 0, False)] == [3]
    assert [r[0] for r in hm.sites(calls[1:], block, starts, 2, True)] == [1, 3, 7]
    assert hm.sites(calls[1:], block, starts, 3, True) == []
    assert hm.columns(calls, [7, 1, 1, 4]) == [b"CAAN", b"GTTN", b"GTTN"]
    assert hm.columns(calls, []) == [b"", b"", b""]


@functools.lru_cache(maxsize=None)
def cohort_on_the_cpu(seed):
    cohort = hm.planted_cohort(random.Random(seed))
    ref = cohort["reference"]
    params = dict(am.DEFAULTS)
    band, max_flank = params.pop("band"), params.pop("max_flank")
    calls = []
    for reads in cohort["reads"]:
        exp = am.expected([ref], reads, cm.expected([ref], reads, True, **params), band, max_flank)
        counts, events = km.walk(ref, pm.records(exp), exp["ops"], exp["op_offsets"], reads, True, True)
        calls.append(hm.raw_calls_from_counts(counts, ref, 1, 1, 2))
    return cohort, calls


@pytest.mark.parametrize("seed", COHORT_SEEDS)
def test_the_distances_of_the_planted_cohort_are_the_planted_ones(seed):
    """the condition of the end-to-end test on the all-CPU path: chain model, align model, walk, calls, distances"""
    cohort, raw = cohort_on_the_cpu(seed)
    ref, B = cohort["reference"], len(cohort["reference"])
    calls = [hm.letters(r) for r in raw]
    diff, comp = hm.distances(calls)
    assert diff == cohort["differences"]
    assert diff[0][1] == 3 and diff[2][3] == 3 and min(diff[i][j] for i in (0, 1) for j in (2, 3, 4)) >= 7  # the tree shows
    # only the stated stretch without reads and the deletion lower `compared`
    (del_sample, del_at, del_len), (gap_sample, gap_lo, gap_hi) = cohort["deletion"], cohort["gap"]
    for i in range(len(calls)):
        for j in range(len(calls)):
            lost = (del_len if del_sample in (i, j) else 0) + (gap_hi - gap_lo if gap_sample in (i, j) else 0)
            assert comp[i][j] == B - lost, (i, j)
    for s, r in enumerate(raw):
        info = hm.infos(r, ref)
        assert info["deleted"] == (del_len if s == del_sample else 0) and info["low"] == (gap_hi - gap_lo if s == gap_sample else 0)
        seen = [p for p in cohort["snps"][s] if not (s == gap_sample and gap_lo <= p < gap_hi)]
        assert info["differs"] == len(seen) and len(seen) < len(cohort["snps"][s]) + (s != gap_sample)  # (a private SNP lies in the stretch)
    assert calls[gap_sample][gap_lo:gap_hi] == b"N" * (gap_hi - gap_lo) == cohort["truth"][gap_sample][gap_lo:gap_hi]
    # the core sites: every planted position that all five samples call, and no other
    planted = sorted({p for snps in cohort["snps"] for p in snps})
    core = hm.sites(calls, ref, [0], len(calls), True)
    assert [r[0] for r in core] == [p for p in planted if not gap_lo <= p < gap_hi]
    shared = [r for r in core if r[3] == 5 and max(r[4]) == 5]  # all agree on a base that is not the reference's
    assert [r[0] for r in shared] == [p for p in planted if all(p in snps for snps in cohort["snps"]) and not gap_lo <= p < gap_hi]
    assert [r[0] for r in hm.sites(calls, ref, [0], len(calls), False)] == [r[0] for r in core if r not in shared]


def test_symbols_layouts_and_exports():
    header = open(_lib.__file__.replace("nolzss_amd/_lib.py", "include/nolzss_hip.h")).read()
    declared = set(re.findall(r"\b(nolzss_(?:free_)?rlz_cohort\w*)\(", header))
    assert declared == set(NEW_SYMBOLS)
    for name in NEW_SYMBOLS:
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(_lib.lib, name)
    assert "#define NOLZSS_RLZ_COHORT_MAX_SAMPLES 16384" in header and COHORT_MAX_SAMPLES == 16384
    assert 2 * 4 * COHORT_MAX_SAMPLES ** 2 <= 1 << 32  # both matrices of a full cohort stay addressable
    assert COHORT_SITE_DTYPE.itemsize == 48 and COHORT_SITE_DTYPE.names == hm.SITE_FIELDS
    assert [COHORT_SITE_DTYPE.fields[n][1] for n in hm.SITE_FIELDS] == [0, 8, 16, 20, 24, 40]
    assert COHORT_SITE_DTYPE["counts"].shape == (4,)
    assert C.sizeof(_lib.RlzCohortSampleInfo) == 40 and C.sizeof(_lib.RlzCohortSummary) == 40
    assert C.sizeof(_lib.RlzCohortDistancesResult) == 24 and C.sizeof(_lib.RlzCohortSitesResult) == 16
    import noLZSS.genomics.rlz as shim
    from nolzss_amd.genomics import rlz
    for name in ("COHORT_SITE_DTYPE", "RlzCohort"):
        assert name in rlz.__all__ and name in shim.__all__ and getattr(shim, name) is getattr(rlz, name)
    assert rlz.COHORT_SITE_DTYPE is native.COHORT_SITE_DTYPE
    for method in ("add", "add_calls", "distances", "sites", "alignment", "calls", "samples", "close"):
        assert hasattr(rlz.RlzCohort, method)
    for method in ("add_pileup", "add_calls", "distances", "sites", "columns", "calls", "samples", "close"):
        assert hasattr(native.RlzCohortHandle, method)
    assert hasattr(rlz.RlzIndex, "cohort")


def test_bad_arguments_raise_before_the_native_layer_is_touched():
    from nolzss_amd.genomics import rlz
    ix = rlz.RlzIndex.__new__(rlz.RlzIndex)
    ix._handle = None
    with pytest.raises(ValueError, match="the index is closed"):
        ix.cohort()
    cohort = rlz.RlzCohort(None, ix)  # closed: anything that reached for the handle would say so
    pile = rlz.RlzPileup(None, ix, True)
    for kwargs in (dict(min_depth=0), dict(min_depth=1 << 32), dict(min_fraction=(3, 2)), dict(min_fraction=(1, 0)),
                   dict(min_fraction=(1, 1 << 32)), dict(min_fraction=0.5), dict(min_fraction=(-1, 2))):
        with pytest.raises(ValueError, match="min_depth|min_fraction"):
            cohort.add(pile, **kwargs)
    with pytest.raises(ValueError, match="min_present"):
        cohort.sites(min_present=-1)
    with pytest.raises(ValueError, match="min_present"):
        cohort.alignment(min_present=-1)
    for call in (lambda: cohort.add(pile), lambda: cohort.add_calls(b"ACGT"), lambda: cohort.distances(), lambda: cohort.sites(),
                 lambda: cohort.alignment(), lambda: cohort.alignment([1, 2]), lambda: cohort.calls(0), lambda: cohort.info,
                 lambda: cohort.samples()):
        with pytest.raises(ValueError, match="the cohort is closed"):
            call()
    assert cohort.ids == [] and len(cohort) == 0
    cohort.close()
    # an open cohort over a closed index, and a closed pileup: the Python layer says so before the library is called
    opened = rlz.RlzCohort(native.RlzCohortHandle(C.c_void_p(0), None), ix)
    with pytest.raises(ValueError, match="the index is closed"):
        opened.distances()
    opened._handle._h = None
    # the id rules
    assert rlz._cohort_id(None, {}) is None and rlz._cohort_id(b"iso-1", {}) == "iso-1" and rlz._cohort_id("x", {"y": 0}) == "x"
    with pytest.raises(ValueError, match="distinct"):
        rlz._cohort_id("x", {"x": 0})
    with pytest.raises(ValueError, match="str or bytes"):
        rlz._cohort_id(7, {})
    # the handle's own argument checks, each in front of the native call (the stand-in handle is never read)
    class Index:
        def _handle(self):
            return C.c_void_p(0)

    h = native.RlzCohortHandle(C.c_void_p(0), Index())
    with pytest.raises(ValueError, match="min_present"):
        h.sites(-1)
    with pytest.raises(ValueError, match="min_depth"):
        h.add_pileup(None, 0)
    h._h = None
    with pytest.raises(ValueError, match="the cohort is closed"):
        h.columns([0])


def test_refusals_before_any_device_work():
    lib, bad = _lib.lib, _lib.ERR_INVALID_ARGUMENT
    stand_in = C.create_string_buffer(4096)  # zero bytes stand in for a handle where it is hardly read: a cohort of block length 0
    other = C.create_string_buffer(4096)
    out = C.c_void_p(5)
    assert lib.nolzss_rlz_cohort_open(None, C.byref(out)) == bad and not out.value
    assert b"handle is null" in lib.nolzss_last_error()
    assert lib.nolzss_rlz_cohort_open(stand_in, None) == bad
    info = _lib.RlzCohortSampleInfo(9, 9, 9, 9, 9)
    good = _lib.RlzConsensusParams(1, 0, 1, 2)
    assert lib.nolzss_rlz_cohort_add_pileup(None, other, C.byref(good), C.byref(info)) == bad and info.called == 0
    assert lib.nolzss_rlz_cohort_add_pileup(stand_in, None, C.byref(good), C.byref(info)) == bad
    assert lib.nolzss_rlz_cohort_add_pileup(stand_in, other, C.byref(good), None) == bad
    assert lib.nolzss_rlz_cohort_add_pileup(stand_in, other, None, C.byref(info)) == bad
    assert lib.nolzss_rlz_cohort_add_pileup(stand_in, other, C.byref(good), C.byref(info)) == bad
    assert b"the pileup is not open over the index of this cohort" in lib.nolzss_last_error()
    for min_depth, low, num, den in ((0, 0, 1, 2), (1, 2, 1, 2), (1, 0, 1, 0), (1, 0, 3, 2), (1, 0, 1, 1 << 32)):
        refused = _lib.RlzConsensusParams(min_depth, low, num, den)
        assert lib.nolzss_rlz_cohort_add_pileup(stand_in, other, C.byref(refused), C.byref(info)) == bad, (min_depth, low, num, den)
        assert b"rlz pileup: a consensus takes" in lib.nolzss_last_error() or b"denominator" in lib.nolzss_last_error()
    assert lib.nolzss_rlz_cohort_add_calls(None, b"ACGT", 4, C.byref(info)) == bad
    assert lib.nolzss_rlz_cohort_add_calls(stand_in, b"ACGT", 4, None) == bad
    assert lib.nolzss_rlz_cohort_add_calls(stand_in, b"ACGT", 4, C.byref(info)) == bad  # (the stand-in's block holds 0 positions)
    assert b"one byte per block position (0), not 4" in lib.nolzss_last_error()
    summary = _lib.RlzCohortSummary()
    assert lib.nolzss_rlz_cohort_info(None, C.byref(summary)) == bad and lib.nolzss_rlz_cohort_info(stand_in, None) == bad
    assert lib.nolzss_rlz_cohort_info(stand_in, C.byref(summary)) == _lib.OK and summary.samples == 0 and summary.device_bytes == 0
    count = C.c_size_t(7)
    assert lib.nolzss_rlz_cohort_samples(None, None, 0, C.byref(count)) == bad
    assert lib.nolzss_rlz_cohort_samples(stand_in, None, 0, None) == bad
    assert lib.nolzss_rlz_cohort_samples(stand_in, None, 3, C.byref(count)) == bad
    assert lib.nolzss_rlz_cohort_samples(stand_in, None, 0, C.byref(count)) == _lib.OK and count.value == 0
    dist = _lib.RlzCohortDistancesResult(7, None, None)
    assert lib.nolzss_rlz_cohort_distances(None, C.byref(dist)) == bad and dist.num_samples == 0
    assert lib.nolzss_rlz_cohort_distances(stand_in, None) == bad
    assert lib.nolzss_rlz_cohort_distances(stand_in, C.byref(dist)) == _lib.OK and dist.num_samples == 0 and not dist.differences
    sites = _lib.RlzCohortSitesResult(7, None)
    assert lib.nolzss_rlz_cohort_sites(None, 0, 1, C.byref(sites)) == bad and sites.num_sites == 0
    assert lib.nolzss_rlz_cohort_sites(stand_in, 0, 1, None) == bad
    assert lib.nolzss_rlz_cohort_sites(stand_in, 0, 1, C.byref(sites)) == _lib.OK and sites.num_sites == 0 and not sites.sites
    positions = (C.c_uint64 * 2)(0, 1)
    letters = C.create_string_buffer(8)
    assert lib.nolzss_rlz_cohort_columns(None, positions, 2, letters) == bad
    assert lib.nolzss_rlz_cohort_columns(stand_in, None, 2, letters) == bad
    assert lib.nolzss_rlz_cohort_columns(stand_in, positions, 2, letters) == bad
    assert b"position 0 (entry 0) lies at or beyond the block's length 0" in lib.nolzss_last_error()
    assert lib.nolzss_rlz_cohort_columns(stand_in, None, 0, None) == _lib.OK
    assert lib.nolzss_rlz_cohort_calls(None, 0, 0, 0, letters) == bad
    assert lib.nolzss_rlz_cohort_calls(stand_in, 0, 0, 1, letters) == bad and b"block length (0)" in lib.nolzss_last_error()
    assert lib.nolzss_rlz_cohort_calls(stand_in, 0, 1, 0, letters) == bad
    assert lib.nolzss_rlz_cohort_calls(stand_in, 0, 0, 0, letters) == bad and b"sample 0 of 0" in lib.nolzss_last_error()
    lib.nolzss_free_rlz_cohort_distances_result(None)
    lib.nolzss_free_rlz_cohort_sites_result(None)
    lib.nolzss_free_rlz_cohort_distances_result(C.byref(dist))
    lib.nolzss_free_rlz_cohort_sites_result(C.byref(sites))
    assert lib.nolzss_rlz_cohort_close(None) == _lib.OK


def test_the_device_buffer_counters_of_a_process_that_opened_nothing():
    """nolzss_debug_device_buffers: (0, 0) in a fresh process -- this one may hold handles of other tests --, no device
    touched, null pointers refused"""
    lib, n = _lib.lib, C.c_size_t(7)
    assert "nolzss_debug_device_buffers" in _lib.EXPORTED_SYMBOLS
    assert lib.nolzss_debug_device_buffers(None, C.byref(n)) == _lib.ERR_INVALID_ARGUMENT and n.value == 7
    assert b"output pointer is null" in lib.nolzss_last_error()
    assert lib.nolzss_debug_device_buffers(C.byref(n), None) == _lib.ERR_INVALID_ARGUMENT
    assert lib.nolzss_debug_device_buffers(C.byref(n), C.byref(C.c_size_t())) == _lib.OK
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    child = "from nolzss_amd import _noLZSS as native; print(native.debug_device_buffers())"
    r = subprocess.run([sys.executable, "-c", child], cwd=root, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip() == "(0, 0)", r.stdout[-2000:] + r.stderr[-4000:]
