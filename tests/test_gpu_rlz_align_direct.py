"""The alignment stages on arbitrary jobs, through the debug hook (nolzss_debug_rlz_align_jobs: the production sizes,
offsets, recurrence and traceback of rlz_align.hip).  Cost, end column and one code per column of every job are compared
with tests/rlz_align_model.job by integer equality."""
import random

import numpy as np
import pytest

import rlz_align_model as am

pytestmark = pytest.mark.gpu

GAP, RIGHT, LEFT = am.GAP, am.RIGHT, am.LEFT


@pytest.fixture(scope="module")
def native():
    from nolzss_amd import _noLZSS
    assert _noLZSS.device_count() >= 1, "no MI355X visible"
    return _noLZSS


def related(rng, n, rate=0.06, alphabet=b"ACGT"):
    """a query of n bases and a reference that differs from it by substitutions and single-base indels"""
    query = bytes(rng.choice(alphabet) for _ in range(n))
    ref = bytearray()
    for c in query:
        u = rng.random()
        if u < rate / 3:
            continue
        if u < 2 * rate / 3:
            ref.append(rng.choice(alphabet))
        ref.append(rng.choice(alphabet) if u > 1 - rate / 3 else c)
    return query, bytes(ref)


def check(native, query, reference, jobs, band):
    cols = [np.array([j[k] for j in jobs], dtype=np.uint32) for k in range(5)]
    got = native.debug_rlz_align_jobs(query, reference, *cols, band)
    assert len(got["cost"]) == len(got["end_col"]) == len(jobs) and len(got["col_offsets"]) == len(jobs) + 1
    columns = 0
    for n, (kind, q0, nq, y0, ny) in enumerate(jobs):
        cost, end_col, codes = am.job(kind, query, reference, q0, nq, y0, ny, band)
        mine = got["cols"][int(got["col_offsets"][n]):int(got["col_offsets"][n + 1])].tolist()
        if (int(got["cost"][n]), int(got["end_col"][n]), mine) != (cost, end_col, codes):
            raise AssertionError(f"job {n} {jobs[n]} band {band}: cost {got['cost'][n]} end {got['end_col'][n]} {mine[:40]} != "
                                 f"cost {cost} end {end_col} {codes[:40]}")
        columns += len(codes)
    assert int(got["col_offsets"][-1]) == columns == len(got["cols"])
    return got


SIZES = (0, 1, 2, 31, 32, 33, 63, 64, 65, 200)


@pytest.mark.parametrize("band,deltas", [(16, (-31, 31)), (31, (-1, 0, 1)), (0, (0,))])
def test_gaps_of_every_size_at_full_width_and_at_width_one(native, band, deltas):
    """|delta| + 2 band + 1 is 64 for the odd deltas, 63 for delta 0 at band 31, and 1 at band 0"""
    rng = random.Random(10 + band)
    query, reference = related(rng, 700)
    jobs = []
    for delta in deltas:
        assert abs(delta) + 2 * band + 1 in (64, 63, 1)
        for gq in SIZES:
            for gy in {gq + delta} | ({g for g in SIZES if g - gq == delta}):
                if gy < 0:
                    continue
                q0 = rng.randrange(0, len(query) - gq - 40)
                jobs.append((GAP, q0, gq, min(q0 + rng.randrange(0, 3), len(reference) - gy), gy))
    assert len(jobs) >= 7 * len(deltas)  # (a negative delta has no job for the three smallest gq)
    got = check(native, query, reference, jobs, band)
    assert int(got["cost"].max()) >= 1


def test_windows_that_straddle_packed_words(native):
    rng = random.Random(20)
    query, reference = related(rng, 400)
    jobs = []
    for qm in (0, 1, 31):
        for ym in (0, 1, 31):
            q0, y0 = 64 + qm, 96 + ym
            jobs += [(GAP, q0, 40, y0, 41), (GAP, q0, 70, y0, 66), (RIGHT, q0, 45, y0, 80), (LEFT, q0, 50, y0, y0),
                     (LEFT, q0 + 32, q0 + 32, y0, 60)]
    check(native, query, reference, jobs, 5)
    # unrelated windows: costs as large as the rectangle
    check(native, query, reference[::-1], jobs[:10], 5)


@pytest.mark.parametrize("band", [4, 16])
def test_flanks_with_every_kind_of_room(native, band):
    rng = random.Random(30 + band)
    query, reference = related(rng, 600)
    jobs = []
    for fq in (1, 2, band, band + 1, 40, 97):
        for avail in (0, fq - band - 1, fq - band, fq, fq + band, fq + 150):
            if avail < 0:
                continue
            q0 = rng.randrange(120, 300)
            jobs.append((RIGHT, q0, fq, q0 + rng.randrange(0, 3), avail))
            jobs.append((LEFT, q0 + fq, fq, max(q0 + fq + rng.randrange(0, 3), avail), avail))
    # left flanks that reach position 0 of both texts, of the query alone, of the reference alone
    jobs += [(LEFT, 60, 60, 61, 61), (LEFT, 33, 33, 200, 80), (LEFT, 200, 50, 48, 48), (LEFT, 1, 1, 1, 1), (LEFT, 0, 0, 0, 0)]
    # right flanks that reach the last base
    jobs += [(RIGHT, len(query) - 50, 50, len(reference) - 52, 52), (RIGHT, len(query), 0, len(reference), 0)]
    got = check(native, query, reference, jobs, band)
    clipped = sum(1 for j, n in zip(jobs, np.diff(got["col_offsets"])) if j[2] and not n)
    assert clipped >= 4  # (no end cell: avail < fq - band)


def test_two_thousand_small_jobs_among_three_large_ones(native):
    """offsets over rows and slots, and wavefronts of one workgroup that finish three thousand rows apart"""
    rng = random.Random(40)
    query, reference = related(rng, 3300, rate=0.03)
    big = [(GAP, 10, 3000, 12, 3010), (RIGHT, 100, 2990, 101, 3150), (LEFT, 3200, 3000, 3190, 3190)]
    small = []
    for _ in range(2000):
        q0, kind = rng.randrange(50, 3200), rng.choice([GAP, GAP, RIGHT, LEFT])
        nq = rng.randrange(1, 4)
        small.append((kind, q0, nq, min(q0 + rng.randrange(0, 2), len(reference) - 8), rng.randrange(0, 5)))
    jobs = [big[0]] + small[:1000] + [big[1]] + small[1000:] + [big[2]]
    got = check(native, query, reference, jobs, 8)
    assert int(np.diff(got["col_offsets"]).max()) >= 3000


@pytest.mark.parametrize("unit", [b"A", b"AC", b"AAC"])
def test_low_complexity_texts_where_every_cell_ties(native, unit):
    query, reference = unit * (240 // len(unit)), unit * (260 // len(unit))
    jobs = []
    for gq, gy in ((2, 3), (3, 2), (4, 6), (30, 41), (41, 30), (64, 64), (65, 60), (7, 0), (0, 7)):
        for q0 in (0, 1, 2, 33):
            jobs.append((GAP, q0, gq, q0 + 1, gy))
    for fq, avail in ((1, 2), (2, 3), (4, 6), (30, 60), (30, 25), (30, 20)):
        jobs += [(RIGHT, 3, fq, 4, avail), (LEFT, 100 + fq, fq, 150, avail)]
    check(native, query, reference, jobs, 5)
    if unit == b"A":  # (diagonal first: the indel of a run at its low end)
        assert am.job(GAP, query, reference, 0, 2, 1, 3, 5)[2] == [am.D, am.EQ, am.EQ]


def test_an_empty_job_list_and_refusals_before_launch(native):
    got = native.debug_rlz_align_jobs(b"ACGT", b"ACGT", [], [], [], [], [], 3)
    assert got["col_offsets"].tolist() == [0] and len(got["cols"]) == 0
    with pytest.raises(ValueError, match="64 diagonals"):
        native.debug_rlz_align_jobs(b"ACGT" * 30, b"ACGT" * 30, [GAP], [0], [10], [0], [60], 7)
    with pytest.raises(ValueError, match="leaves a text"):
        native.debug_rlz_align_jobs(b"ACGT", b"ACGT", [RIGHT], [2], [3], [0], [4], 3)
    # jobs without a recurrence only: no DP row at all
    got = check(native, b"ACGTACGT", b"TTTT", [(GAP, 1, 3, 0, 0), (GAP, 1, 0, 1, 2), (RIGHT, 8, 0, 4, 0), (RIGHT, 6, 2, 4, 0)], 3)
    assert got["cost"].tolist() == [3, 2, 0, 2]
