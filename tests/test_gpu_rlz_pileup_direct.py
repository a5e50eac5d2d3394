"""The pileup stages on arbitrary alignments, through the debug hook (nolzss_debug_rlz_pileup: the production
accumulate, resolve and compose of rlz_pileup.hip).  The B x 8 counters are compared with tests/rlz_pileup_model.pileup
by integer equality, at the smallest shapes where the kernels can go wrong: a difference entry at index B, op lengths
around a wavefront and a workgroup, alignments whose ops cross workgroup and scan-tile seams, thousands of atomics on one
counter, insertions at either end, a separator between two records, and target bases across 64-bit words."""
import random

import numpy as np
import pytest

import rlz_pileup_model as pm

pytestmark = pytest.mark.gpu

I, D, EQ, X = pm.I, pm.D, pm.EQ, pm.X


@pytest.fixture(scope="module")
def native():
    from nolzss_amd import _noLZSS
    assert _noLZSS.device_count() >= 1, "no MI355X visible"
    return _noLZSS


def dna(rng, n):
    return bytes(rng.choice(b"ACGT") for _ in range(n))


def place(target, t_start, r_start, is_rc, ops, target_bases, primary=1):
    """one alignment from its first coordinates and its ops (length, code): the ends follow from what the ops consume"""
    t = sum(n for n, code in ops if code != D)
    r = sum(n for n, code in ops if code != I)
    assert t_start + t <= len(target_bases)
    return dict(target=target, t_start=t_start, t_end=t_start + t, r_start=r_start, r_end=r_start + r, is_rc=is_rc,
                primary=primary), [(n << 4) | code for n, code in ops]


def check(native, block, targets, placed, primary_only=False):
    """the hook against the model on the same alignments -> the counters"""
    alignments = [a for a, _ in placed]
    ops, offsets = [], [0]
    for _, mine in placed:
        ops += mine
        offsets.append(len(ops))
    recs = np.zeros(len(alignments), dtype=native.ALIGN_DTYPE)
    for c, a in enumerate(alignments):
        for key, v in a.items():
            recs[key][c] = v
        recs["num_ops"][c] = offsets[c + 1] - offsets[c]
        recs["columns"][c] = sum(op >> 4 for op in placed[c][1])
    got = native.debug_rlz_pileup(block, targets, recs, offsets, ops, primary_only)  # (first: it refuses what the model cannot walk)
    exp = pm.pileup(len(block), alignments, ops, offsets, targets, block, primary_only)
    assert got.shape == exp.shape and got.dtype == np.uint32
    if not np.array_equal(got, exp):
        p, ch = np.argwhere(got != exp)[0]
        raise AssertionError(f"position {p} channel {pm.CHANNELS[ch]}: {got[p].tolist()} != {exp[p].tolist()} "
                             f"({int((got != exp).sum())} counters differ)")
    return got


def test_one_base_and_runs_that_end_the_block(native):
    rng = random.Random(1)
    block = dna(rng, 37)
    B = len(block)
    got = check(native, block, [b"A"], [place(0, 0, 20, 0, [(1, EQ)], b"A")])
    assert got.sum() == 1 and got[20, pm.CODE[block[20]]] == 1
    # the -1 of a difference entry at index B: `=` runs and a reverse-strand span that end at B - 1, alone and stacked
    read = dna(rng, 12)
    for rc in (0, 1):
        for ops in ([(12, EQ)], [(5, EQ), (2, X), (5, EQ)], [(4, EQ), (3, D), (5, EQ)], [(7, EQ), (5, X)], [(7, EQ), (5, D)],
                    [(5, X), (7, EQ)]):
            placed = place(0, 0, 0, rc, ops, read)
            r = placed[0]["r_end"]
            placed[0].update(r_start=B - r, r_end=B)
            got = check(native, block, [read], [placed, placed, placed])
            assert got[B - 1, :5].sum() == 3 and got[B - 1, pm.REV] == 3 * rc
    whole = check(native, block, [block], [place(0, 0, 0, 0, [(B, EQ)], block), place(0, 0, 0, 1, [(B, EQ)], block)])
    assert whole[:, :4].sum(axis=1).tolist() == [2] * B and whole[:, pm.REV].tolist() == [1] * B


@pytest.mark.parametrize("length", (63, 64, 65, 255, 256, 257))
def test_op_lengths_around_a_wavefront_and_a_workgroup(native, length):
    rng = random.Random(length)
    block = dna(rng, 3 * length + 40)
    read = dna(rng, 3 * length + 20)
    placed = []
    for rc in (0, 1):
        for code in (EQ, X, D, I):
            placed.append(place(0, 3, 7, rc, [(5, EQ), (length, code), (4, EQ)], read))
        placed.append(place(0, 1, 11, rc, [(length, X), (length, EQ), (length, D), (length, I), (3, X)], read))
    got = check(native, block, [read], placed)
    assert got[:, pm.DEL].sum() == 4 * length and got[:, pm.INS].sum() == 4


def test_300_ops_in_one_alignment_cross_the_workgroup_seams(native):
    rng = random.Random(300)
    pattern = [(2, EQ), (1, X), (3, EQ), (1, D), (1, EQ), (2, I)]
    ops = (pattern * 50)[:300]
    r = sum(n for n, code in ops if code != I)
    block, read = dna(rng, r + 60), dna(rng, 460)
    placed = [place(0, 2, 5, 0, ops[:7], read)]          # seven ops in front: the long alignment starts mid-workgroup
    placed += [place(0, 1, 30, rc, ops, read) for rc in (0, 1, 1, 0)]
    placed.append(place(0, 0, 9, 1, ops[:5], read))
    got = check(native, block, [read], placed)
    assert got[:, pm.INS].sum() == 4 * 50 + 1 and (got[:, pm.REV] == 2).any()


def test_5000_alignments_over_one_window_on_both_strands(native):
    """atomic contention on a handful of counters, depths far above a wavefront, and -- with 25000 ops -- the scans of
    the per-op prefixes across their 4096-entry tiles; X and DEL meet at one position"""
    rng = random.Random(5000)
    block = dna(rng, 64)
    fwd_ops = [(10, EQ), (1, X), (5, EQ), (2, D), (22, EQ)]           # X at window position 10
    rev_ops = [(27, EQ), (3, D), (10, EQ)]                            # in the block: DEL at window positions 10 .. 12
    read_f, read_r = dna(rng, 38), dna(rng, 37)
    placed = []
    for j in range(5000):
        placed.append(place(j % 2, 0, 12, 0, fwd_ops, read_f) if j % 2 == 0 else place(1, 0, 12, 1, rev_ops, read_r))
    got = check(native, block, [read_f, read_r], placed)
    assert got[12:52, :5].sum(axis=1).tolist() == [5000] * 40 and got[12:52, pm.REV].tolist() == [2500] * 40
    assert got[22, pm.DEL] == 2500 and got[22, :4].sum() == 2500 and not got[:12].any() and not got[52:].any()


def test_insertions_at_either_end_on_both_strands(native):
    rng = random.Random(9)
    block, read = dna(rng, 30), dna(rng, 20)
    for rc in (0, 1):
        got = check(native, block, [read], [place(0, 0, 10, rc, [(3, I), (6, EQ), (2, I)], read),
                                            place(0, 2, 10, rc, [(1, I), (6, X)], read),
                                            place(0, 2, 10, rc, [(6, D), (4, I)], read),
                                            place(0, 0, 29, rc, [(1, I), (1, EQ), (1, I)], read),
                                            place(0, 0, 0, rc, [(2, I), (1, EQ), (1, I)], read)])
        assert got[10, pm.INS] == 2 and got[15, pm.INS] == 2 and got[29, pm.INS] == 2 and got[0, pm.INS] == 2
        assert got[:, pm.INS].sum() == 8 and got[:, pm.BREAK].sum() > 0


def test_a_separator_between_two_records_stays_zero(native):
    rng = random.Random(11)
    first, second = dna(rng, 70), dna(rng, 45)
    block = first + b"\x01" + second
    read = dna(rng, 40)
    placed = []
    for rc in (0, 1):
        placed.append(place(0, 1, 70 - 12, rc, [(4, EQ), (2, X), (1, I), (3, D), (3, EQ)], read))   # ends at the base in front
        placed.append(place(0, 0, 71, rc, [(2, X), (5, EQ), (2, D), (2, I), (6, EQ)], read))        # begins at the base behind
        placed.append(place(0, 3, 71 + 45 - 9, rc, [(9, EQ)], read))                                # ends the block
    got = check(native, block, [read], placed)
    assert not got[70].any() and got[69, :5].sum() == 2 and got[71, :5].sum() == 2 and got[69, pm.BREAK] + got[71, pm.BREAK] >= 2
    with pytest.raises(ValueError, match="covers a separator"):
        check(native, block, [read], [place(0, 0, 65, 0, [(10, EQ)], read)])


def test_target_bases_across_64_bit_words(native):
    """a first target of 5 bases shifts the second to batch position 6: its X runs cross the words at 32, 64 and 96"""
    rng = random.Random(13)
    block = dna(rng, 150)
    short, read = dna(rng, 5), dna(rng, 120)
    placed = []
    for rc in (1, 0):
        placed.append(place(1, 0, 10, rc, [(120, X)], read))
        placed.append(place(1, 17, 3, rc, [(4, EQ), (30, X), (2, D), (41, X), (1, I), (20, X)], read))
        placed.append(place(0, 0, 140, rc, [(5, X)], short))
    got = check(native, block, [short, read], placed)
    assert got[:, pm.REV].sum() == 120 + 97 + 5


def test_random_alignments_over_two_records(native):
    rng = random.Random(17)
    first, second = dna(rng, 333), dna(rng, 259)
    block = first + b"N" + second
    targets = [dna(rng, rng.randrange(1, 200)) for _ in range(9)]
    placed = []
    while len(placed) < 400:
        t = rng.randrange(len(targets))
        ops = [(rng.randrange(1, 9), rng.choice((EQ, EQ, EQ, X, D, I))) for _ in range(rng.randrange(1, 12))]
        tq = sum(n for n, code in ops if code != D)
        rq = sum(n for n, code in ops if code != I)
        lo, hi = rng.choice(((0, 333), (334, 334 + 259)))
        if tq > len(targets[t]) or rq == 0 or rq > hi - lo:
            continue
        placed.append(place(t, rng.randrange(0, len(targets[t]) - tq + 1), rng.randrange(lo, hi - rq + 1), rng.randrange(2), ops,
                            targets[t], primary=rng.randrange(2)))
    every = check(native, block, targets, placed)
    primary = check(native, block, targets, placed, primary_only=True)
    assert not every[333].any() and 0 < primary.sum() < every.sum()


def test_no_alignment_and_none_that_is_primary(native):
    rng = random.Random(19)
    block, read = dna(rng, 50), dna(rng, 30)
    assert not check(native, block, [read], []).any()
    placed = [place(0, 0, 5, rc, [(10, EQ), (2, X), (1, I), (3, D)], read, primary=0) for rc in (0, 1)]
    assert not check(native, block, [read], placed, primary_only=True).any()  # (the kernels run and write nothing)
    assert check(native, block, [read], placed).sum() > 0
