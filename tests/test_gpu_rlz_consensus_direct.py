"""The normalised pileup walk, the insertion log, the allele table and the consensus on arbitrary alignments, through the
debug hook (nolzss_debug_rlz_pileup_consensus: the production accumulate, resolve, compose, allele sort and consensus
stages).  Counters, alleles, text, map and statistics are compared with tests/rlz_consensus_model.py by integer and byte
equality, at the smallest shapes where the kernels can go wrong."""
import random

import numpy as np
import pytest

import rlz_consensus_model as km
import rlz_pileup_model as pm

pytestmark = pytest.mark.gpu

I, D, EQ, X = pm.I, pm.D, pm.EQ, pm.X


@pytest.fixture(scope="module")
def native():
    from nolzss_amd import _noLZSS
    assert _noLZSS.device_count() >= 1, "no MI355X visible"
    return _noLZSS


def dna(rng, n, letters=b"ACGT"):
    return bytes(rng.choice(letters) for _ in range(n))


def revcomp(s):
    return s.translate(pm.COMP)[::-1]


def place(target, t_start, r_start, is_rc, ops, target_bases, primary=1):
    """one alignment from its first coordinates and its ops (length, code): the ends follow from what the ops consume"""
    t = sum(n for n, code in ops if code != D)
    r = sum(n for n, code in ops if code != I)
    assert t_start + t <= len(target_bases)
    return dict(target=target, t_start=t_start, t_end=t_start + t, r_start=r_start, r_end=r_start + r, is_rc=is_rc,
                primary=primary), [(n << 4) | code for n, code in ops]


def stretch_of(block, r_start, ops, rng):
    """the forward read an alignment of these ops at r_start describes: `=` copies the block, X differs from it, D skips
    it; an I op is (n, I, word) and inserts the word -> (read, ops as (length, code))"""
    read, r, plain = bytearray(), r_start, []
    for op in ops:
        n, code = op[0], op[1]
        plain.append((n, code))
        if code == I:
            read += op[2] if len(op) > 2 else dna(rng, n)
            assert len(op) < 3 or len(op[2]) == n
            continue
        if code == EQ:
            read += block[r:r + n]
        elif code == X:
            read += bytes(rng.choice([c for c in b"ACGT" if c != block[r + j]]) for j in range(n))
        r += n
    return bytes(read), plain


def on_strand(target, block, r_start, ops, rng, rc):
    """-> (the target's bases, the placed alignment) of one stretch read on the forward or on the reverse strand"""
    read, plain = stretch_of(block, r_start, ops, rng)
    if rc:
        return revcomp(read), place(target, 0, r_start, 1, plain[::-1], read)
    return read, place(target, 0, r_start, 0, plain, read)


def record_starts(block):
    return [0] + [p + 1 for p in range(len(block)) if block[p:p + 1].upper() not in (b"A", b"C", b"G", b"T")]


def check(native, block, targets, placed, primary_only=False, normalize=True, min_depth=1, fraction=(1, 2), low="reference"):
    """the hook against the model on the same alignments -> (the hook's dict, the model's events)"""
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
    got = native.debug_rlz_pileup_consensus(block, targets, recs, offsets, ops, primary_only, normalize, min_depth, fraction, low)
    counts, events = km.walk(block, alignments, ops, offsets, targets, primary_only, normalize)
    assert got["counts"].shape == counts.shape and got["counts"].dtype == np.uint32
    if not np.array_equal(got["counts"], counts):
        p, ch = np.argwhere(got["counts"] != counts)[0]
        raise AssertionError(f"position {p} channel {pm.CHANNELS[ch]}: {got['counts'][p].tolist()} != {counts[p].tolist()} "
                             f"({int((got['counts'] != counts).sum())} counters differ)")
    table = km.alleles(events)
    exp = km.insertions(table, counts, record_starts(block), 1, 0, 1)
    assert len(exp) == len(table)  # (count >= 1 and fraction 0: the whole table)
    ins = got["insertions"]
    assert ins.dtype == native.INSERTION_DTYPE
    assert [tuple(int(v) for v in rec.tolist()[:8]) + (tuple(int(w) for w in rec["bases"]),) for rec in ins] == exp
    cons = km.consensus(counts, table, block, min_depth, fraction[0], fraction[1], 1 if low == "N" else 0)
    assert got["consensus"]["records"] == cons["records"]
    assert got["consensus"]["starts"].tolist() == cons["starts"]
    assert {name: got["consensus"][name] for name in km.STATS} == {name: cons[name] for name in km.STATS}
    return got, events


def test_every_shift_of_a_deletion_and_an_insertion_on_both_strands(native):
    """shifts 0, 1, n - 1, n, n + 1 (the rotation wraps) and the whole preceding `=` run; either strand of one stretch
    gives the same counters and alleles"""
    rng = random.Random(1)
    #          0         1         2         3
    #          0123456789012345678901234567890123
    block = b"GTCAAAAAAAAGTCACACACACTGGATATATATATATCGGT"
    cases = []
    for m in range(1, 9):                       # the `=` run in front of the gap: 1 .. 8 bases, the first at position 2
        for n in (1, 2, 3):
            cases.append((2, [(m, EQ), (n, D), (4, EQ)]))                    # inside the As: shift min(m, what matches)
            cases.append((2, [(m, EQ), (n, I, b"A" * n), (4, EQ)]))
            cases.append((13, [(m, EQ), (n, I, (b"AC" * 2)[:n]), (3, EQ)]))  # inside ACACACAC: rotations
            cases.append((23, [(m, EQ), (2, D), (2, EQ)]))                   # inside ATATATA
    for r_start, ops in cases:
        fwd, placed_f = on_strand(0, block, r_start, ops, rng, False)
        rev, placed_r = on_strand(0, block, r_start, ops, rng, True)
        got_f, events_f = check(native, block, [fwd], [placed_f])
        got_r, events_r = check(native, block, [rev], [placed_r])
        assert np.array_equal(got_f["counts"][:, :6], got_r["counts"][:, :6]) and events_f == events_r, (r_start, ops)
        assert np.array_equal(got_f["insertions"], got_r["insertions"])
    # the whole `=` run given up, a deletion moved to r_start; without the flag nothing moves
    fwd, placed = on_strand(0, block, 3, [(5, EQ), (2, D), (3, EQ)], rng, False)
    got, _ = check(native, block, [fwd], [placed])
    assert got["counts"][3:5, pm.DEL].tolist() == [1, 1] and got["counts"][5:10, 0].tolist() == [1] * 5
    got, _ = check(native, block, [fwd], [placed], normalize=False)
    assert got["counts"][8:10, pm.DEL].tolist() == [1, 1]


@pytest.mark.parametrize("run", (1023, 1024, 1025))
def test_the_cap_of_a_shift_inside_a_homopolymer(native, run):
    rng = random.Random(run)
    block = b"C" + b"A" * 1100 + b"GT"
    placed, targets = [], []
    for rc in (False, True):
        for gap in ((1, D), (2, I, b"AA")):
            read, one = on_strand(len(targets), block, 3, [(run, EQ), gap, (6, EQ)], rng, rc)
            targets.append(read)
            placed.append(one)
    got, events = check(native, block, targets, placed)
    at = 3 + run - min(run, 1024)
    assert got["counts"][at, pm.DEL] == 2 and [e[0] for e in events] == [max(at - 1, 3)] * 2


def test_compared_bases_across_the_words_of_the_packed_block(native):
    """a D and an I whose block bases cross 64-bit words of the packed block (32 bases each) at 31 / 32 / 33 and
    63 / 64 / 65, in a run and in a period-3 repeat, with a first target that moves the reads off the word grid"""
    rng = random.Random(3)
    for block in (b"GT" + b"C" * 90 + b"AG", b"GT" + b"CAT" * 30 + b"AG"):
        unit = b"C" if block[2:4] == b"CC" else None
        placed, targets = [], [dna(rng, 5)]
        for at in (31, 32, 33, 63, 64, 65):
            for start in (2, at - 3, at - 1):
                word = unit * 6 if unit else block[at - 3:at] * 2
                for gap in ((3, D), (len(word), I, word), (1, D), (4, I, word[:4])):
                    for rc in (False, True):
                        read, one = on_strand(len(targets), block, start, [(at - start, EQ), gap, (5, EQ)], rng, rc)
                        targets.append(read)
                        placed.append(one)
        check(native, block, targets, placed)


def test_indels_as_first_and_last_op_and_gaps_that_cannot_shift(native):
    rng = random.Random(5)
    block = b"TTAAAAAAAACCCCCCCCGG"
    cases = [[(2, I, b"AA"), (6, EQ)], [(2, D), (6, EQ)], [(6, EQ), (2, I, b"AA")], [(6, EQ), (2, D)],      # first / last op
             [(3, EQ), (1, X), (1, D), (3, EQ)], [(3, EQ), (1, X), (1, I, b"A"), (3, EQ)],                # behind an X
             [(3, EQ), (1, D), (1, I, b"A"), (3, EQ)], [(3, EQ), (1, I, b"A"), (1, D), (3, EQ)],          # behind a gap
             [(1, I, b"A"), (1, D), (4, EQ)], [(1, D), (1, I, b"A"), (4, EQ)]]
    for rc in (False, True):
        placed, targets = [], []
        for r_start in (2, 3, 10):
            for ops in cases:
                read, one = on_strand(len(targets), block, r_start, ops, rng, rc)
                targets.append(read)
                placed.append(one)
        check(native, block, targets, placed)
    # the shift is 0 for each of these: the flag changes nothing
    for ops in ([(3, EQ), (1, X), (1, D), (3, EQ)], [(2, D), (6, EQ)], [(2, I, b"AA"), (6, EQ)]):
        read, one = on_strand(0, block, 3, ops, rng, False)
        with_flag, _ = check(native, block, [read], [one])
        without, _ = check(native, block, [read], [one], normalize=False)
        assert np.array_equal(with_flag["counts"], without["counts"]) and np.array_equal(with_flag["insertions"], without["insertions"])


def test_insertion_lengths_around_the_words_and_near_equal_alleles(native):
    rng = random.Random(7)
    block = dna(rng, 40)
    placed, targets = [], []
    for n in (1, 31, 32, 33, 63, 64, 65, 70):
        word = dna(rng, n)
        others = [word, word[:-1] + bytes([b"ACGT"[(b"ACGT".index(word[-1:]) + 1) % 4]])]  # differs in the last base only
        if n > 33:
            others.append(word[:32] + bytes([b"ACGT"[(b"ACGT".index(word[32:33]) + 1) % 4]]) + word[33:])  # second word only
        for copy, w in enumerate(others * 2):
            rc = copy % 2 == 1
            read, one = on_strand(len(targets), block, 4, [(9, EQ), (n, I, w), (9, EQ)], rng, rc)
            targets.append(read)
            placed.append(one)
    # beyond 64 bases the last base is not kept: those two are one allele, the modal one, and it is truncated
    got, _ = check(native, block, targets, placed, normalize=False, fraction=(0, 1))
    ins = got["insertions"]
    assert sorted(set(ins["length"].tolist())) == [1, 31, 32, 33, 63, 64, 65, 70]
    assert ins["truncated"].tolist() == [int(n > 64) for n in ins["length"].tolist()] and got["consensus"]["truncated_skipped"] == 1
    assert (ins["count"] >= 2).all() and int(ins["count"].sum()) == len(placed) == int(ins["ins_total"][0])
    for rec in ins[ins["length"] == 33]:
        assert len(native.insertion_bases(rec)) == 33
    check(native, block, targets, placed, normalize=True)


@pytest.mark.parametrize("events", (4095, 4096, 4097, 5000, 25000))
def test_many_events_on_few_positions(native, events):
    """the sort and the scans of the allele table across their tile seams; 5000: three alleles on one position with an
    exact tie, which goes to the first in table order"""
    rng = random.Random(events)
    block = dna(rng, 64)
    words = (b"GA", b"GT", b"C")
    reads = [stretch_of(block, 10, [(7, EQ), (len(w), I, w), (8, EQ)], rng) for w in words]
    targets = [r for r, _ in reads]
    if events == 5000:
        plan = [0] * 2000 + [1] * 2000 + [2] * 1000
        starts = [10] * events
    else:
        plan = [rng.randrange(3) for _ in range(events)]
        starts = [rng.randrange(8, 14) for _ in range(events)]
    rng.shuffle(plan)
    placed = [place(k, 0, starts[j], 0, reads[k][1], targets[k]) for j, k in enumerate(plan)]
    got, seen = check(native, block, targets, placed, normalize=False, fraction=(1, 3))
    assert len(seen) == events and int(got["insertions"]["count"].sum()) == events
    if events == 5000:
        assert got["insertions"]["count"].tolist() == [1000, 2000, 2000] and got["consensus"]["records"][0][17:19] == b"GA"


@pytest.mark.parametrize("B", (4095, 4096, 4097))
def test_consensus_shapes_and_rules(native, B):
    """a record wholly deleted, a consensus longer and one shorter than the block, the scans of the output lengths
    across their tiles, low in both modes with min_depth on either side of the depth, and the three fractions"""
    rng = random.Random(B)
    first, gone = dna(rng, B - 40 - 2), dna(rng, 12)
    last = dna(rng, B - len(first) - len(gone) - 2)
    block = first + b"\x01" + gone + b"N" + last
    assert len(block) == B
    s2, s3 = len(first) + 1, len(first) + len(gone) + 2
    targets, placed = [b"A"], []
    for _ in range(3):
        placed.append(place(0, 0, s2, 0, [(len(gone), D)], b"A"))           # nothing of the second record is left
    long_ops, short_ops = [], []
    for k in range(30):
        long_ops += [(20, EQ), (5, I, dna(rng, 5))]
        short_ops += [(20, EQ), (3, D)]
    for ops, r_start in ((long_ops + [(10, EQ)], 100), (short_ops + [(10, EQ)], 1200), ([(len(last) - 1, EQ), (1, X)], s3)):
        for rc in (False, True, False):
            read, one = on_strand(len(targets), block, r_start, ops, rng, rc)
            targets.append(read)
            placed.append(one)
    # one more read over the first window with other bases: depth 4 there, majorities of 3
    targets.append(dna(rng, 200))
    placed.append(place(len(targets) - 1, 0, 100, 0, [(150, X)], targets[-1]))
    for fraction in ((0, 1), (1, 2), (1, 1)):
        for low in ("reference", "N"):
            for min_depth in (1, 3, 4, 5):
                got, _ = check(native, block, targets, placed, min_depth=min_depth, fraction=fraction, low=low)
                assert got["consensus"]["records"][1] == (b"" if min_depth <= 3 else (gone if low == "reference" else b"N" * len(gone)))
    got, _ = check(native, block, targets, placed)
    cons = got["consensus"]
    assert cons["deleted"] >= 90 + len(gone) and cons["inserted_bases"] == 150 and cons["starts"][-1] == sum(map(len, cons["records"])) + 2
    assert cons["starts"][s2 - 1] + 1 == cons["starts"][s2] == cons["starts"][s3 - 1] == cons["starts"][s3] - 1  # the separators


def test_no_alignment_at_all_is_the_block(native):
    rng = random.Random(11)
    block = dna(rng, 300) + b"\x01" + dna(rng, 200)
    for low in ("reference", "N"):
        got, events = check(native, block, [b"ACGT"], [], low=low)
        assert not events and not got["counts"].any() and len(got["insertions"]) == 0
        assert got["consensus"]["low_positions"] == 500 and got["consensus"]["starts"].tolist() == list(range(502))
        assert got["consensus"]["records"] == ([block[:300], block[301:]] if low == "reference" else [b"N" * 300, b"N" * 200])


@pytest.mark.parametrize("letters", (b"ACGT", b"AC", b"A"))
def test_random_alignments_over_two_records(native, letters):
    """few letters: nearly every gap can shift, by amounts the cases above do not plan"""
    rng = random.Random(17 + len(letters))
    first, second = dna(rng, 333, letters), dna(rng, 259, letters)
    block = first + b"N" + second
    targets = [dna(rng, rng.randrange(1, 200), letters) for _ in range(9)]
    placed = []
    while len(placed) < 400:
        t = rng.randrange(len(targets))
        ops = []
        for _ in range(rng.randrange(1, 12)):
            code = rng.choice((EQ, EQ, EQ, X, D, I))
            if not ops or ops[-1][1] != code:  # (neighbours of one code are merged in an align result)
                ops.append((rng.randrange(1, 9), code))
        tq = sum(n for n, code in ops if code != D)
        rq = sum(n for n, code in ops if code != I)
        lo, hi = rng.choice(((0, 333), (334, 334 + 259)))
        if tq > len(targets[t]) or rq == 0 or rq > hi - lo:
            continue
        placed.append(place(t, rng.randrange(0, len(targets[t]) - tq + 1), rng.randrange(lo, hi - rq + 1), rng.randrange(2), ops,
                            targets[t], primary=rng.randrange(2)))
    for normalize in (True, False):
        every, events = check(native, block, targets, placed, normalize=normalize)
        primary, fewer = check(native, block, targets, placed, primary_only=True, normalize=normalize, fraction=(1, 3))
        assert not every["counts"][333].any() and 0 < len(fewer) < len(events)
        assert int(every["counts"][:, pm.INS].sum()) == len(events) == int(every["insertions"]["count"].sum())
