"""Model of the cohort of samples over the block of a relative-LZ index (nolzss_rlz_cohort_*, include/nolzss_hip.h).

  calls_from_counts   the letter of every block position under the consensus' call rule, from (B, 8) pileup counters
  calls_from_bytes    ... from one byte per position
  infos               called, low, deleted, differs of such a sample
  distances           the two N x N matrices
  sites               the records of a sites query
  columns             the N x S letters at a list of positions
  planted_cohort      one reference, five samples with SNPs planted on a small tree, a deletion, a stretch without reads

A sample here is a bytes of B letters: A, C, G, T for a call, N for none (and, where the statistics need them, `-` for
a DEL call and `.` for a separator, which the read-outs turn into N).  Sequential, plain Python integers and bytes: no
bit planes, no popcounts, nothing shared with the kernels."""
from rlz_pileup_model import CODE, COMP

LETTERS = b"ACGT"
SITE_FIELDS = ("position", "record_offset", "record", "present", "counts", "reference")


def raw_calls_from_counts(counts, block, min_depth, num, den):
    """-> bytes of B symbols: a letter (call), `-` (DEL call), `n` (LOW), `.` (separator)"""
    block = bytes(block).upper()
    out = bytearray()
    for p in range(len(block)):
        if block[p] not in CODE:
            out.append(ord("."))
            continue
        b = CODE[block[p]]
        row = [int(v) for v in counts[p][:5]]
        depth, most = sum(row), max(row)
        if depth < min_depth or most * den < num * depth:
            out.append(ord("n"))
            continue
        call = b if row[b] == most else row.index(most)
        out.append(ord("-") if call == 4 else LETTERS[call])
    return bytes(out)


def raw_calls_from_bytes(data, block):
    block, data = bytes(block).upper(), bytes(data)
    assert len(data) == len(block)
    out = bytearray()
    for p in range(len(block)):
        if block[p] not in CODE:
            out.append(ord("."))
        else:
            c = bytes([data[p]]).upper()[0]
            out.append(c if c in CODE else ord("n"))
    return bytes(out)


def letters(raw):
    """what calls() and columns() read back: N wherever there is no base call"""
    return bytes(c if c in CODE else ord("N") for c in raw)


def calls_from_counts(counts, block, min_depth, num, den):
    return letters(raw_calls_from_counts(counts, block, min_depth, num, den))


def calls_from_bytes(data, block):
    return letters(raw_calls_from_bytes(data, block))


def infos(raw, block):
    block = bytes(block).upper()
    out = dict(called=0, low=0, deleted=0, differs=0)
    for p, c in enumerate(raw):
        if c in CODE:
            out["called"] += 1
            out["differs"] += int(c != block[p])
        elif c == ord("-"):
            out["deleted"] += 1
        elif c == ord("n"):
            out["low"] += 1
    return out


def distances(calls):
    """calls: N bytes of letters (N: no call) -> (differences, compared) as lists of lists"""
    n = len(calls)
    diff = [[0] * n for _ in range(n)]
    comp = [[0] * n for _ in range(n)]
    for i in range(n):
        for j in range(i, n):
            for a, b in zip(calls[i], calls[j]):
                if a in CODE and b in CODE:
                    comp[i][j] += 1
                    diff[i][j] += int(a != b)
            comp[j][i], diff[j][i] = comp[i][j], diff[i][j]  # (both counts are symmetric by their definition)
    return diff, comp


def record_starts(block):
    block = bytes(block).upper()
    return [0] + [p + 1 for p in range(len(block)) if block[p] not in CODE]


def sites(calls, block, starts, min_present, with_reference):
    """-> the records as tuples in the order of SITE_FIELDS (counts: a 4-tuple; reference: the block's code)"""
    block = bytes(block).upper()
    out = []
    for p in range(len(block)):
        if block[p] not in CODE:
            continue
        counts = [0, 0, 0, 0]
        for s in calls:
            if s[p] in CODE:
                counts[CODE[s[p]]] += 1
        present = sum(counts)
        seen = {k for k in range(4) if counts[k]}
        if with_reference:
            seen.add(CODE[block[p]])
        if len(seen) >= 2 and present >= min_present:
            record = max(k for k, s in enumerate(starts) if s <= p)
            out.append((p, p - starts[record], record, present, tuple(counts), CODE[block[p]]))
    return out


def columns(calls, positions):
    """-> N bytes of S letters"""
    return [bytes(s[p] for p in positions) for s in calls]


# ---- the planted cohort -------------------------------------------------------------------------------------------------
TREE = {"all": (0, 1, 2, 3, 4), "left": (0, 1), "right": (2, 3), "p0": (0,), "p1": (1,), "p2": (2,), "p3": (3,), "p4": (4,)}
SPOTS_PER_BRANCH = {"all": 2, "left": 3, "right": 3, "p0": 2, "p1": 1, "p2": 2, "p3": 2, "p4": 3}
DELETION_SAMPLE, DELETION_LENGTH = 1, 3
GAP_SAMPLE, GAP_LENGTH = 3, 150


def planted_cohort(rng, length=3000, samples=5, read=100, step=10):
    """One random reference and `samples` samples of it.  SNPs are planted on the branches of TREE (a branch's SNPs go to
    all its samples: some are shared, some private; those of `all` agree on a base that is not the reference's).  Sample
    DELETION_SAMPLE lacks DELETION_LENGTH bases; sample GAP_SAMPLE has no read over GAP_LENGTH bases, one of its private
    SNPs among them.  Reads are `read` bases, every `step` bases, alternating strands.
    -> dict(reference, sequences, reads: per sample, snps: per sample {position: letter}, deletion: (sample, position,
    length), gap: (sample, lo, hi) in block positions, truth: per sample the letters the reads can show -- the sample's
    base, N inside the deletion and the gap --, differences: the planted Hamming distances over positions called in
    both)"""
    ref = bytes(rng.choice(b"ACGT") for _ in range(length))
    spots = []
    while len(spots) < sum(SPOTS_PER_BRANCH.values()) + 1:
        p = rng.randrange(200, length - 200 - GAP_LENGTH)
        if all(abs(p - o) >= 50 for o in spots):
            spots.append(p)
    deletion_at = spots.pop()
    snps = [dict() for _ in range(samples)]
    for branch in sorted(TREE):
        for _ in range(SPOTS_PER_BRANCH[branch]):
            p = spots.pop()
            base = rng.choice([c for c in b"ACGT" if c != ref[p]])
            for s in TREE[branch]:
                snps[s][p] = base
    # the stretch without reads of GAP_SAMPLE lies over one of its private SNPs, which no read then shows
    hidden = sorted(p for p in snps[GAP_SAMPLE] if all(p not in snps[s] for s in range(samples) if s != GAP_SAMPLE))[0]
    want = (hidden - 20, hidden - 20 + GAP_LENGTH)
    gap = None
    sequences, reads, truth = [], [], []
    for s in range(samples):
        seq = bytearray(ref)
        for p, base in snps[s].items():
            seq[p] = base
        shown = bytearray(seq)
        if s == DELETION_SAMPLE:
            shown[deletion_at:deletion_at + DELETION_LENGTH] = b"N" * DELETION_LENGTH
            del seq[deletion_at:deletion_at + DELETION_LENGTH]
        seq = bytes(seq)
        mine, covered = [], bytearray(len(seq))
        for j, lo in enumerate(list(range(0, len(seq) - read, step)) + [len(seq) - read]):
            if s == GAP_SAMPLE and lo < want[1] and lo + read > want[0]:
                continue
            piece = seq[lo:lo + read]
            covered[lo:lo + read] = b"\1" * read
            mine.append(piece.translate(COMP)[::-1] if j % 2 else piece)
        if s == GAP_SAMPLE:  # (no deletion in this sample: sequence and block positions agree)
            bare = [p for p in range(len(seq)) if not covered[p]]
            gap = (s, bare[0], bare[-1] + 1)
            assert bare == list(range(gap[1], gap[2])) and gap[1] <= hidden < gap[2]
            shown[gap[1]:gap[2]] = b"N" * len(bare)
        else:
            assert all(covered)
        sequences.append(seq)
        reads.append(mine)
        truth.append(bytes(shown))
    differences = [[sum(1 for a, b in zip(truth[i], truth[j]) if a != b and a != ord("N") and b != ord("N"))
                    for j in range(samples)] for i in range(samples)]
    return dict(reference=ref, sequences=sequences, reads=reads, snps=snps, deletion=(DELETION_SAMPLE, deletion_at, DELETION_LENGTH),
                gap=gap, truth=truth, differences=differences)
