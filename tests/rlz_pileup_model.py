"""Model of the pileup counts and variant sites of the relative-LZ index (nolzss_rlz_pileup_*, include/nolzss_hip.h).

  pileup     the B x 8 counters of a list of alignments, by the walk the header states, one column at a time
  variants   the records a variants query reports over such counters
  records    the alignment records of an align result (the dict RlzIndex.align returns, or its model) as dicts
  planted_sample  a reference, error-free reads of a sample with planted edits, and the planted substitutions

Sequential, plain Python integers, no difference arrays and no prefix sums: nothing here is shared with the kernels."""
import numpy as np

I, D, EQ, X = 1, 2, 7, 8
A, C, G, T, DEL, INS, REV, BREAK = range(8)
CHANNELS = ("A", "C", "G", "T", "DEL", "INS", "REV", "BREAK")
CODE = {65: 0, 67: 1, 71: 2, 84: 3}  # A, C, G, T
COMP = bytes.maketrans(b"ACGT", b"TGCA")
VARIANT_FIELDS = ("position", "record_offset", "record", "ref_base", "allele", "count", "depth", "rev")


def records(result):
    """an align result (dict of arrays) -> a list of dicts, one per alignment"""
    keys = ("target", "t_start", "t_end", "r_start", "r_end", "is_rc", "primary")
    return [{k: int(result[k][c]) for k in keys} for c in range(len(result["target"]))]


def pileup(B, alignments, ops, op_offsets, targets, block, primary_only):
    """alignments: dicts with target, t_start, t_end, r_start, r_end, is_rc, primary; ops (length << 4 | code) and
    op_offsets as align returns them; targets: the batch's sequences; block: B bytes, the records joined by one
    separator byte each -> (B, 8) uint32"""
    counts = [[0] * 8 for _ in range(B)]
    block = bytes(block).upper()
    assert len(block) == B
    for c, a in enumerate(alignments):
        if primary_only and not a["primary"]:
            continue
        rc = bool(a["is_rc"])
        target = bytes(targets[a["target"]]).upper()
        mine = [int(o) for o in ops[int(op_offsets[c]):int(op_offsets[c + 1])]]
        # the target stretch in forward-block orientation: reversed and complemented on the reverse strand, where the ops
        # are read last to first
        stretch = target[a["t_start"]:a["t_end"]]
        if rc:
            stretch = stretch.translate(COMP)[::-1]
            mine = mine[::-1]
        r_start, r_end = a["r_start"], a["r_end"]
        r, q = r_start, 0
        for op in mine:
            n, code = op >> 4, op & 15
            if code == I:
                counts[min(max(r - 1, r_start), r_end - 1)][INS] += 1
                q += n
                continue
            for _ in range(n):
                assert r_start <= r < r_end
                if code == EQ:
                    counts[r][CODE[block[r]]] += 1
                elif code == X:
                    counts[r][CODE[stretch[q]]] += 1
                else:
                    assert code == D
                    counts[r][DEL] += 1
                if rc:
                    counts[r][REV] += 1
                r += 1
                if code != D:
                    q += 1
        assert r == r_end and q == len(stretch), "the ops do not consume both stretches"
        before = a["t_end"] < len(target) if rc else a["t_start"] > 0
        after = a["t_start"] > 0 if rc else a["t_end"] < len(target)
        if before:
            counts[r_start][BREAK] += 1
        if after:
            counts[r_end - 1][BREAK] += 1
    return np.array(counts, dtype=np.uint32).reshape(B, 8)


def variants(counts, block, record_starts, min_count, num, den):
    """counts: (B, 8); block: B bytes; record_starts: the first position of every record in the block, ascending ->
    a list of tuples in the order of VARIANT_FIELDS, ascending by (position, allele)"""
    assert den >= 1 and 0 <= num <= den and min_count >= 1
    block = bytes(block).upper()
    out = []
    for p in range(len(block)):
        if block[p] not in CODE:
            continue
        b = CODE[block[p]]
        row = [int(v) for v in counts[p]]
        depth = row[A] + row[C] + row[G] + row[T] + row[DEL]
        record = max(k for k, s in enumerate(record_starts) if s <= p)
        for allele in (A, C, G, T, DEL, INS):
            if allele == b:
                continue
            if row[allele] >= min_count and row[allele] * den >= num * depth:
                out.append((p, p - int(record_starts[record]), record, b, allele, row[allele], depth, row[REV]))
    return out


# ---- the seeded sample of the end-to-end test ------------------------------------------------------------------------
def planted_sample(rng, length=4000, read=100, step=4):
    """-> (reference: one record of `length` bases; reads: error-free pieces of `read` bases of a sample at every
    `step`-th offset, alternating strands; substitutions: [(position in the reference, allele code)]).  The sample is a
    copy of the reference with 5 substitutions, one deletion of 3 bases and one insertion of 2, each edit at least 50
    bases from every other and 200 from either end."""
    ref = bytes(rng.choice(b"ACGT") for _ in range(length))
    spots = []
    while len(spots) < 7:
        p = rng.randrange(200, length - 200)
        if all(abs(p - o) >= 50 for o in spots):
            spots.append(p)
    sample, substitutions = bytearray(ref), []
    for k, p in sorted(enumerate(spots), key=lambda kp: -kp[1]):  # from the back: earlier positions stay put
        if k == 5:
            del sample[p:p + 3]
        elif k == 6:
            sample[p:p] = bytes(rng.choice(b"ACGT") for _ in range(2))
        else:
            base = rng.choice([c for c in b"ACGT" if c != ref[p]])
            sample[p] = base
            substitutions.append((p, CODE[base]))
    sample = bytes(sample)
    reads = []
    for j, lo in enumerate(range(0, len(sample) - read + 1, step)):
        piece = sample[lo:lo + read]
        reads.append(piece.translate(COMP)[::-1] if j % 2 else piece)
    return ref, reads, sorted(substitutions)
