"""Model of the normalised pileup walk, the insertion alleles and the consensus of the relative-LZ index
(nolzss_rlz_pileup_open_flags, _insertions, _consensus, include/nolzss_hip.h).

  walk       the B x 8 counters and the insertion events of a list of alignments, one op and one column at a time
  alleles    the distinct events with their multiplicities, in table order
  insertions the records an insertions query reports over such a table
  consensus  the text, the records, the map and the statistics of a consensus query
  planted_sample_with_truth   rlz_pileup_model.planted_sample, the same draws, and the sample itself

Sequential, plain Python integers and bytes; no difference arrays, no scans, no sort keys: nothing here is shared with
the kernels."""
import numpy as np

from rlz_pileup_model import A, BREAK, C, CODE, COMP, D, DEL, EQ, G, I, INS, REV, T, X

MAX_SHIFT = 1024
INS_BASES = 64
LETTERS = b"ACGT"
INSERTION_FIELDS = ("position", "record_offset", "record", "length", "count", "depth", "ins_total", "truncated", "bases")
STATS = ("called", "low_positions", "substitutions", "deleted", "insertions", "inserted_bases", "truncated_skipped")


def walk(block, alignments, ops, op_offsets, targets, primary_only, normalize):
    """-> ((B, 8) uint32 counters, events): an event is (position, n, the first 64 bases of the allele as bytes), one
    per I op of a kept alignment, in the order of the walk"""
    block = bytes(block).upper()
    B = len(block)
    counts = [[0] * 8 for _ in range(B)]
    events = []
    for c, a in enumerate(alignments):
        if primary_only and not a["primary"]:
            continue
        rc = bool(a["is_rc"])
        target = bytes(targets[a["target"]]).upper()
        mine = [(int(o) >> 4, int(o) & 15) for o in ops[int(op_offsets[c]):int(op_offsets[c + 1])]]
        stretch = target[a["t_start"]:a["t_end"]]
        if rc:
            stretch = stretch.translate(COMP)[::-1]
            mine = mine[::-1]
        r_start, r_end = a["r_start"], a["r_end"]
        # the values in front of every op, then its shift: each reads the block and the op's own target bases only
        at, r, q = [], r_start, 0
        for n, code in mine:
            at.append((r, q))
            r += 0 if code == I else n
            q += 0 if code == D else n
        assert r == r_end and q == len(stretch), "the ops do not consume both stretches"
        shift = [0] * len(mine)
        for k, (n, code) in enumerate(mine):
            if not normalize or code not in (D, I) or k == 0 or mine[k - 1][1] != EQ:
                continue
            limit, (rk, qk), s = min(mine[k - 1][0], MAX_SHIFT), at[k], 0
            if code == D:
                while s < limit and block[rk - (s + 1)] == block[rk + n - (s + 1)]:
                    s += 1
            else:
                word = stretch[qk:qk + n]
                while s < limit and block[rk - (s + 1)] == word[(n - (s + 1)) % n]:
                    s += 1
            shift[k] = s

        def column(p, channel):
            assert r_start <= p < r_end and block[p] in CODE
            counts[p][channel] += 1
            if rc:
                counts[p][REV] += 1

        for k, (n, code) in enumerate(mine):
            rk, qk = at[k]
            s = shift[k]
            if code == EQ:
                keep = n - (shift[k + 1] if k + 1 < len(mine) and mine[k + 1][1] == D else 0)
                for p in range(rk, rk + keep):
                    column(p, CODE[block[p]])
            elif code == X:
                for j in range(n):
                    column(rk + j, CODE[stretch[qk + j]])
            elif code == D:
                for p in range(rk - s, rk - s + n):
                    column(p, DEL)
                for p in range(rk - s + n, rk + n):  # the `=` columns that moved behind the gap
                    column(p, CODE[block[p]])
            else:
                assert code == I
                p = min(max(rk - s - 1, r_start), r_end - 1)
                counts[p][INS] += 1
                word = stretch[qk:qk + n]
                events.append((p, n, bytes(word[(i - s) % n] for i in range(min(n, INS_BASES)))))
        before = a["t_end"] < len(target) if rc else a["t_start"] > 0
        after = a["t_start"] > 0 if rc else a["t_end"] < len(target)
        if before:
            counts[r_start][BREAK] += 1
        if after:
            counts[r_end - 1][BREAK] += 1
    return np.array(counts, dtype=np.uint32).reshape(B, 8), events


def words_of(bases):
    """at most 64 bases -> the two words of big-endian 2-bit codes, zero behind the last base"""
    words = [0, 0]
    for j, b in enumerate(bases):
        words[j // 32] |= CODE[b] << (62 - 2 * (j % 32))
    return tuple(words)


def alleles(events):
    """-> [(position, n, (word0, word1), count)] ascending by (position, n, word0, word1): two events are one allele iff
    position, n and both words agree"""
    table = {}
    for p, n, bases in events:
        key = (p, n, words_of(bases))
        table[key] = table.get(key, 0) + 1
    return [key + (table[key],) for key in sorted(table)]


def depth_of(row):
    return int(row[A]) + int(row[C]) + int(row[G]) + int(row[T]) + int(row[DEL])


def insertions(table, counts, record_starts, min_count, num, den):
    """-> the records of an insertions query as tuples in the order of INSERTION_FIELDS (bases: the two words)"""
    out = []
    for p, n, words, count in table:
        depth = depth_of(counts[p])
        if count >= min_count and count * den >= num * depth:
            record = max(k for k, s in enumerate(record_starts) if s <= p)
            out.append((p, p - int(record_starts[record]), record, n, count, depth, int(counts[p][INS]), int(n > INS_BASES), words))
    return out


def bases_of(n, words):
    return bytes(LETTERS[(words[j // 32] >> (62 - 2 * (j % 32))) & 3] for j in range(min(n, INS_BASES)))


def consensus(counts, table, block, min_depth, num, den, low):
    """low: 0 keeps the block's base at a low position, 1 writes N -> dict(text, records, starts, and STATS)"""
    block = bytes(block).upper()
    out = {name: 0 for name in STATS}
    text, starts = bytearray(), []
    for p in range(len(block)):
        starts.append(len(text))
        if block[p] not in CODE:
            text.append(1)
            continue
        b = CODE[block[p]]
        row = [int(v) for v in counts[p][:5]]
        depth, most = sum(row), max(row)
        if depth < min_depth or most * den < num * depth:
            out["low_positions"] += 1
            text.append(ord("N") if low else block[p])
            continue
        out["called"] += 1
        call = b if row[b] == most else row.index(most)
        if call == DEL:
            out["deleted"] += 1
        else:
            text.append(LETTERS[call])
            out["substitutions"] += int(call != b)
        here = [entry for entry in table if entry[0] == p]
        if not here:
            continue
        modal = max(here, key=lambda entry: entry[3])  # (max returns the first of equal counts: table order)
        if modal[3] * den >= num * depth:
            if modal[1] > INS_BASES:
                out["truncated_skipped"] += 1
            else:
                text += bases_of(modal[1], modal[2])
                out["insertions"] += 1
                out["inserted_bases"] += modal[1]
    starts.append(len(text))
    records, piece = [], bytearray()
    for p in range(len(block)):  # cut where the block's separators were written, not at every 0x01 of the text
        if block[p] not in CODE:
            records.append(bytes(piece))
            piece = bytearray()
        else:
            piece += text[starts[p]:starts[p + 1]]
    records.append(bytes(piece))
    out.update(text=bytes(text), records=records, starts=starts)
    return out


def planted_sample_with_truth(rng, length=4000, read=100, step=4):
    """rlz_pileup_model.planted_sample with the same draws -> (reference, reads, substitutions, sample)"""
    ref = bytes(rng.choice(b"ACGT") for _ in range(length))
    spots = []
    while len(spots) < 7:
        p = rng.randrange(200, length - 200)
        if all(abs(p - o) >= 50 for o in spots):
            spots.append(p)
    sample, substitutions = bytearray(ref), []
    for k, p in sorted(enumerate(spots), key=lambda kp: -kp[1]):
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
    return ref, reads, sorted(substitutions), sample
