"""Models of the pattern queries inside the targets of a relative-LZ archive (nolzss_rlz_finder_*, include/nolzss_hip.h;
DESIGN.md 5, "Relative-LZ archive: locate through the parse").  Test infrastructure, like rlz_locate_model.py.

  brute_find      the definition itself over the plain target strings: a slice compare per position and strand
  primary_flags   the `primary` flag of occurrences from the archive's exported records
  expected        the dict RlzArchiveFinder.locate returns, from the two above
  intervals       the windows of the record starts merged into the intervals of the kernel text, in numpy
  kernel_text     K and its two tables from the intervals and the plain targets
"""
import numpy as np

_COMP = bytes.maketrans(b"ACGT", b"TGCA")


def revcomp(b: bytes) -> bytes:
    return bytes(b).translate(_COMP)[::-1]


def dna(rng, n, alphabet=b"ACGT"):
    return np.frombuffer(alphabet, dtype=np.uint8)[rng.integers(0, len(alphabet), n)].tobytes()


class Texts:
    """the plain targets laid out for the brute force: upper case, one 0 byte behind each, so that no slice compare of
    a pattern succeeds across two targets"""

    def __init__(self, targets):
        parts = [bytes(t).upper() for t in targets]
        self.cat = np.frombuffer(b"".join(x + b"\0" for x in parts), dtype=np.uint8)
        self.starts = np.cumsum([0] + [len(x) + 1 for x in parts]).astype(np.int64)


def _occurrences(text, p):
    """positions i with text[i : i + m] == p: every position is a candidate, and column by column of the slice compare
    the candidates that disagree are dropped"""
    m = len(p)
    if len(text) < m:
        return np.zeros(0, dtype=np.int64)
    cand = np.arange(len(text) - m + 1, dtype=np.int64)
    for c in range(m):
        cand = cand[text[cand + c] == p[c]]
        if len(cand) == 0:
            break
    return cand


def brute_find(targets, pattern, with_rc=True):
    """(n, 3) int64 rows (target, position, is_rc), ascending: target[position : position + m] == pattern (is_rc 0) or,
    with_rc, its reverse complement (is_rc 1).  An empty pattern occurs nowhere.  targets: byte strings, or a Texts."""
    texts = targets if isinstance(targets, Texts) else Texts(targets)
    p = bytes(pattern).upper()
    if len(p) == 0:
        return np.zeros((0, 3), dtype=np.int64)
    strands = [p] + ([revcomp(p)] if with_rc else [])
    found = [_occurrences(texts.cat, np.frombuffer(q, dtype=np.uint8)) for q in strands]
    at = np.concatenate(found)
    rc = np.concatenate([np.full(len(o), s, dtype=np.int64) for s, o in enumerate(found)])
    order = np.lexsort((rc, at))
    at, rc = at[order], rc[order]
    t = np.searchsorted(texts.starts, at, side="right") - 1
    return np.stack([t, at - texts.starts[t], rc], axis=1).astype(np.int64)


def decoded_records(records, block_length):
    """exported records (absolute start, length, ref) -> (decoded start, length, is_literal) arrays"""
    start = records["start"].astype(np.int64) - block_length
    return start, records["length"].astype(np.int64), records["ref"] == records["start"]


def primary_flags(records, block_length, bases, hits, m):
    """hits: (target, position, is_rc) rows; bases[t] = decoded position of target t.  An occurrence [p, p + m) is
    secondary iff it lies inside ONE copy record, else primary."""
    start, length, literal = decoded_records(records, block_length)
    hits = np.asarray(hits, dtype=np.int64).reshape(-1, 3)
    p = np.asarray(bases, dtype=np.int64)[hits[:, 0]] + hits[:, 1]
    k = np.searchsorted(start, p, side="right") - 1
    return literal[k] | (p + m > start[k] + length[k])


def expected(targets, records, block_length, patterns, with_rc=True, max_hits=0):
    """dict as RlzArchiveFinder.locate returns it"""
    bases = np.cumsum([0] + [len(t) for t in targets])
    arrays = Texts(targets)
    counts, offsets, rows, flags = [], [0], [np.zeros((0, 3), dtype=np.int64)], [np.zeros(0, dtype=bool)]
    for p in patterns:
        h = brute_find(arrays, p, with_rc)
        counts.append(len(h))
        if max_hits == 0 or len(h) <= max_hits:
            rows.append(h)
            flags.append(primary_flags(records, block_length, bases, h, len(p)))
        offsets.append(offsets[-1] + (len(h) if max_hits == 0 or len(h) <= max_hits else 0))
    rows, flags = np.concatenate(rows), np.concatenate(flags)
    return {"counts": np.array(counts, dtype=np.uint64), "offsets": np.array(offsets, dtype=np.uint64),
            "target": rows[:, 0].astype(np.uint64), "position": rows[:, 1].astype(np.uint64),
            "is_rc": rows[:, 2].astype(bool), "primary": flags.astype(bool)}


def intervals(record_starts, target_lengths, M):
    """decoded record starts (ascending) and the target lengths -> (dstart, dend) int64 arrays of the intervals: the
    window [max(tb, b - W), min(te, b + W)) of every record start b in target [tb, te), W = max(M - 1, 1), merged while
    windows overlap or touch; a new interval begins where a window starts behind the end of the previous one and at the
    first record of every target."""
    b = np.asarray(record_starts, dtype=np.int64)
    if len(b) == 0:
        return np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64)
    W = max(M - 1, 1)
    bases = np.cumsum([0] + [int(x) for x in target_lengths]).astype(np.int64)
    t = np.searchsorted(bases, b, side="right") - 1  # (an empty target repeats a base: the last one at or below b)
    tb, te = bases[t], bases[t + 1]
    ws, we = np.maximum(tb, b - W), np.minimum(te, b + W)
    opens = np.ones(len(b), dtype=bool)
    opens[1:] = (b[1:] == tb[1:]) | (ws[1:] > we[:-1])
    first = np.flatnonzero(opens)
    last = np.append(first[1:] - 1, len(b) - 1)
    return ws[first], we[last]


def kernel_text(targets, record_starts, M):
    """-> (K bytes, kstart, dstart) with intervals + 1 entries each, as nolzss_rlz_finder_kernel returns them"""
    lengths = [len(t) for t in targets]
    whole = b"".join(bytes(t).upper() for t in targets)
    ds, de = intervals(record_starts, lengths, M)
    K = b"".join(whole[s:e] for s, e in zip(ds, de))
    kstart = np.concatenate([[0], np.cumsum(de - ds)]).astype(np.uint64)
    dstart = np.append(ds, len(whole)).astype(np.uint64)
    return K, kstart, dstart


def mosaic(rng, refs, length, mutate=0.03, max_piece=60):
    """a target of about `length` bases cut from the references: forward and reverse-complement pieces of 1 .. max_piece
    bases, with point mutations"""
    out = bytearray()
    while len(out) < length:
        r = refs[int(rng.integers(0, len(refs)))]
        n = int(rng.integers(1, min(max_piece, len(r)) + 1))
        at = int(rng.integers(0, len(r) - n + 1))
        piece = r[at:at + n]
        out += revcomp(piece) if rng.integers(0, 2) else piece
    out = out[:length]
    for i in np.flatnonzero(rng.random(len(out)) < mutate):
        out[i] = b"ACGT"[int(rng.integers(0, 4))]
    return bytes(out)


def substrings(targets, lengths):
    """every distinct substring of every target with one of the lengths"""
    seen = set()
    for t in targets:
        t = bytes(t).upper()
        for m in lengths:
            for i in range(len(t) - m + 1):
                seen.add(t[i:i + m])
    return sorted(seen)
