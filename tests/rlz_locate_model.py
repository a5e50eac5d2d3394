"""Models of the pattern queries on the relative-LZ index (nolzss_rlz_index_count / _locate, include/nolzss_hip.h).

  brute_locate    the definition itself: bytes.find per reference record for P, and for rc(P) when the index has the
                  reverse complement
  LocateModel     the interval formulation the kernels run, in plain Python over IndexModel: the insertion rank q of the
                  pattern, the common prefix with its right neighbour, I(m) around q, and the coordinate and record of
                  every suffix in it
  case / patterns the seeded generator both the CPU and the GPU tests draw from

A hit is (position, record, is_rc); the hits of a pattern ascend by (position, is_rc).  Small inputs only."""
import rlz_index_model as index_model
import rlz_model as model


def record_starts(refs):
    """the first position of every record in Rblk = R1 s R2 s .. Rm"""
    out, at = [], 0
    for r in refs:
        out.append(at)
        at += len(r) + 1
    return out


def brute_locate(refs, pattern, with_rc=True):
    """-> sorted [(position, record, is_rc)] by the definition"""
    p = bytes(pattern).upper()
    if not p:
        return []
    hits = []
    for record, (start, r) in enumerate(zip(record_starts(refs), refs)):
        r = bytes(r).upper()
        for is_rc, needle in ((0, p), (1, model.revcomp(p)))[:2 if with_rc else 1]:
            at = r.find(needle)
            while at >= 0:
                hits.append((start + at, record, is_rc))
                at = r.find(needle, at + 1)
    return sorted(hits)


class LocateModel(index_model.IndexModel):
    def __init__(self, refs, with_rc=True):
        super().__init__(refs, with_rc)
        self.m = len(refs)
        # term[a] = the index of the next terminator at or behind a: the separators of X in order, then its end
        self.term, k = [0] * (len(self.X) + 1), 0
        for a in range(len(self.X)):
            self.term[a] = k
            if self.X[a] not in b"ACGT":
                k += 1
        self.term[len(self.X)] = k

    def interval(self, pattern):
        """-> (lo, count): the ranks [lo, lo + count) whose suffixes start with the pattern; (0, 0) without one"""
        p = bytes(pattern).upper()
        m = len(p)
        if m == 0:
            return 0, 0
        lo, hi = 0, len(self.sa)
        while lo < hi:
            mid = (lo + hi) // 2
            if self.compare(self.sa[mid], p, 0)[0]:
                lo = mid + 1
            else:
                hi = mid
        q = lo
        if q > 0:  # the left neighbour is smaller than the pattern: it can never carry all of it
            assert self.compare(self.sa[q - 1], p, 0)[1] < m
        if q == len(self.sa) or self.compare(self.sa[q], p, 0)[1] != m:
            return 0, 0
        lo = hi = q
        while self.lcp[lo] >= m:
            lo -= 1
        while self.lcp[hi + 1] >= m:
            hi += 1
        assert lo == q  # the insertion rank is the lower end of the interval
        return lo, hi - lo + 1

    def hit(self, a, m):
        """suffix a of X that starts with a pattern of m bases -> (position, record, is_rc)"""
        k = self.term[a]
        if a < self.B:
            return a, k, 0
        assert self.with_rc and a > self.B
        return 2 * self.B - a - m + 1, 2 * self.m - 1 - k, 1

    def count(self, pattern):
        return self.interval(pattern)[1]

    def locate(self, pattern):
        lo, count = self.interval(pattern)
        return sorted(self.hit(self.sa[r], len(pattern)) for r in range(lo, lo + count))


# ---- the seeded generator ----------------------------------------------------------------------------------------
ALPHABETS = (b"ACGT", b"AC", b"AT", b"A")


def _dna(rng, n, alphabet):
    return bytes(rng.choice(alphabet) for _ in range(n))


def case(rng, lo=0, hi=24, records=None):
    """-> refs: 1 to 5 records of lo .. hi bases over one of the alphabets, empty ones among them, never all; repeats of
    one record inside another so that patterns occur in several records"""
    alphabet = rng.choice(ALPHABETS)
    m = records or rng.randint(1, 5)
    refs = [b"" if rng.random() < 0.15 else _dna(rng, rng.randint(max(lo, 1), hi), alphabet) for _ in range(m)]
    if not any(refs):
        refs[rng.randrange(m)] = _dna(rng, rng.randint(max(lo, 1), hi), alphabet)
    for j in range(m):  # a piece of another record, or its reverse complement, copied in
        if refs[j] and rng.random() < 0.5:
            src = refs[rng.randrange(m)]
            if src:
                a = rng.randrange(len(src))
                piece = src[a:a + rng.randint(2, 10)]
                if rng.random() < 0.5:
                    piece = model.revcomp(piece)
                at = rng.randrange(len(refs[j]) + 1)
                refs[j] = refs[j][:at] + piece + refs[j][at:]
    return refs


def patterns(rng, refs, count, longest=12):
    """`count` patterns: cut from a record, reverse-complemented, extended by one base, random, spanning a record
    boundary, ending exactly at a record's end, self-reverse-complementary, and now and then empty or lower case"""
    full = [r for r in refs if r]
    alphabet = bytes(sorted(set(b"".join(full)))) or b"A"
    out = []
    for _ in range(count):
        kind = rng.random()
        r = rng.choice(full)
        a = rng.randrange(len(r))
        piece = r[a:a + rng.randint(1, longest)]
        if kind < 0.30:
            p = piece
        elif kind < 0.45:
            p = model.revcomp(piece)
        elif kind < 0.55:
            p = piece + bytes([rng.choice(b"ACGT")])
        elif kind < 0.65:
            p = _dna(rng, rng.randint(1, 6), alphabet)
        elif kind < 0.73:  # across a boundary: the end of one record and the start of another
            s = rng.choice(full)
            p = r[-rng.randint(1, 4):] + s[:rng.randint(1, 4)]
        elif kind < 0.85:  # ends exactly at the record's end
            p = r[-rng.randint(1, min(longest, len(r))):]
        elif kind < 0.97:  # its own reverse complement: w rc(w)
            w = piece[:rng.randint(1, 4)]
            p = w + model.revcomp(w)
        else:
            p = b""
        if rng.random() < 0.05:
            p = p.lower()
        out.append(p)
    return out
