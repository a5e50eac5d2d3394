"""Two independent models of the maximal repeats of the reference (nolzss_rlz_index_repeat_count / _repeats,
include/nolzss_hip.h).

  brute_repeats   (a) the definition itself: every substring of every record, its occurrences on both strands by
                  bytes.find scans (rlz_locate_model.brute_locate), the extension, mirror and palindrome rules applied
                  literally.  Blocks of a few hundred bases.
  RepeatsModel    (b) the array formulation the kernels run: X as the index lays it out, its suffix array and LCP array,
                  the left-context flags and their scan D, one representative rank per LCP interval, the count, the
                  left-diversity and the mirror rule from min / max SA over the interval.  Blocks up to about 2^16 bases.

Both return records as (position, length, count, record, palindrome), ascending by (position, length), and per record the
hits (position, record, is_rc), ascending by (position, is_rc)."""
import numpy as np

import rlz_locate_model as lm
import rlz_model as model


# ---- (a) the definition ------------------------------------------------------------------------------------------------
def _extensions(refs, starts, w, occ):
    """-> (right, left): the sets of extensions of the occurrences of w; an end mark is a tuple no base equals and no
    other end mark equals"""
    L = len(w)
    comp = {65: 84, 67: 71, 71: 67, 84: 65}
    right, left = set(), set()
    for position, record, is_rc in occ:
        r, s = refs[record], starts[record]
        at = position - s  # inside the record
        after = r[at + L] if at + L < len(r) else None   # Rblk[a + L], None: the record ends there
        before = r[at - 1] if at > 0 else None            # Rblk[a - 1], None: the record starts at a
        if not is_rc:
            right.add(after if after is not None else ("end", position, 0, "r"))
            left.add(before if before is not None else ("end", position, 0, "l"))
        else:
            right.add(comp[before] if before is not None else ("end", position, 1, "r"))
            left.add(comp[after] if after is not None else ("end", position, 1, "l"))
    return right, left


def is_maximal_repeat(refs, w, with_rc=True):
    """the three conditions of the definition"""
    refs = [bytes(r).upper() for r in refs]
    occ = lm.brute_locate(refs, w, with_rc)
    if len(occ) < 2:
        return False
    right, left = _extensions(refs, lm.record_starts(refs), w, occ)
    return len(right) > 1 and len(left) > 1


def brute_repeats(refs, with_rc=True, min_length=1, min_count=2):
    """-> [((position, length, count, record, palindrome), hits)] by the definition"""
    assert min_length >= 1 and min_count >= 2
    refs = [bytes(r).upper() for r in refs]
    starts = lm.record_starts(refs)
    # a reported repeat has a forward occurrence: p(w) is finite, or p(rc(w)) would be smaller
    words = {r[a:b] for r in refs for a in range(len(r)) for b in range(a + min_length, len(r) + 1)}
    out = []
    for w in words:
        occ = lm.brute_locate(refs, w, with_rc)
        if len(occ) < 2:
            continue
        right, left = _extensions(refs, starts, w, occ)
        if len(right) < 2 or len(left) < 2:
            continue
        if len(occ) < min_count:
            continue
        palindrome = 0
        if with_rc:
            mirror = lm.brute_locate(refs, model.revcomp(w), True)
            assert sorted((p, r, 1 - s) for p, r, s in mirror) == occ  # Occ(rc(w)) is Occ(w) with the strands flipped
            inf = float("inf")
            p_w = min((p for p, _, s in occ if s == 0), default=inf)
            p_rc = min((p for p, _, s in mirror if s == 0), default=inf)
            if not p_w <= p_rc:
                continue
            assert (p_w == p_rc) == (w == model.revcomp(w))
            if p_w == p_rc:
                palindrome = 1
                if len(occ) < 4:
                    continue
        position, record = min((p, r) for p, r, s in occ if s == 0)
        out.append(((position, len(w), len(occ), record, palindrome), occ))
    return sorted(out)


# ---- (b) the arrays ----------------------------------------------------------------------------------------------------
def sa_lcp(X):
    """suffix array and LCP array (n + 1 entries, lcp[0] = lcp[n] = 0) of a string whose sentinels are unique, by prefix
    doubling: the order of rlz_model.python_sa_lcp without its quadratic memory"""
    n = len(X)
    x = np.frombuffer(bytes(X), dtype=np.uint8).astype(np.int64)
    rank, k = x.copy(), 1
    while True:
        second = np.zeros(n, dtype=np.int64)
        if k < n:  # (0: the suffix ends before its second half begins)
            second[:n - k] = rank[k:] + 1
        key = rank * (max(n, 256) + 2) + second  # (the first ranks are byte values)
        sa = np.argsort(key, kind="stable")
        ks = key[sa]
        rank = np.zeros(n, dtype=np.int64)
        rank[sa] = np.cumsum(np.concatenate(([0], (ks[1:] != ks[:-1]).astype(np.int64))))
        if n == 0 or int(rank.max()) == n - 1:
            break
        k *= 2
    sa_l, rank_l, lcp, h = sa.tolist(), rank.tolist(), [0] * (n + 1), 0
    for i in range(n):  # Kasai
        r = rank_l[i]
        if r == 0:
            h = 0
            continue
        j = sa_l[r - 1]
        while i + h < n and j + h < n and X[i + h] == X[j + h]:
            h += 1
        lcp[r] = h
        if h:
            h -= 1
    return sa.astype(np.int64), np.array(lcp, dtype=np.int64)


def _previous(values, strict):
    """out[r] = the largest q < r with values[q] < values[r] (strict) or <= values[r]; -1 without one"""
    out, stack = [-1] * len(values), []
    for r, v in enumerate(values):
        while stack and (values[stack[-1]] >= v if strict else values[stack[-1]] > v):
            stack.pop()
        out[r] = stack[-1] if stack else -1
        stack.append(r)
    return out


def _next_smaller(values):
    """out[r] = the smallest q > r with values[q] < values[r]; len(values) without one"""
    n = len(values)
    out, stack = [n] * n, []
    for r in range(n - 1, -1, -1):
        v = values[r]
        while stack and values[stack[-1]] >= v:
            stack.pop()
        out[r] = stack[-1] if stack else n
        stack.append(r)
    return out


class RepeatsModel:
    def __init__(self, refs, with_rc=True):
        refs = [bytes(r).upper() for r in refs]
        lay = model.layout(refs, [], with_rc)
        assert not lay["pad"]
        self.refs, self.with_rc, self.m = refs, with_rc, len(refs)
        self.X, self.B = lay["S"], lay["block_length"]
        self.n = len(self.X)
        self.starts = np.array(lm.record_starts(refs), dtype=np.uint64)
        self.sa, self.lcp = sa_lcp(self.X)
        x = np.frombuffer(self.X, dtype=np.uint8)
        base = np.isin(x, np.frombuffer(b"ACGT", dtype=np.uint8))
        # term[a] = the index of the next terminator at or behind a
        self.term = np.concatenate(([0], np.cumsum(~base)))[:self.n]
        # stage 1: the symbol in front of every suffix in rank order (-1: position 0 or a terminator), diff and its scan D
        before = self.sa - 1
        left = np.where((before >= 0) & base[np.maximum(before, 0)], x[np.maximum(before, 0)].astype(np.int64), -1)
        diff = np.ones(self.n, dtype=np.int64)
        diff[1:] = ~((left[1:] >= 0) & (left[1:] == left[:-1]))
        self.diff, self.D = diff, np.cumsum(diff)
        values = self.lcp.tolist()
        self.prev_lt, self.prev_le, self.next_lt = _previous(values, True), _previous(values, False), _next_smaller(values)

    def intervals(self, min_length=1, min_count=2):
        """stage 2 -> [(lo, hi, length, position, palindrome)] of the reported repeats, by representative rank"""
        assert min_length >= 1 and min_count >= 2
        out, B = [], self.B
        for r in np.flatnonzero(self.lcp[:self.n] >= min_length).tolist():
            if r == 0:
                continue
            l = int(self.lcp[r])
            lo, hi = self.prev_lt[r], self.next_lt[r] - 1
            if self.prev_le[r] != lo:  # not the leftmost rank of (lo, hi] whose LCP is l
                continue
            if hi - lo + 1 < min_count:
                continue
            if self.D[hi] - self.D[lo] == 0:
                continue
            members = self.sa[lo:hi + 1]
            pmin, pmax, palindrome = int(members.min()), int(members.max()), 0
            if self.with_rc:
                if pmin > B:
                    continue
                if pmax > B:
                    mirror = 2 * B - pmax - l + 1
                    if pmin > mirror:
                        continue
                    if pmin == mirror:
                        if hi - lo + 1 < 4:
                            continue
                        palindrome = 1
            out.append((lo, hi, l, pmin, palindrome))
        return out

    def repeat_count(self, min_length=1, min_count=2):
        return len(self.intervals(min_length, min_count))

    def hits_of(self, lo, hi, l):
        """the members of [lo, hi] as (position, record, is_rc) arrays, ascending by (position, is_rc)"""
        a = self.sa[lo:hi + 1]
        rc = a > self.B
        position = np.where(rc, 2 * self.B - a - l + 1, a)
        k = self.term[a]
        record = np.where(rc, 2 * self.m - 1 - k, k)
        order = np.lexsort((rc, position))
        return position[order], record[order], rc[order]

    def repeats(self, min_length=1, min_count=2, max_hits=0):
        """-> the dict RlzIndex.repeats returns"""
        found = sorted(self.intervals(min_length, min_count), key=lambda t: (t[3], t[2]))
        keys = [(t[3], t[2]) for t in found]
        assert len(set(keys)) == len(keys), "the order key (position, length) is unique"
        position = np.array([t[3] for t in found], dtype=np.uint64)
        record = np.array([self.term[t[3]] for t in found], dtype=np.uint32)
        offsets, hp, hr, hs = [0], [], [], []
        for lo, hi, l, _, _ in found:
            if max_hits == 0 or hi - lo + 1 <= max_hits:
                p, r, s = self.hits_of(lo, hi, l)
                hp.append(p)
                hr.append(r)
                hs.append(s)
                offsets.append(offsets[-1] + len(p))
            else:
                offsets.append(offsets[-1])
        hit_position = np.concatenate(hp).astype(np.uint64) if hp else np.zeros(0, dtype=np.uint64)
        hit_record = np.concatenate(hr).astype(np.uint32) if hr else np.zeros(0, dtype=np.uint32)
        return {"position": position, "length": np.array([t[2] for t in found], dtype=np.uint64),
                "count": np.array([t[1] - t[0] + 1 for t in found], dtype=np.uint64), "record": record,
                "record_offset": position - self.starts[record] if len(found) else np.zeros(0, dtype=np.uint64),
                "palindrome": np.array([t[4] for t in found], dtype=bool), "offsets": np.array(offsets, dtype=np.uint64),
                "hit_position": hit_position, "hit_record": hit_record,
                "hit_record_offset": hit_position - self.starts[hit_record] if len(hit_position) else np.zeros(0, dtype=np.uint64),
                "hit_is_rc": np.concatenate(hs).astype(bool) if hs else np.zeros(0, dtype=bool)}

    def records(self, min_length=1, min_count=2):
        """-> [((position, length, count, record, palindrome), hits)] as brute_repeats lays them out"""
        out = []
        for lo, hi, l, position, palindrome in self.intervals(min_length, min_count):
            p, r, s = self.hits_of(lo, hi, l)
            hits = list(zip(p.tolist(), r.tolist(), s.astype(int).tolist()))
            out.append(((position, l, hi - lo + 1, int(self.term[position]), palindrome), hits))
        return sorted(out)
