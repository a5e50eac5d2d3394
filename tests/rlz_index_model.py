"""Model of the relative-LZ index (nolzss_rlz_index_*, include/nolzss_hip.h): a target suffix is placed among the sorted
suffixes of the index text X, the longest match is the larger common prefix with the two neighbours of the insertion
rank, and strand and reference come from min / max SA over the LCP interval I(L) around the neighbour.  Plain loops over
rlz_model.layout and rlz_model.python_sa_lcp: small inputs only."""
import rlz_model as model

RC_MASK = model.RC_MASK


class IndexModel:
    def __init__(self, refs, with_rc=True):
        lay = model.layout(refs, [], with_rc)  # X = the prepared string of the references and no target
        assert not lay["pad"]
        self.X, self.B, self.with_rc = lay["S"], lay["block_length"], with_rc
        sa, lcp = model.python_sa_lcp(self.X)
        self.sa, self.lcp = [int(x) for x in sa], [int(x) for x in lcp]
        self.seg = [0] * (len(self.X) + 1)  # bases before the next terminator
        for i in range(len(self.X) - 1, -1, -1):
            self.seg[i] = self.seg[i + 1] + 1 if self.X[i] in b"ACGT" else 0

    def compare(self, a, t, p):
        """-> (the X suffix at a is smaller than t[p:], their common prefix): compare up to the nearer terminator, the
        suffix that reaches its terminator first is the smaller one, the end of the target is the smallest terminator"""
        lx, rem = self.seg[a], len(t) - p
        limit, h = min(lx, rem), 0
        while h < limit and self.X[a + h] == t[p + h]:
            h += 1
        if h < limit:
            return self.X[a + h] < t[p + h], h
        return lx < rem, limit

    def match(self, t, p):
        """-> (L, is_rc, ref) of position p of the target t (upper case); L = 0: a literal"""
        lo, hi = 0, len(self.sa)  # the insertion rank: the X suffixes below it are the smaller ones
        while lo < hi:
            mid = (lo + hi) // 2
            if self.compare(self.sa[mid], t, p)[0]:
                lo = mid + 1
            else:
                hi = mid
        q = lo
        left = self.compare(self.sa[q - 1], t, p)[1] if q > 0 else 0
        right = self.compare(self.sa[q], t, p)[1] if q < len(self.sa) else 0
        L = max(left, right)
        if L == 0:
            return 0, False, 0
        lo = hi = q - 1 if left >= right else q
        while self.lcp[lo] >= L:
            lo -= 1
        while self.lcp[hi + 1] >= L:
            hi += 1
        occ = self.sa[lo:hi + 1]
        if min(occ) < self.B:
            return L, False, min(occ)
        return L, True, 2 * self.B - max(occ) - L + 1  # rcN = B

    def codes(self, target):
        t = bytes(target).upper()
        out = []
        for p in range(len(t)):
            L, rc, _ = self.match(t, p)
            out.append(L | (1 << 31) if rc else L)
        return out

    def parse(self, target):
        """-> [(start, length, ref, is_rc, is_literal)] as rlz_model.brute_parse"""
        t = bytes(target).upper()
        out, p = [], 0
        while p < len(t):
            L, rc, ref = self.match(t, p)
            if L == 0:
                out.append((p, 1, 0, False, True))
                p += 1
            else:
                out.append((p, L, ref, rc, False))
                p += L
        return out
