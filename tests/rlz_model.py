"""Models of the relative-LZ parse (nolzss_rlz_factorize, include/nolzss_hip.h): every target against the reference
block only.

  brute_parse      the definition itself: longest prefix of T[p:] that occurs in Rblk (bytes.find), forward wins ties,
                   leftmost occurrence, evaluated at chain positions only
  layout           the prepared string S = Rblk s T1 s .. Tk s [pad] rc-block s in Python
  array_codes /    the array formulation over (sa, lcp) of S with plain loops: nearest flagged rank above and below,
  array_records    codes into text order, the chain from B + 1, references from min / max SA over I(L)
"""
import numpy as np

RC_MASK = 1 << 63
LEN_MASK = 0x7fffffff
SEP = b"|"  # between the reference records of the brute force: matches nothing
_COMP = bytes.maketrans(b"ACGT", b"TGCA")
SENTINELS = [b for b in range(1, 256) if b not in b"ACGT"]


def revcomp(s: bytes) -> bytes:
    return s.translate(_COMP)[::-1]


def _longest(block: bytes, t: bytes, p: int, rc: bool) -> int:
    """largest L such that t[p:p+L] (rc: its reverse complement) occurs in block; occurrence is monotone in L"""
    lo, hi = 0, len(t) - p
    if hi and block.find(revcomp(t[p:p + 1]) if rc else t[p:p + 1]) < 0:
        return 0
    while lo < hi:
        mid = (lo + hi + 1) // 2
        piece = t[p:p + mid]
        if block.find(revcomp(piece) if rc else piece) >= 0:
            lo = mid
        else:
            hi = mid - 1
    return lo


def brute_parse(refs, target, with_rc=True):
    """-> [(start, length, ref, is_rc, is_literal)] with start relative to the target and ref a position in Rblk
    (0 for a literal)"""
    block = SEP.join(bytes(r).upper() for r in refs)
    t = bytes(target).upper()
    out, p = [], 0
    while p < len(t):
        lf = _longest(block, t, p, False)
        lr = _longest(block, t, p, True) if with_rc else 0
        if max(lf, lr) == 0:
            out.append((p, 1, 0, False, True))
            p += 1
        elif lf >= lr:
            out.append((p, lf, block.find(t[p:p + lf]), False, False))
            p += lf
        else:
            out.append((p, lr, block.find(revcomp(t[p:p + lr])), True, False))
            p += lr
    return out


def brute_codes(refs, target, with_rc=True):
    """the code of EVERY position of the target by the definition: length, bit 31 = reverse complement, 0 = literal"""
    block = SEP.join(bytes(r).upper() for r in refs)
    t = bytes(target).upper()
    code = np.zeros(len(t), dtype=np.uint32)
    n, lf, lr = len(t), 0, 0
    for p in range(n):
        # a match of length L at p leaves one of L - 1 at p + 1: the search goes on from there, one base at a time
        lf, lr = max(lf - 1, 0), max(lr - 1, 0)
        while p + lf < n and block.find(t[p:p + lf + 1]) >= 0:
            lf += 1
        while with_rc and p + lr < n and block.find(revcomp(t[p:p + lr + 1])) >= 0:
            lr += 1
        code[p] = lf if lf >= lr else (lr | (1 << 31))
    return code


def layout(refs, targets, with_rc=True):
    """-> dict(S, target_offsets, block_length, rc_block_start, rcN, chain_end, pad) as nolzss_rlz_prepare lays it out"""
    refs = [bytes(r).upper() for r in refs]
    targets = [bytes(t).upper() for t in targets]
    sent = iter(SENTINELS)
    S = bytearray()
    for i, r in enumerate(refs):
        if i:
            S.append(next(sent))
        S += r
    B = len(S)
    S.append(next(sent))
    offsets = []
    for t in targets:
        offsets.append(len(S))
        S += t
        S.append(next(sent))
    chain_end = len(S) - 1
    pad = False
    if with_rc:
        if (B - 1 + len(S)) % 2:
            S.append(next(sent))
            pad = True
        E = len(S)
        for r in reversed(refs):
            S += revcomp(r)
            S.append(next(sent))
        rcN = (B - 1 + E) // 2
    else:
        E, rcN = len(S), 0
    return {"S": bytes(S), "target_offsets": offsets, "block_length": B, "rc_block_start": E, "rcN": rcN,
            "chain_end": chain_end, "pad": pad}


def python_sa_lcp(S: bytes):
    """suffix array and LCP array (n + 1 entries, lcp[0] = lcp[n] = 0) by sorting: small inputs only.  The sentinels are
    unique, so no common prefix runs across one, whatever order they sort in."""
    n = len(S)
    sa = sorted(range(n), key=lambda i: S[i:])
    lcp = [0] * (n + 1)
    for r in range(1, n):
        a, b = sa[r - 1], sa[r]
        L = 0
        while a + L < n and b + L < n and S[a + L] == S[b + L]:
            L += 1
        lcp[r] = L
    return np.array(sa, dtype=np.uint32), np.array(lcp, dtype=np.uint32)


def _nearest_flagged_min(flag, lcp, m):
    """per rank: max over the two directions of the minimum LCP towards the nearest flagged rank (0 without one)"""
    best = [0] * m
    seen, cur = False, 0
    for r in range(m):  # min lcp[j + 1 .. r], j the nearest flagged rank below r
        if seen:
            cur = min(cur, lcp[r])
            best[r] = cur
        if flag[r]:
            seen, cur = True, 1 << 62
    seen, cur = False, 0
    for r in range(m - 1, -1, -1):  # min lcp[r + 1 .. j], j the nearest flagged rank above r
        if seen and cur > best[r]:
            best[r] = cur
        if flag[r]:
            seen, cur = True, lcp[r]
        elif seen:
            cur = min(cur, lcp[r])
    return best


def array_codes(sa, lcp, block_length, rc_block_start, with_rc):
    """-> code of every position of S (text order): length, bit 31 = reverse complement, 0 = no match"""
    m = len(sa)
    sa_l, lcp_l = [int(x) for x in sa], [int(x) for x in lcp]
    lf = _nearest_flagged_min([p < block_length for p in sa_l], lcp_l, m)
    lr = _nearest_flagged_min([p >= rc_block_start for p in sa_l], lcp_l, m) if with_rc else [0] * m
    code = np.zeros(m, dtype=np.uint32)
    for r in range(m):
        code[sa_l[r]] = lf[r] if lf[r] >= lr[r] else (lr[r] | (1 << 31))
    return code


def array_records(sa, lcp, code, block_length, chain_end, rcN):
    """the chain from block_length + 1 to chain_end over the codes -> absolute (start, length, ref) records, the
    sentinel literals between the targets included"""
    m = len(sa)
    sa_l, lcp_l = [int(x) for x in sa], [int(x) for x in lcp]
    isa = [0] * m
    for r, p in enumerate(sa_l):
        isa[p] = r
    out, p = [], block_length + 1
    while p < chain_end:
        c = int(code[p])
        L = c & LEN_MASK
        if L == 0:
            out.append((p, 1, p))
            p += 1
            continue
        lo = hi = isa[p]
        while lcp_l[lo] >= L:
            lo -= 1
        while hi + 1 < m and lcp_l[hi + 1] >= L:
            hi += 1
        if c >> 31:
            out.append((p, L, RC_MASK | (2 * rcN - max(sa_l[lo:hi + 1]) - L + 1)))
        else:
            out.append((p, L, min(sa_l[lo:hi + 1])))
        p += L
    return np.array(out, dtype=np.dtype([("start", "<u8"), ("length", "<u8"), ("ref", "<u8")]))


def records_of_target(records, offset, length):
    """the absolute records whose start lies inside one target"""
    keep = (records["start"] >= offset) & (records["start"] < offset + length)
    return records[keep]


def brute_absolute(refs, targets, with_rc=True):
    """brute_parse of every target in the absolute coordinates of the C ABI: one (start, length, ref) array per target;
    a literal has ref = start, a reverse-complement factor carries RC_MASK"""
    lay = layout(refs, targets, with_rc)
    res = []
    for t, off in zip(targets, lay["target_offsets"]):
        rows = [(off + s, L, off + s if lit else (ref | (RC_MASK if rc else 0))) for s, L, ref, rc, lit in
                brute_parse(refs, t, with_rc)]
        res.append(np.array(rows, dtype=np.dtype([("start", "<u8"), ("length", "<u8"), ("ref", "<u8")])))
    return res
