"""The group-sort rounds of the suffix-array construction (group_sort.hpp: group_dir_kernel, group_sort_kernel as window
rounds and as pivot rounds) in plain numpy -- TEST INFRASTRUCTURE ONLY.  Three things:

  * (a) the definition (Text.compare): the order and the LCP of two suffixes under the rules of text.hpp, symbol by symbol;
  * (b) a round-level model of what the kernels are documented to do (model): per group the segments, their depths, the
    scan, the windows with their terminator words, the pivot keys, the budget, the cap and the reach -- it gives the
    exact sa, out_lo, lcp_list and min_depth that nolzss_debug_group_sort must return; `bug` switches one named mistake
    on, so that tests/test_group_sort_model_host.py can show which input is there for which mistake;
  * the inputs (CASES): texts, h0, which groups are listed and in which order, the input order inside the groups.

Everything works on symbols (dense codes, one per array element), never on packed words: where the kernels shift, mask
and count leading zeros, the model compares symbol arrays.
"""
import functools
from collections import namedtuple

import numpy as np

SMALL, MID0, MID, MAX = 64, 128, 256, 1024   # kGroupSortSmall, kGroupSortMid0, kGroupSortMid, kGroupSortMax
SCAN_WORDS, ROUNDS, PIVOT_WORDS = 8, 24, 32  # kScanWords, kGroupSortRounds, kPivotWords
PENDING = 0xffffffff                         # kLcpPending
COMPARED = PENDING - 1                       # kLcpPendingCompared
NONE = 0xffffffff                            # min_depth: nothing reported
PAD = 1200                                   # zero symbols behind the text (the packed text is padded too)
ACGT = (65, 67, 71, 84)
ORDERS = ("text", "reversed", "shuffle")
BUGS = ("mask_more", "mask_fewer", "no_tt", "no_term_index", "lcp_no_valid", "no_second_word", "scan_no_limit",
        "scan_no_stop", "unstable", "above_ascending", "no_sym_tiebreak", "lcp_wrong_neighbour", "cap_gt", "take_1025",
        "mark_at_g", "no_capped_depth")


# ---- the text as pack_text sees it, and (a) the definition -----------------------------------------------------------------
class Text:
    """bytes -> dense codes, bits per symbol and terminator table, decided as pack_text decides them"""

    def __init__(self, data):
        self.data = bytes(data)
        b = np.frombuffer(self.data, dtype=np.uint8)
        self.n = n = b.size
        present = np.bincount(b, minlength=256)
        distinct = np.nonzero(present)[0]
        self.bits = 2 if distinct.size <= 4 else (4 if distinct.size <= 16 else 8)
        others = [c for c in distinct if c not in ACGT]
        self.segmented = (1 <= len(others) <= 250 and any(c in ACGT for c in distinct) and
                          all(present[c] == 1 for c in others))
        lut = np.zeros(256, dtype=np.uint8)
        if self.segmented:  # nucleotides at 2 bits, the once-only bytes are terminators (packed as code 0)
            self.bits = 2
            lut[list(ACGT)] = [0, 1, 2, 3]
            terms = np.nonzero(np.isin(b, others))[0]
        else:
            lut[distinct] = np.arange(distinct.size)
            terms = np.zeros(0, dtype=np.int64)
        self.per = 64 // self.bits  # symbols per 64-bit word
        self.terms = np.concatenate([terms, [n]]).astype(np.int64)
        self.codes = np.concatenate([lut[b], np.zeros(PAD, dtype=np.uint8)])
        p = np.arange(n)
        self.term = np.searchsorted(self.terms, p, side="left")  # index of the next terminator of every suffix ...
        self.lim = self.terms[self.term] - p                     # ... and the symbols in front of it
        self.enc = (self.codes[:n] + 1).tobytes()

    def compare(self, a, b):
        """(a): -> (-1 | +1, lcp).  The comparison runs to the nearer terminator; the suffix that reaches one first is the
        smaller, at equal distance the one with the lower terminator index, and the LCP is then the limit."""
        la, lb = int(self.lim[a]), int(self.lim[b])
        limit, enc = min(la, lb), self.enc
        i, step = 0, 64
        while i < limit:
            j = min(i + step, limit)
            if enc[a + i:a + j] != enc[b + i:b + j]:
                while j - i > 8:  # (the first difference lies in [i, j): halve)
                    mid = (i + j) // 2
                    i, j = (i, mid) if enc[a + i:a + mid] != enc[b + i:b + mid] else (mid, j)
                while enc[a + i] == enc[b + i]:
                    i += 1
                return (-1 if enc[a + i] < enc[b + i] else 1), i
            i, step = j, step * 2
        if la != lb:
            return (-1 if la < lb else 1), limit
        return (-1 if self.term[a] < self.term[b] else 1), limit

    def lcp(self, a, b):
        return self.compare(a, b)[1]

    @functools.lru_cache(maxsize=None)
    def groups(self, h0):
        """the suffixes with at least h0 symbols in front of their terminator, grouped by those symbols: a list of
        ascending position arrays, in the order of the symbols; singletons included"""
        p = np.nonzero(self.lim >= h0)[0]
        rows = self.codes[p[:, None] + np.arange(h0)]
        _, inv = np.unique(rows, axis=0, return_inverse=True)
        order = np.argsort(inv.ravel(), kind="stable")
        cuts = np.nonzero(np.diff(inv.ravel()[order]))[0] + 1
        return [g for g in np.split(p[order], cuts)]


# ---- the case builder ---------------------------------------------------------------------------------------------------------
Listed = namedtuple("Listed", "sa slot grp")


def check_precondition(text, h0, groups):
    """what the hook cannot check: the members of a group agree on h0 symbols and none ends in front of h0"""
    for g in groups:
        g = np.asarray(g, dtype=np.int64)
        if g.size < 2 or np.unique(g).size != g.size:
            raise ValueError("a group of fewer than two distinct suffixes")
        if (text.lim[g] < h0).any():
            raise ValueError("a member ends in front of h0")
        rows = text.codes[g[:, None] + np.arange(h0)]
        if (rows != rows[0]).any():
            raise ValueError("the members of a group do not agree on h0 symbols")


def lay_out(text, h0, groups, order="text", gap=1, seed=0):
    """groups (arrays of suffix starts) -> sa with the groups on consecutive slots, `gap` finished slots in front of each
    where suffixes are left for them, and the active list (slot, grp) in slot order"""
    check_precondition(text, h0, groups)
    rng = np.random.default_rng(seed)
    used = np.zeros(text.n, dtype=bool)
    for g in groups:
        if used[g].any():
            raise ValueError("a suffix in two groups")
        used[g] = True
    rest = list(np.nonzero(~used)[0][::-1])
    sa, slot, grp = [], [], []
    for g in groups:
        g = np.sort(np.asarray(g, dtype=np.int64))
        g = g[::-1] if order == "reversed" else (rng.permutation(g) if order == "shuffle" else g)
        for _ in range(min(gap, len(rest))):
            sa.append(rest.pop())
        slot += range(len(sa), len(sa) + g.size)
        grp += [len(sa)] * g.size
        sa += g.tolist()
    sa += rest[::-1]
    return Listed(np.array(sa, dtype=np.uint32), np.array(slot, dtype=np.uint32), np.array(grp, dtype=np.uint32))


# ---- (b) the round-level model ---------------------------------------------------------------------------------------------
def _first_diff(codes, pa, pb, start, end):
    """per pair the first h in [start, end) with codes[pa + h] != codes[pb + h], else end"""
    h = start.astype(np.int64).copy()
    res = end.astype(np.int64).copy()
    live = np.nonzero(h < end)[0]
    off = np.arange(64)
    while live.size:
        x = codes[(pa[live] + h[live])[:, None] + off]
        y = codes[(pb[live] + h[live])[:, None] + off]
        ne = x != y
        found = ne.any(axis=1)
        cand = h[live] + np.where(found, ne.argmax(axis=1), 64)
        done = found | (cand >= end[live])
        res[live[done]] = np.minimum(cand[done], end[live[done]])
        h[live] = cand
        live = live[~done]
    return res


def _pack(w):
    """symbols (rows of one word) -> one unsigned integer per row that orders like the row"""
    bits = 64 // w.shape[1]
    return np.bitwise_or.reduce(w.astype(np.uint64) << (np.arange(w.shape[1] - 1, -1, -1) * bits).astype(np.uint64), axis=1)


def form_of(size):
    return "tiled" if size <= SMALL else "m128" if size <= MID0 else "m256" if size <= MID else "m1024" if size <= MAX else "none"


def model(text, listed, h0, pivot=False, max_rounds=ROUNDS, depth_cap=NONE, lcp_mark=None, bug=None):
    """-> {"sa", "out_lo", "lcp_list", "min_depth"} as the hook must return them, and what ran: "forms" (taken groups by
    form), "tied" (members left in classes of more than one), "rounds" (rounds in which something was still tied)"""
    assert bug is None or bug in BUGS
    codes, per = text.codes, text.per
    sa = listed.sa.astype(np.int64)
    slot, grp = listed.slot.astype(np.int64), listed.grp.astype(np.int64)
    m = slot.size
    out = {"sa": listed.sa.copy(), "out_lo": np.zeros(m, dtype=np.uint32), "lcp_list": np.full(m, PENDING, dtype=np.uint32),
           "min_depth": NONE, "forms": {}, "tied": 0, "rounds": 0}
    if m == 0:
        return out
    # ---- reach: which groups are taken at all
    first = np.nonzero(np.concatenate([[True], grp[1:] != grp[:-1]]))[0]
    size = np.diff(np.concatenate([first, [m]]))
    gid = np.repeat(np.arange(first.size), size)
    gstart = first[gid]
    passes = np.ones(first.size, dtype=bool)
    if lcp_mark is not None:  # the equalising round: the boundary behind the group's first member still holds the pending code
        passes = np.asarray(lcp_mark, dtype=np.int64)[grp[first] + (0 if bug == "mark_at_g" else 1)] == PENDING
    reach = MAX + 1 if bug == "take_1025" else MAX
    min_depth = NONE
    if (passes & (size > reach)).any():  # beyond the kernels' reach: untouched, tied on what the caller says
        min_depth = min(min_depth, h0)
    taken_g = passes & (size <= reach)
    for s in size[taken_g]:
        out["forms"][form_of(s)] = out["forms"].get(form_of(s), 0) + 1
    taken = taken_g[gid]
    # ---- state by sorted position (= list position)
    P = sa[slot]                       # the member at this position
    L, K = text.lim[P], text.term[P]   # its symbols in front of its terminator, and the terminator's index
    seg = gstart.copy()                # first position of my segment
    act = taken.copy()                 # my segment has more than one member
    depth = np.full(m, h0, dtype=np.int64)   # symbols my segment agrees on
    scanit = np.zeros(m, dtype=bool)         # the last round did not split my segment
    head = np.ones(m + 1, dtype=bool)        # a segment starts here (what is not taken never moves)
    head[:m] = ~taken | (np.arange(m) == gstart)
    blcp = np.full(m, PENDING, dtype=np.int64)
    for rnd in range(max_rounds):
        A = np.nonzero(act)[0]
        if A.size == 0:
            break
        out["rounds"] = rnd + 1
        hs = seg[A]
        if pivot:
            D = depth[A]
            limit = np.minimum(L[A], L[hs])
            stop = np.minimum(D + PIVOT_WORDS * per, depth_cap)
            stop2 = np.minimum(limit, stop)
            h = _first_diff(codes, P[A], P[hs], D, stop2)
            found = (h < stop2) & (A != hs)
            ended = ~found & (limit <= stop) & (A != hs)
            la, lb = L[A], L[hs]
            side = np.ones(A.size, dtype=np.int64)       # the pivot and what equals it as far as compared
            lrel = np.zeros(A.size, dtype=np.int64)
            sym = np.zeros(A.size, dtype=np.int64)       # 0: the suffix ends, else 1 + my symbol at l
            tword = np.zeros(A.size, dtype=np.int64)     # terminator index + 1 of a suffix that ends at l
            mine, theirs = codes[P[A] + h].astype(np.int64), codes[P[hs] + h].astype(np.int64)
            side[found] = np.where(mine[found] < theirs[found], 0, 2)
            lrel[found] = (h - D)[found]
            sym[found] = mine[found] + 1
            e1 = ended & (la < lb)   # I end first: the smaller one
            e2 = ended & (la > lb)   # the pivot ends: I go on with a symbol of my own
            e3 = ended & (la == lb)  # both end here: the lower terminator index first
            side[e1], side[e2] = 0, 2
            side[e3] = np.where(K[A][e3] < K[hs][e3], 0, 2)
            lrel[ended] = (limit - D)[ended]
            sym[e2] = codes[P[A] + limit].astype(np.int64)[e2] + 1
            tword[e1 | e3] = K[A][e1 | e3] + 1
            if bug == "no_sym_tiebreak":
                sym[:] = 0
            lfield = np.where(side == 0, lrel, np.where(side == 2, (lrel if bug == "above_ascending" else 2047 - lrel), 0))
            key = (side << 52) | (lfield << 41) | (sym << 32) | tword  # (pivot_key; the side two bits further down)
            keys = (key,)
            lfin = np.where(side == 1, 1 << 40, lrel)    # (the pivot's class: every other class decides an LCP with it)
            agreed = np.where(side == 1, stop, D + lrel + 1)
        else:
            # 1. a segment the last round did not split scans ahead
            D = depth.copy()
            S = A[scanit[A] & (A != hs)]
            if S.size:
                lead = seg[S]
                stop = depth[S] + SCAN_WORDS * per
                lim2 = np.minimum(L[S], L[lead])
                end = stop if bug == "scan_no_limit" else (lim2 if bug == "scan_no_stop" else np.minimum(stop, lim2))
                hh = _first_diff(codes, P[S], P[lead], depth[S], end)
                D[np.unique(lead)] = 1 << 40
                np.minimum.at(D, lead, hh)
            D = D[hs]
            # 2. the window of two words at that depth, zero behind the terminator, and its terminator word
            tag = np.clip(L[A] - D, 0, 2 * per)
            # (mask_fewer keeps TWO symbols too many: the first is the terminator itself, which packs as code 0 like the mask)
            keep = tag + (2 if bug == "mask_fewer" else -1 if bug == "mask_more" else 0)
            keep = np.where(tag < 2 * per, np.clip(keep, 0, 2 * per), tag)
            W = codes[(P[A] + D)[:, None] + np.arange(2 * per)]
            W = np.where(np.arange(2 * per) < keep[:, None], W, 0).astype(np.uint8)
            if bug == "no_second_word":
                W[:, per:] = 0
            tt = (tag << 16) | np.where(tag < 2 * per, K[A] & 0xffff, 0)
            if bug == "no_tt":
                tt = np.zeros_like(tt)
            elif bug == "no_term_index":
                tt = tag << 16
            keys = (tt, _pack(W[:, per:]), _pack(W[:, :per]))
        # 3. every segment sorted stably by its keys
        tie = -np.arange(A.size) if bug == "unstable" else np.arange(A.size)
        perm = np.lexsort((tie,) + keys + (hs,))
        P[A], L[A], K[A] = P[A][perm], L[A][perm], K[A][perm]
        # 4. new boundaries inside the old segments, with their LCP
        inner = np.nonzero(A != hs)[0]  # (its predecessor lies in the same segment)
        if pivot:
            key, lfin, agreed = key[perm], lfin[perm], agreed[perm]
            differ = key[inner] != key[inner - 1]
            low = np.minimum(lfin[inner], lfin[inner - 1])
            if bug == "lcp_wrong_neighbour":
                low = np.where(lfin[inner] < (1 << 40), lfin[inner], lfin[inner - 1])
            new_lcp = D[inner] + low
        else:
            W, tt, tag = W[perm], tt[perm], tag[perm]
            ne = W[inner] != W[inner - 1]
            d = np.where(ne.any(axis=1), ne.argmax(axis=1), 2 * per)
            differ = ne.any(axis=1) | (tt[inner] != tt[inner - 1])
            valid = np.minimum(tag[inner], tag[inner - 1])
            new_lcp = D[inner] + (d if bug == "lcp_no_valid" else np.minimum(d, valid))
            agreed = D + 2 * per  # members that stay together agree on the whole window
        at = A[inner[differ]]
        head[at] = True
        blcp[at] = new_lcp[differ]
        split = np.zeros(m, dtype=bool)
        split[hs[inner[differ]]] = True
        # 5. the segments of the next round
        seg[A] = np.maximum.accumulate(np.where(head[A], A, -1))
        still = ~(head[A] & head[A + 1])
        depth[A] = agreed
        if pivot:  # a segment that agrees up to the cap stays tied: the doubling rounds start at its depth
            capped = still & ((agreed > depth_cap) if bug == "cap_gt" else (agreed >= depth_cap))
            if capped.any() and bug != "no_capped_depth":
                min_depth = min(min_depth, int(agreed[capped].min()))
            still &= ~capped
        else:
            scanit[A] = ~split[hs]
        act[A] = still
    if act.any():  # out of rounds: what is still tied agrees on the depth its segment has reached
        min_depth = min(min_depth, int(depth[act].min()))
    e = np.nonzero(taken)[0]
    out["sa"][slot[e]] = P[e]
    out["out_lo"][e] = seg[e] - gstart[e]
    out["lcp_list"][e] = np.where(e == gstart[e], 0, np.where(head[e], blcp[e], PENDING))
    out["min_depth"] = min_depth
    out["tied"] = int((taken & ~(head[:m] & head[1:])).sum())
    return out


# ---- texts ---------------------------------------------------------------------------------------------------------------------
A2 = b"ACGT"
A4 = b"abcdefghijklmnop"              # 16 distinct bytes: 4 bits
A8 = bytes(range(32, 232))            # 200: 8 bits (nucleotides among them, but the other bytes occur more than once)
ALPHA = {2: A2, 4: A4, 8: A8}
TERM_BYTES = bytes(c for c in range(1, 256) if c not in ACGT)[:250]


def _rand(rng, alpha, length):
    return bytes(np.frombuffer(alpha, dtype=np.uint8)[rng.integers(0, len(alpha), length)])


def _digits(alpha, value, length):
    out = []
    for _ in range(length):
        out.append(alpha[value % len(alpha)])
        value //= len(alpha)
    return bytes(out)


def copies_text(seed, bits, fams, tail=None):
    """families (copies, head length): every family is a random head repeated `copies` times, each copy followed by the
    digits of a number of its own and by 0 .. 3 random symbols -- so the suffixes at one offset of the head form a group
    of `copies` members at every alignment, tied to the end of the head.  The whole alphabet stands at the end."""
    rng = np.random.default_rng(seed)
    alpha = ALPHA[bits]
    parts = []
    for copies, head_len in fams:
        head = _rand(rng, alpha, head_len)
        nd = 1
        while len(alpha) ** nd < copies:
            nd += 1
        for c in rng.permutation(copies):
            parts.append(head + _digits(alpha, int(c), nd) + _rand(rng, alpha, int(rng.integers(0, 4))))
    return b"".join(parts) + (tail if tail is not None else alpha)


def deep_text(seed, bits, h0):
    """a pair and a triple tied PIVOT_WORDS words and two symbols beyond h0 at offset 0 of their head -- so the groups at
    the offsets of the head have their first difference at every depth from h0 to there: every residue of position + depth,
    both halves of a word, the second word of a window, the edges of window, scan and pivot round.  The first differing
    symbols of the pair are code 0 against the highest bit of the code, those of the triple's last two code 0 against 1;
    the third member of the triple leaves half way.  position + depth is one value per copy, so short pairs follow whose
    first differing symbol stands at every residue of the text position modulo the symbols per word."""
    rng = np.random.default_rng(seed)
    alpha = ALPHA[bits]
    per = 64 // bits
    body = PIVOT_WORDS * per + 2 + h0
    top = alpha[1 << (bits - 1)]
    pair, triple = _rand(rng, alpha, body), _rand(rng, alpha, body)
    half = triple[:body // 2] + bytes([alpha[(alpha.index(triple[body // 2]) + 1) % len(alpha)]])
    junk = lambda: _rand(rng, alpha, int(rng.integers(5, 9)))  # noqa: E731
    out = b"".join([junk(), pair, alpha[:1], junk(), triple, alpha[:1], junk(), pair, bytes([top]), junk(), half, junk(),
                    triple, alpha[1:2], junk()])
    for r in range(2 * per):
        head = _rand(rng, alpha, h0 + 3)
        for last in (alpha[:1], alpha[-1:]):
            out += _rand(rng, alpha, 1 + (r + 1 - len(out) - len(head)) % per) + head + last
    return out + alpha


def mutated_text(seed, bits, k, length, rate=0.03, hotspots=0):
    """k copies of one random sequence, each with point mutations of its own (a collection of similar genomes); at
    `hotspots` places every copy carries a random symbol: equal l, different symbols"""
    rng = np.random.default_rng(seed)
    alpha = np.frombuffer(ALPHA[bits], dtype=np.uint8)
    base = rng.integers(0, alpha.size, length)
    spots = rng.choice(length, hotspots, replace=False) if hotspots else np.zeros(0, dtype=np.int64)
    parts = []
    for _ in range(k):
        c = base.copy()
        hit = rng.random(length) < rate
        c[hit] = (c[hit] + rng.integers(1, alpha.size, int(hit.sum()))) % alpha.size
        c[spots] = rng.integers(0, alpha.size, spots.size)
        parts.append(bytes(alpha[c]))
    return b"".join(parts) + bytes(alpha)


def periodic_text(seed, k, length):
    """exact copies back to back: every group stays tied as deep as anybody looks, down to the end of the text"""
    return _rand(np.random.default_rng(seed), A2, length) * k


def terminator_text(seed, nterms, h0):
    """nterms segments (the last ends with the text).  A core U of h0 symbols and two words is cut off behind h0 + j symbols
    in segment after segment, j = 0 .. 2 words and back: members that end inside the window at every length, one exactly
    at h0.  Some segments go on with code-0 symbols where others end; two pairs of segments are equal from U on (the same
    distance to different terminators), one of them deeper than a window, with equal symbols behind both terminators;
    the text ends inside a truncated U."""
    rng = np.random.default_rng(seed)
    core = _rand(rng, A2, h0 + 66)
    cuts = [5, 64, 0, 9, 33, 1, 63, 32, 31, 65, 2] + list(range(3, 66))
    bodies = []
    for s in range(nterms):
        j = cuts[s % len(cuts)]
        body = _rand(rng, b"CGT", int(rng.integers(1, 5))) + core[:h0 + j]
        if s % 7 == 3:
            body += b"A" * 70 + _rand(rng, b"CGT", 3)   # goes on with code-0 symbols where others end
        bodies.append(body)
    if nterms >= 3:
        bodies[1] = b"G" + core[:h0 + 9]       # ends at the distance of the last segment, at another terminator
    if nterms >= 5:
        twin = _rand(rng, A2, 2) + core[:h0 + 60] + _rand(rng, A2, 30)
        bodies[2], bodies[3] = b"T" + twin, b"C" + twin   # equal for more than a window; behind both terminators: "GT"
        bodies[4] = b"GT" + bodies[4]
    bodies[-1] = b"GT" + _rand(rng, b"CGT", 2) + core[:h0 + 9]
    out = b""
    for s, body in enumerate(bodies):
        out += body + (TERM_BYTES[s:s + 1] if s + 1 < nterms else b"")
    return out


def cap_edge_text(h0):
    """pivot R = V A ..., x = V C <terminator>, y = V C G T ...: x and y leave R at |V| with the same symbol and x ends one
    symbol later -- with depth_cap = |V| + 1 they stay one class at the cap"""
    v = _rand(np.random.default_rng(5), A2, h0 + 6)
    return b"GG" + v + b"A" + b"CCGGTTAACC" + b"\x01" + b"TG" + v + b"C" + b"\x02" + b"CT" + v + b"C" + b"GTTGCA"


# ---- cases ---------------------------------------------------------------------------------------------------------------------
# layout: ("sizes", [s, ...]) one unused group of each size, in this order | ("range", lo, hi) every group of lo .. hi members,
# in the order of the symbols | ("top", c) the c largest groups of at most MAX members | ("offsets", positions) the groups of the
# suffixes at the given positions.  runs: (pivot, max_rounds, depth_cap - h0 or None, marked) -- marked: with an lcp_mark --, in
# every input order of the case; extra: more of them, in text order only.
Case = namedtuple("Case", "name text h0 layout orders runs gap extra")
WIN, PV = False, True
BOTH = ((WIN, ROUNDS, None, False), (PV, ROUNDS, None, False))
MID_SIZES = [2, 3, 63, 64, 65, 127, 128, 129, 255, 256, 257]
BIG_SIZES = [1023, 1024, 1025]
H0 = {2: 14, 4: 7, 8: 5}


@functools.lru_cache(maxsize=None)
def text_of(name):
    kind, _, arg = name.partition(":")
    bits = int(arg) if arg.isdigit() else 2
    if kind == "sizes":
        return Text(copies_text(11 + bits, bits, [(k, H0[bits] + 3) for k in MID_SIZES + [2, 2, 40]]))
    if kind == "big":
        return Text(copies_text(21 + bits, bits, [(k, H0[bits] + 1) for k in BIG_SIZES]))
    if kind == "tiles":
        return Text(copies_text(31, 2, [(k, 15) for k in (63, 2, 64, 61, 3, 100, 2, 40)]))
    if kind == "queues":
        return Text(copies_text(41, 8, [(k, 5 + 169) for k in range(65, 71)]))
    if kind == "deep":
        return Text(deep_text(51 + bits, bits, H0[bits]))
    if kind == "verydeep":
        rng = np.random.default_rng(61 + bits)
        body = _rand(rng, ALPHA[bits], 8200)
        return Text(body + ALPHA[bits][:1] + body[:150] + ALPHA[bits][1:2] + body + ALPHA[bits][2:3] + ALPHA[bits])
    if kind == "terms":
        return Text(terminator_text(71, bits, 14))  # (bits: the entries of the table)
    if kind == "mutated":
        k = bits
        return Text(mutated_text(81, 2, k, {5: 400, 17: 300, 65: 200, 300: 120, 1024: 70}[k]))
    if kind == "hotspots":
        return Text(mutated_text(91 + bits, bits, 17, 300, rate=0.01, hotspots=12))
    if kind == "periodic":
        return Text(periodic_text(95, 20, 300))
    if kind == "capedge":
        return Text(cap_edge_text(14))
    raise KeyError(name)


def _cases():
    out = []
    add = lambda *a, orders=("text",), runs=BOTH, gap=1, extra=(): out.append(Case(*a, orders, runs, gap, extra))  # noqa: E731
    for bits in (2, 4, 8):
        h0, per = H0[bits], 64 // bits
        # group sizes, each alone and all in one list with singleton gaps, in the three input orders
        for s in MID_SIZES:
            add(f"size_{s}_w{bits}", f"sizes:{bits}", h0, ("sizes", [s]))
        add(f"sizes_w{bits}", f"sizes:{bits}", h0, ("sizes", MID_SIZES), orders=ORDERS)
        for s in BIG_SIZES:
            add(f"size_{s}_w{bits}", f"big:{bits}", h0, ("sizes", [s]))
        add(f"big_w{bits}", f"big:{bits}", h0, ("sizes", BIG_SIZES), orders=ORDERS)
        # every depth of the first difference from h0 to a pivot round and two symbols; caps on, around and below it;
        # budgets of one and two rounds (window rounds reach 2 and 2 + 8 + 2 words)
        caps = (0, -3, 1, 37, 4 * per, PIVOT_WORDS * per, PIVOT_WORDS * per + 1)
        add(f"deep_w{bits}", f"deep:{bits}", h0, ("range", 2, 3), orders=ORDERS,
            extra=tuple((PV, ROUNDS, c, False) for c in caps) +
            ((WIN, 1, None, False), (WIN, 2, None, False), (PV, 1, None, False), (PV, 2, 40 * per, False)))
    # a tie deeper than 24 rounds of scan and window reach, in a group of two and in a group of three
    for bits in (2, 8):
        add(f"verydeep_w{bits}", f"verydeep:{bits}", H0[bits], ("offsets", (0, 1, 2, 200, 201, 202)), runs=((WIN, ROUNDS, None, False), (WIN, 2, None, False)))
    # the tiled form: groups that start at places 0, 63, 1, 1, 62 of a tile and run into the next one, a small group
    # right behind a large one, a last tile of fewer than 128 positions
    add("tiles", "tiles", 14, ("sizes", [63, 2, 64, 61, 3, 100, 2, 40]), orders=ORDERS, gap=0)
    # queues: several workgroups of group_dir_kernel per shard, more items in a shard than gridDim.y; no large group at all
    add("queues", "queues", 5, ("range", 65, 70), gap=0)
    add("small_only", "sizes:2", 14, ("range", 2, 64))
    # the equalising form: marked and unmarked groups of every size, a reduced budget
    add("equalise", "sizes:2", 14, ("sizes", MID_SIZES + [2, 40]), orders=ORDERS, runs=((WIN, 3, None, True), (WIN, 1, None, True)))
    add("equalise_big", "big:2", 14, ("sizes", BIG_SIZES), runs=((WIN, 2, None, True),))
    # terminators: tables of 2 .. 4 entries (in the kernel arguments), 5, 33, 251
    for c in (2, 3, 4, 5, 33, 251):
        add(f"terms_{c}", f"terms:{c}", 14, ("range", 2, MAX), orders=ORDERS if c in (4, 251) else ("text",))
    # pivot collections: k mutated copies; equal l with different symbols; exact copies; the class that ends at the cap
    for k in (5, 17, 65, 300, 1024):
        add(f"mutated_{k}", f"mutated:{k}", 14, ("top", 3 if k >= 300 else 40), orders=ORDERS, runs=BOTH + ((PV, ROUNDS, 100, False),))
    for bits in (4, 8):
        add(f"hotspots_w{bits}", f"hotspots:{bits}", H0[bits], ("top", 40), orders=ORDERS, runs=BOTH)
    add("periodic", "periodic", 14, ("top", 12), orders=ORDERS, runs=((PV, ROUNDS, 1000, False), (PV, 3, 5000, False), (WIN, 4, None, False)))
    add("capedge", "capedge", 14, ("offsets", (2,)), runs=((PV, ROUNDS, 7, False), (PV, ROUNDS, 8, False), (PV, ROUNDS, 6, False)))
    return out


CASES = {c.name: c for c in _cases()}


@functools.lru_cache(maxsize=None)
def chosen_groups(name):
    """the groups a case lists, by its layout"""
    case = CASES[name]
    text = text_of(case.text)
    pool = [g for g in text.groups(case.h0) if g.size >= 2]
    kind = case.layout[0]
    if kind == "sizes":
        out, used = [], set()
        for s in case.layout[1]:
            k = next(i for i, g in enumerate(pool) if g.size == s and i not in used)
            used.add(k)
            out.append(pool[k])
        return out
    if kind == "range":
        return [g for g in pool if case.layout[1] <= g.size <= case.layout[2]]
    if kind == "top":
        fit = [g for g in pool if g.size <= MAX]
        keep = sorted(sorted(range(len(fit)), key=lambda i: -fit[i].size)[:case.layout[1]])
        return [fit[i] for i in keep]
    if kind == "offsets":
        want = set(case.layout[1])
        return [g for g in pool if want & set(g.tolist())]
    raise KeyError(kind)


@functools.lru_cache(maxsize=None)
def listed(name, order):
    case = CASES[name]
    return lay_out(text_of(case.text), case.h0, chosen_groups(name), order, case.gap, seed=len(name))


@functools.lru_cache(maxsize=None)
def mark_for(name, order):
    """the equalising round's filter: every other group (and so small and large ones alike) counts as compared; the entry
    AT the head slot holds a decided LCP, as in the construction"""
    lst, text = listed(name, order), text_of(CASES[name].text)
    mark = np.arange(text.n, dtype=np.uint32) % 7
    heads = np.unique(lst.grp)
    mark[heads[0::2] + 1] = PENDING
    mark[heads[1::2] + 1] = COMPARED
    mark.setflags(write=False)
    return mark


def runs_of(name):
    """every (order, pivot, max_rounds, depth_cap, marked) a case is run with; marked: with mark_for(name, order)"""
    case = CASES[name]
    for order in case.orders:
        for pivot, max_rounds, cap, marked in case.runs + (case.extra if order == "text" else ()):
            depth_cap = NONE if cap is None else case.h0 + cap
            yield order, pivot, max_rounds, depth_cap, marked


@functools.lru_cache(maxsize=None)
def expected(name, order, pivot, max_rounds, depth_cap, marked, bug=None):
    """the model's answer for one run of a case: computed once, shared by the tests, not to be written to"""
    case = CASES[name]
    mark = mark_for(name, order) if marked else None
    got = model(text_of(case.text), listed(name, order), case.h0, pivot, max_rounds, depth_cap, mark, bug)
    for v in got.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return got
