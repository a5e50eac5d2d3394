"""A plain numpy model of the 16-ary min / max pyramids (nolzss_amd/csrc/pyramid.hpp, pyramid.hip) and of the searches
built on them (nearest.hpp), with the inputs the tests run on them.  Test infrastructure, like rlz_locate_model.py.

Every query is defined on the base array alone, by a scan of a slice; nothing here walks levels.  The `*_many` helpers
answer a batch of queries with one sorted list of hit positions per threshold; test_pyramid_model_host.py pins them, and
the scalar definitions, to a pure-Python brute force.

The wrong-rule variants (keyword arguments that default to the right rule) exist for the CPU test alone: it shows, for
every input family below, that an implementation following the wrong rule would answer at least one of the family's
queries differently, i.e. that the inputs can see the mistake they are there for.
"""
from collections import namedtuple

import numpy as np

FAN = 16
MAX_LEVELS = 9
NONE = 0xffffffff          # nearest_left without a hit; "no position" of a search
FAR_CLEARED = 252          # nearest.hpp: ranks a search has passed before the far searches take over
OP_LEFT, OP_RIGHT, OP_RANGE = range(3)   # nolzss_hip.h: NOLZSS_PYR_*
(UP_LESS, UP_GREATER, DOWN_LESS, DOWN_GREATER, FAR_UP_LESS, FAR_UP_GREATER, FAR_DOWN_LESS, FAR_DOWN_GREATER,
 LCP_INTERVAL, LPNF_LEFTMOST, LPNF_SEARCH) = range(11)   # NOLZSS_NEAR_*

U32 = np.uint32


def identity(is_max):
    return 0 if is_max else 0xffffffff


def hit(v, x, is_max, strict=True):
    """v beats the threshold x: v < x in a min pyramid, v > x in a max pyramid (wrong rule: <= / >=)"""
    if strict:
        return v > x if is_max else v < x
    return v >= x if is_max else v <= x


# ---- the levels ------------------------------------------------------------------------------------------------------
def level_lengths(n):
    lens = [n]
    while lens[-1] > 1 and len(lens) < MAX_LEVELS:
        lens.append((lens[-1] + FAN - 1) // FAN)
    return lens


def levels(base, is_max, pad=None):
    """[level 0 = base, level 1, ...]: level k + 1 holds the min (max) of each aligned group of 16 entries of level k,
    the last group short.  Wrong rule (pad = the u32 the padding holds): the short group reduces the padding too."""
    out = [np.asarray(base, dtype=U32)]
    while len(out[-1]) > 1 and len(out) < MAX_LEVELS:
        cur = out[-1]
        m = (len(cur) + FAN - 1) // FAN
        ext = np.full(m * FAN, identity(is_max) if pad is None else pad, dtype=U32)
        ext[:len(cur)] = cur
        grouped = ext.reshape(m, FAN)
        out.append(grouped.max(axis=1) if is_max else grouped.min(axis=1))
    return out


def flag_word(base, flag_min):
    """the pending flag of the first level: 1 if some base entry is >= flag_min"""
    return int(bool((np.asarray(base, dtype=U32) >= flag_min).any()))


# ---- the three queries -----------------------------------------------------------------------------------------------
def nearest_left(base, r, x, is_max, strict=True):
    """the largest q in [0, r] whose entry beats x; NONE if there is none"""
    h = np.flatnonzero(hit(base[:r + 1], U32(x), is_max, strict))
    return int(h[-1]) if h.size else NONE


def nearest_right(base, r, x, is_max, strict=True, pad=None):
    """the smallest q in [r, len) whose entry beats x; len if there is none (r >= len included).

    Wrong rule (pad = the u32 the padding holds): entries at or beyond a level's length are not hidden.  On level 0 that
    cannot show (nor can it in nearest_left, which counts only entries at or below idx on the way up and descends only
    into blocks in front of the one it left, which are full): the first padding entry has index len, which is the answer for "none" anyway.  It shows one level up:
    a walk without a hit climbs through the block behind its own on every level until that block is the last one; where
    the last block is short, its first padding entry -- entry len[l] of level l -- beats x and is taken for a hit, and
    the descent from there ends at base index len[l] * 16^l or beyond."""
    n = len(base)
    if r >= n:
        return n
    h = np.flatnonzero(hit(base[r:], U32(x), is_max, strict))
    if h.size:
        return r + int(h[0])
    if pad is not None and hit(U32(pad), U32(x), is_max, strict):
        idx = r
        for l, ln in enumerate(level_lengths(n)):
            if idx >> 4 == (ln - 1) >> 4:      # the last block of level l
                return min(ln << (4 * l), 0xffffffff) if ln % FAN else n
            idx = (idx >> 4) + 1
    return n


def range_reduce(base, a, b, is_max, rule=None, pad=None):
    """min (max) of base[a .. b], a <= b.  Wrong rules: "a-1" and "b+1" take in the neighbour outside (b + 1 == len is
    the padding: pad, or nothing if pad is None), "excl_b" leaves b out."""
    lo, hi = a, b + 1
    src = np.asarray(base, dtype=U32)
    if rule == "a-1":
        lo = max(a - 1, 0)
    elif rule == "b+1":
        hi = b + 2
        if pad is not None:
            src = np.concatenate([src, np.array([pad], dtype=U32)])
    elif rule == "excl_b":
        hi = b
    part = src[lo:hi]
    if part.size == 0:
        return identity(is_max)
    return int(part.max() if is_max else part.min())


def answers(base, is_max, queries, strict=True, pad=None, rule=None):
    """the model's answer to every (op, a, b) row, one at a time from the definitions.  strict, pad, rule: a wrong-rule
    variant (strict: left and right; pad alone: right; rule, with or without pad: range)"""
    base = np.asarray(base, dtype=U32)
    out = np.zeros(len(queries), dtype=U32)
    for k, (op, a, b) in enumerate(np.asarray(queries).tolist()):
        if op == OP_LEFT:
            out[k] = nearest_left(base, a, b, is_max, strict)
        elif op == OP_RIGHT:
            out[k] = nearest_right(base, a, b, is_max, strict, pad=None if rule else pad)
        else:
            out[k] = range_reduce(base, a, b, is_max, rule=rule, pad=pad)
    return out


def answers_many(base, is_max, queries):
    """the same answers (right rules only) for long arrays and many queries: per threshold one sorted list of the hit
    positions and a binary search in it; ranges one slice each"""
    base = np.asarray(base, dtype=U32)
    q = np.asarray(queries, dtype=np.int64).reshape(-1, 3)
    n = len(base)
    out = np.zeros(len(q), dtype=U32)
    near = q[:, 0] != OP_RANGE
    for x in np.unique(q[near, 2]):
        H = np.flatnonzero(hit(base, U32(x), is_max))
        left = np.flatnonzero(near & (q[:, 2] == x) & (q[:, 0] == OP_LEFT))
        right = np.flatnonzero(near & (q[:, 2] == x) & (q[:, 0] == OP_RIGHT))
        if not H.size:
            out[left], out[right] = NONE, n
            continue
        at = np.searchsorted(H, q[left, 1], side="right") - 1
        out[left] = np.where(at >= 0, H[np.maximum(at, 0)], NONE)
        at = np.searchsorted(H, q[right, 1], side="left")
        out[right] = np.where(at < H.size, H[np.minimum(at, H.size - 1)], n)
    for k in np.flatnonzero(~near):
        part = base[q[k, 1]:q[k, 2] + 1]
        out[k] = part.max() if is_max else part.min()
    return out


# ---- the searches of nearest.hpp -----------------------------------------------------------------------------------
def search(sa, lcp, r, x, floor, up, greater, start=1, strict=True):
    """The nearest rank q in the direction, at distance `start` or more, whose suffix start qualifies (greater: sa[q] >
    x, else sa[q] < x), and m = the minimum of the LCP entries crossed between r and q: lcp[q + 1 .. r] upwards,
    lcp[r + 1 .. q] downwards.  (m, sa[q]), or (0, NONE) if there is no such q, m == 0 or m < floor."""
    n = len(sa)
    if up:
        stop = r - start + 1
        h = np.flatnonzero(hit(sa[:stop], U32(x), greater, strict)) if stop > 0 else np.zeros(0, dtype=np.int64)
        if not h.size:
            return 0, NONE
        q = int(h[-1])
        crossed = lcp[q + 1:r + 1]
    else:
        first = r + start
        h = np.flatnonzero(hit(sa[first:], U32(x), greater, strict)) if first < n else np.zeros(0, dtype=np.int64)
        if not h.size:
            return 0, NONE
        q = first + int(h[0])
        crossed = lcp[r + 1:q + 1]
    m = int(crossed.min()) if crossed.size else 0xffffffff   # (nothing crossed: only under the too-near wrong rule)
    if m == 0 or m < floor:
        return 0, NONE
    return m, int(sa[q])


def lcp_interval(lcp, r, d, strict=True):
    """I(d) around rank r: [lo, hi] with lcp[lo] < d, lcp[lo + 1 .. hi] >= d, lcp[hi + 1] < d (d >= 1, lcp[0] = lcp[n] = 0)"""
    lo = nearest_left(lcp, r, d, False, strict)
    hi = nearest_right(lcp, r + 1, d, False, strict) - 1
    return lo, hi


def lpnf_leftmost(sa, lcp, r, d):
    lo, hi = lcp_interval(lcp, r, d)
    return int(sa[lo:hi + 1].min())


def lpnf_search(sa, lcp, r, i, lo, cap, memo=None, strict=True):
    """max{d in [lo, cap] : min SA[I(d)] + d <= i} by a linear scan over d; defined where the predicate holds at lo (or
    lo == 0), i.e. on a true SA / LCP with r = ISA[i].  lo >= cap: lo, as the device function answers.  memo: a dict
    that keeps min SA[I(d)] per (r, d) between calls.  Wrong rule (strict=False): `<` in the predicate."""
    if lo >= cap:
        return lo
    best = lo
    for d in range(max(lo, 1), cap + 1):
        key = (r, d)
        g = memo.get(key) if memo is not None else None
        if g is None:
            g = lpnf_leftmost(sa, lcp, r, d)
            if memo is not None:
                memo[key] = g
        if not (g + d <= i if strict else g + d < i):
            break
        best = d
    return best


def near_answers(sa, lcp, queries, memo=None, **rule):
    """(nq, 2) answers to (op, r, a, b, c) rows.  rule: strict=False (ties qualify; `<=` in the interval; `<` in the
    search's predicate) or shift=+1 / -1 (a search starts one rank too far / too near)."""
    sa = np.asarray(sa, dtype=U32)
    lcp = np.asarray(lcp, dtype=U32)
    strict, shift = rule.get("strict", True), rule.get("shift", 0)
    out = np.zeros((len(queries), 2), dtype=U32)
    for k, (op, r, a, b, c) in enumerate(np.asarray(queries).tolist()):
        if op <= FAR_DOWN_GREATER:
            start = (FAR_CLEARED + 1 if op >= FAR_UP_LESS else 1) + shift
            out[k] = search(sa, lcp, r, a, b, up=op in (UP_LESS, UP_GREATER, FAR_UP_LESS, FAR_UP_GREATER),
                            greater=bool(op & 1), start=start, strict=strict)
        elif op == LCP_INTERVAL:
            out[k] = lcp_interval(lcp, r, a, strict)
        elif op == LPNF_LEFTMOST:
            out[k] = (lpnf_leftmost(sa, lcp, r, a), 0)
        else:
            out[k] = (lpnf_search(sa, lcp, r, a, b, c, memo=memo, strict=strict), 0)
    return out


# ---- inputs ----------------------------------------------------------------------------------------------------------
LENGTHS = [1, 2, 15, 16, 17, 31, 32, 33, 255, 256, 257, 271, 272, 273, 4095, 4096, 4097, 65535, 65536, 65537,
           16 ** 5 - 1, 16 ** 5, 16 ** 5 + 1, 16 ** 5 + 17]
FULL_CROSS_MAX = 4097      # above this length a family sends its chosen queries only
POISONS = (0x00, 0xFF)
HIT_P = [0, 15, 16, 255, 256, 4095, 4096, 65535, 65536]            # and len - 1
HIT_K = [0, 1, 15, 16, 17, 255, 256, 257, 4096, 65536]
RANGE_D = [0, 1, 15, 16, 30, 31, 32, 33, 255, 256, 257, 4095, 4096, 4097]   # and len - 1
NEAR_N = [1, 4, 5, 6, 252, 253, 254, 257, 4097, 65537]
NEAR_DIST = [1, 4, 5, 6, 252, 253, 254, 4096]

# one array and the queries that go with it; `applies`: the wrong rules its queries are there to see
WRONG_RULES = {   # name -> the keyword arguments of answers() / near_answers(); pad: see pad_word
    "nonstrict": {"strict": False}, "unmasked": {"pad": True}, "unmasked_range": {"rule": "b+1", "pad": True},
    "range_a-1": {"rule": "a-1"}, "range_b+1": {"rule": "b+1"}, "range_excl_b": {"rule": "excl_b"},
    "near": {"shift": -1}, "far": {"shift": +1},
}
Case = namedtuple("Case", "name base is_max queries applies")
NearCase = namedtuple("NearCase", "name sa lcp queries applies")


def pad_word(poison):
    return 0xffffffff if poison else 0


def _plateau(is_max):
    """(the constant C of an array, a value that beats the threshold x = C)"""
    return (1000, 1001) if is_max else (1000, 999)


def _rows(rows):
    return np.array(sorted(set(rows)), dtype=np.int64).reshape(-1, 3)


def shuffled(queries, seed):
    """so that one wavefront holds walks of different heights"""
    q = np.asarray(queries)
    return q[np.random.default_rng(seed).permutation(len(q))]


def one_hit_cases(n, is_max):
    """a constant array with one entry at p that beats x = C: the plateau equals x and must not hit"""
    C, v = _plateau(is_max)
    out = []
    for p in sorted({p for p in HIT_P + [n - 1] if p < n}):
        base = np.full(n, C, dtype=U32)
        base[p] = v
        rows = [(OP_LEFT, n - 1, C), (OP_RIGHT, 0, C)]
        for k in HIT_K:
            for r in (max(p - k, 0), min(p + k, n - 1)):
                rows += [(OP_LEFT, r, C), (OP_RIGHT, r, C)]
        out.append(Case(f"one_hit[{n},p={p}]", base, is_max, shuffled(_rows(rows), n + p), ("nonstrict",)))
    return out


def edge_ranks(n):
    last = (n - 1) & ~15
    r = {0, 1, 14, 15, 16, 17, 255, 256, 257, n // 2, last - 1, last, n - 17, n - 16, n - 2, n - 1}
    for l, ln in enumerate(level_lengths(n)):   # the base entries around the start of the last block of every level
        first = ((ln - 1) & ~15) << (4 * l)
        r |= {first - 1, first, first - (1 << (4 * l))}
    return sorted(v for v in r if 0 <= v < n)


def no_hit_cases(n, is_max):
    """nothing beats x = C: left answers NONE (from r < 16 too), right answers len from the last block of a level"""
    C, _ = _plateau(is_max)
    rows = [(OP_RIGHT, n, C), (OP_RIGHT, n + 5, C), (OP_RIGHT, 0xffffffff, C)]
    for r in edge_ranks(n):
        rows += [(OP_LEFT, r, C), (OP_RIGHT, r, C)]
    return [Case(f"no_hit[{n}]", np.full(n, C, dtype=U32), is_max, _rows(rows), ("nonstrict", "unmasked"))]


def identity_cases(n, is_max, seed=1):
    """entries 0 and 0xffffffff, and the thresholds that can never be beaten"""
    rng = np.random.default_rng(seed * 1000003 + n)
    never, other = (0xffffffff, 0) if is_max else (0, 0xffffffff)
    ranks = sorted(set(edge_ranks(n)) | set(rng.integers(0, n, size=40).tolist()))
    mixed = np.where(rng.random(n) < 0.5, 0, 0xffffffff).astype(U32)
    rows = []
    for r in ranks:
        rows += [(op, r, x) for op in (OP_LEFT, OP_RIGHT) for x in (never, other)]
        rows.append((OP_RANGE, min(r, n - 1 - r), max(r, n - 1 - r)))
    flat = np.full(n, other if is_max else 0xffffffff, dtype=U32)   # min: all 0xffffffff with x = 0xffffffff
    flat_x = 0 if is_max else 0xffffffff
    flat_rows = [(op, r, flat_x) for op in (OP_LEFT, OP_RIGHT) for r in ranks] + [(OP_RANGE, 0, n - 1)]
    return [Case(f"identity_mixed[{n}]", mixed, is_max, _rows(rows), ("nonstrict",)),
            Case(f"identity_flat[{n}]", flat, is_max, _rows(flat_rows), ("nonstrict",))]


def _random_rows(rng, n, count, xs):
    r = rng.integers(0, n, size=count)
    x = rng.choice(np.asarray(xs, dtype=np.int64), size=count)
    op = rng.integers(0, 2, size=count)
    rows = np.stack([op, r, x], axis=1)
    # ranges of every length scale: log-uniform extent
    m = count // 3
    ext = np.minimum((2.0 ** rng.uniform(0, np.log2(n) + 1, size=m)).astype(np.int64) - 1, n - 1)
    a = (rng.random(m) * (n - ext)).astype(np.int64)
    rows = np.concatenate([rows, np.stack([np.full(m, OP_RANGE), a, a + ext], axis=1)])
    return rows[rng.permutation(len(rows))]   # one wavefront holds walks of different heights


def random_cases(n, is_max, count=600, seed=2):
    """values in {0 .. 3} (short walks), and a rare hit with probability 16^-k per entry, k = 1 .. 5 (long walks)"""
    rng = np.random.default_rng(seed * 1000003 + n * 2 + int(is_max))
    small = rng.integers(0, 4, size=n).astype(U32)
    out = [Case(f"random_small[{n}]", small, is_max, _random_rows(rng, n, count, [0, 1, 2, 3, 4]), ("nonstrict",))]
    C, v = _plateau(is_max)
    for k in range(1, 6):
        base = np.full(n, C, dtype=U32)
        hits = rng.random(n) < 16.0 ** -k
        spread = rng.integers(0, 3, size=n)
        base[hits] = (v + spread[hits]) if is_max else (v - spread[hits])
        out.append(Case(f"random_rare[{n},k={k}]", base, is_max, _random_rows(rng, n, count, [C]), ("nonstrict",)))
    return out


def range_pairs(n):
    pairs = set()
    for d in sorted({d for d in RANGE_D + [n - 1] if d < n}):
        pairs.add((0, d))
        pairs.add((n - 1 - d, n - 1))
        mid = (n // 2) & ~15
        for a_mod in (0, 1, 15):     # a % 16, b = a + d
            for start in (16, mid):
                a = start + a_mod
                if a + d < n:
                    pairs.add((a, a + d))
        for b_mod in (0, 14, 15):    # b % 16, a = b - d
            for start in (mid, (n - 17) & ~15):
                b = start + b_mod
                if b - d >= 0 and b < n:
                    pairs.add((b - d, b))
    return sorted(pairs)


def range_cases(n, is_max, seed=3):
    """four arrays over a random background: every query's own extreme value (they are all different) sits at its a, its
    b, its a - 1 or its b + 1"""
    pairs = range_pairs(n)
    rows = np.array([(OP_RANGE, a, b) for a, b in pairs], dtype=np.int64)
    rng = np.random.default_rng(seed * 1000003 + n * 2 + int(is_max))
    out = []
    for place, applies in (("a", ()), ("b", ("range_excl_b",)), ("a-1", ("range_a-1",)),
                           ("b+1", ("range_b+1", "unmasked_range"))):
        base = rng.integers(1 << 20, 1 << 21, size=n).astype(np.int64)
        order = rng.permutation(len(pairs))
        for rank, j in enumerate(order.tolist()):   # later writes win: each is more extreme than the ones before
            a, b = pairs[j]
            at = {"a": a, "b": b, "a-1": a - 1, "b+1": b + 1}[place]
            if 0 <= at < n:
                base[at] = len(pairs) - rank
        if is_max:
            base = 0xffffffff - base
        # b + 1 == len is the padding: b = len - 1 is in the list, so the unhidden poison shows there
        out.append(Case(f"range[{n},extreme at {place}]", base.astype(U32), is_max, rows, applies))
    return out


def pyramid_cases(n, is_max):
    """every family of a length: all of them at or below FULL_CROSS_MAX, the chosen queries alone above"""
    cases = one_hit_cases(n, is_max) + no_hit_cases(n, is_max) + identity_cases(n, is_max) + range_cases(n, is_max)
    return cases + random_cases(n, is_max, count=600 if n <= FULL_CROSS_MAX else 300)


def level_cases(n, is_max, seed=4):
    """arrays for the level comparison: the padding poison would beat every entry of the first, none of the second"""
    rng = np.random.default_rng(seed * 1000003 + n)
    return [rng.integers(1, 0xffffffff, size=n).astype(U32),
            np.full(n, identity(not is_max), dtype=U32)]


# ---- inputs of the searches ----------------------------------------------------------------------------------------
PLATEAU, DIP, X = 9, 7, 100
FLOORS = [0, DIP - 1, DIP, DIP + 1, PLATEAU - 1, PLATEAU, PLATEAU + 1]   # m - 1, m, m + 1 for both values of m


def near_ranks(n, more=()):
    r = set(range(0, 7)) | set(range(n - 7, n)) | set(range(252, 259)) | set(more)
    return sorted(v for v in r if 0 <= v < n)


def _near_rows(ranks, x, floors, ds):
    rows = []
    for r in ranks:
        rows += [(op, r, x, f, 0) for op in range(UP_LESS, FAR_DOWN_GREATER + 1) for f in floors]
        rows += [(op, r, d, 0, 0) for op in (LCP_INTERVAL, LPNF_LEFTMOST) for d in ds]
    return np.array(rows, dtype=np.int64)


def plateau_case(n, dist, greater, centre, seed=5):
    """sa from {X - 2 .. X + 2}, lcp from {0 .. 5}; around `centre` a plateau of lcp = 9 on which every sa entry ties
    with x = X, but for one qualifying rank at `dist` above and one at `dist` below; a single dip to 7 at the block
    edge at or above the centre"""
    rng = np.random.default_rng(seed * 1000003 + n * 131 + dist * 2 + int(greater))
    sa = rng.integers(X - 2, X + 3, size=n).astype(U32)
    lcp = rng.integers(0, 6, size=n + 1).astype(U32)
    lo, hi = max(centre - dist - 8, 0), min(centre + dist + 8, n - 1)
    sa[lo:hi + 1] = X
    lcp[lo + 1:hi + 1] = PLATEAU
    q = X + 1 if greater else X - 1
    for at in (centre - dist, centre + dist):
        if 0 <= at < n:
            sa[at] = q
    dip = centre & ~15
    if lo < dip <= hi:
        lcp[dip] = DIP
    lcp[0] = lcp[n] = 0
    ds = [PLATEAU - 1, PLATEAU, PLATEAU + 1, DIP, 1]
    middle = [r for r in range(centre - 1, centre + 2) if 0 <= r < n]
    rows = np.concatenate([_near_rows(middle, X, FLOORS, ds),
                           _near_rows(near_ranks(n, (centre - dist, centre + dist)), X, [0, DIP], ds)])
    return NearCase(f"plateau[{n},dist={dist},{'greater' if greater else 'less'},centre={centre}]", sa, lcp, rows,
                    ("nonstrict", "near", "far"))


def near_cases(n):
    out = []
    for dist in NEAR_DIST:
        if dist >= n:
            continue
        # the centre: mid-array where both qualifying ranks fit, else as close to it as one of them allows
        centres = sorted({max(dist, min(n - 1, n // 2)), max(0, min(n - 1 - dist, n // 2))})
        for greater in (False, True):
            out += [plateau_case(n, dist, greater, c) for c in centres]
    rng = np.random.default_rng(6 * 1000003 + n)
    sa = rng.integers(X - 2, X + 3, size=n).astype(U32)
    lcp = rng.integers(0, 6, size=n + 1).astype(U32)
    lcp[0] = lcp[n] = 0
    ranks = near_ranks(n, rng.integers(0, n, size=20).tolist())
    out.append(NearCase(f"near_random[{n}]", sa, lcp, _near_rows(ranks, X, [0, 1, 2, 3], [1, 2, 5, 6]), ("nonstrict",)))
    return out


def fibonacci_word(n):
    a, b = b"A", b"AB"
    while len(b) < n:
        a, b = b, b + a
    return b[:n]


def lpnf_texts():
    import gen
    return {"run": b"A" * 5000, "period2": b"AC" * 3000 + b"G", "fibonacci": fibonacci_word(10_000),
            "repeat_dna": gen.repeat_dna(20_000, seed=11, lo=16, hi=2048).tobytes()}


def text_arrays(text):
    """(sa, isa, lcp with n + 1 entries) of a text from the oracle, in the layout the device keeps"""
    import oracle_lib as oracle
    sa = oracle.suffix_array(text).astype(np.int64)
    lcp = np.concatenate([oracle.lcp_array(text, sa).astype(np.int64), [0]])
    isa = np.zeros(len(sa), dtype=np.int64)
    isa[sa] = np.arange(len(sa))
    return sa.astype(U32), isa, lcp.astype(U32)


def lpnf_positions(n, count=16):
    return sorted(set(np.linspace(0, n - 1, count).astype(np.int64).tolist()) | {1, 2, n - 2})


def lpnf_case(name, text, memo):
    """rows for lpnf_search at a spread of positions: lo in {0, 1, L - 1, L}, cap in {L, L + 1, n - i}, L = the answer for
    lo = 0, cap = n - i.  Returns (NearCase, {i: L})."""
    sa, isa, lcp = text_arrays(text)
    n = len(sa)
    rows, longest = [], {}
    for i in lpnf_positions(n):
        r = int(isa[i])
        L = lpnf_search(sa, lcp, r, i, 0, n - i, memo=memo)
        longest[i] = L
        for lo in sorted({0, 1, max(L - 1, 0), L}):
            if lo > L:      # the predicate does not hold at lo: outside the search's contract
                continue
            for cap in sorted({L, L + 1, n - i}):
                if cap <= n - i:
                    rows.append((LPNF_SEARCH, r, i, lo, cap))
    return NearCase(f"lpnf_search[{name}]", sa, lcp, np.array(rows, dtype=np.int64), ("nonstrict",)), longest
