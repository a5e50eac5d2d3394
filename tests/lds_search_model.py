"""A numpy model of the LDS tile searches (nolzss_amd/csrc/nearest_lds.hpp) on the arrays alone, and the inputs of
tests/test_gpu_lds_search.py.

answers() is a brute force: every rank walks rank by rank to the nearest qualifying rank, as far as the kernel can
see, and keeps the minimum LCP it crosses.  It knows nothing of rounds, blocks or lanes; what it does know is WHERE the
kernel's view ends (the staged tile and the 16 aligned blocks of 16 ranks behind the first 16 steps) and what the kernel
reports when a search ends without a match.  The rules, per rank r of the tile at base = r - r % 1024, li = r - base + 256:
  * outside the arrays SA and LCP read 0 (stage_tile), and lcp[0] = lcp[n] = 0: a minimum dies where a search leaves;
  * a search towards smaller ranks sees down to local rank 16 * max(((li - 17) >> 4) - 15, 0), one towards larger ranks
    up to 16 * min(((li + 17) >> 4) + 15, 95) + 15: 256 to 272 ranks, depending on the alignment;
  * the nearest qualifying rank q in sight: the length is the minimum LCP crossed, the position SA[q]; a length 0
    reports no position;
  * no qualifying rank within 4 steps and the minimum over those 4 is 0, or the same with 16: length 0;
  * otherwise the search left the reach: FAR | minimum over everything in sight;
  * reverse-complement form: only ranks with SA[r] < strand search; of the searches of one kind still going after 4
    steps in one wavefront (256 ranks) the 129th and later, in rank order, report OVERFLOW.
grouped() restates rounds B and C the way a group of lanes shares them (lanes = 1: one lane per search), with the
mistakes of WRONG_RULES on request; tests/test_lds_search_model_host.py shows that it equals the brute force and that
the inputs below see each mistake."""
from collections import namedtuple

import numpy as np

TILE, REACH, WAVE, BLK = 1024, 256, 256, 16
SPAN = TILE + 2 * REACH
NUM_BLK = SPAN // BLK
STEP0, STEP_A = 4, 12
FAR = 0x80000000
OVERFLOW = 0xffffffff
NONE = 0xffffffff
PLAIN, RC = 0, 1
POISONS = (0x00, 0xFF)
LIST_CAP_RC = 128
MAX_DIST = 17 * BLK                 # 272: the longest walk that can end inside the reach
SIZES = [1, 255, 1024, 1025, 3 * 1024 + 17, 8 * 1024 + 300]
STRAND = 1 << 20                    # the strand boundary of the reverse-complement form of every case

# mistakes a grouped rewrite of rounds B + C can make (grouped(rule=...))
WRONG_RULES = ("later_stop",        # the group takes the stop of its last lane that holds one, not of its first
               "partial_with_stop",  # a lane's partial minimum takes in its stopping block as well
               "carry_dropped",     # the minimum carried from the first 16 steps is not taken in
               "wrong_lane")        # the result is written from the first lane's own view, not from the group's


def searches(form):
    return 4 if form == RC else 2


def kind(k):
    """(greater, up) of search k"""
    return k >= 2, k % 2 == 0


def reach_of(n, up):
    """per rank: how many steps the search sees"""
    li = np.arange(n, dtype=np.int64) % TILE + REACH
    if up:
        return li - BLK * np.maximum(((li - (STEP0 + STEP_A + 1)) >> 4) - (BLK - 1), 0)
    return BLK * np.minimum(((li + (STEP0 + STEP_A + 1)) >> 4) + (BLK - 1), NUM_BLK - 1) + BLK - 1 - li


Walk = namedtuple("Walk", "length pos pend0 pend_a found dist carry true_dist reach")


def walk(sa, lcp, k, form=PLAIN, strand=0):
    """search k of every rank, brute force; see the module docstring"""
    sa, lcp = np.asarray(sa, dtype=np.int64), np.asarray(lcp, dtype=np.int64)
    n = len(sa)
    greater, up = kind(k)
    pad = MAX_DIST + 40
    sap, lcpp = np.zeros(n + 2 * pad, dtype=np.int64), np.zeros(n + 1 + 2 * pad, dtype=np.int64)
    sap[pad:pad + n], lcpp[pad:pad + n + 1] = sa, lcp
    r = np.arange(n, dtype=np.int64)
    x = (2 * strand - sa) & 0xffffffff if greater else sa
    active = sa < strand if form == RC else np.ones(n, dtype=bool)
    reach = reach_of(n, up)
    m = np.full(n, 0xffffffff, dtype=np.int64)
    found, dist = np.zeros(n, dtype=bool), np.zeros(n, dtype=np.int64)
    true_dist = np.zeros(n, dtype=np.int64)    # (0: none within MAX_DIST + 30 steps; ranks outside the arrays count, as staged)
    snap = {}
    for d in range(1, MAX_DIST + 31):
        g = r - d if up else r + d
        v, c = sap[g + pad], lcpp[(g + 1 if up else g) + pad]
        qual = v > x if greater else v < x
        true_dist[(true_dist == 0) & qual] = d
        going = ~found & (d <= reach)
        m = np.where(going, np.minimum(m, c), m)
        stop = going & qual
        dist[stop] = d
        found |= stop
        if d in (STEP0, STEP0 + STEP_A):
            snap[d] = (m.copy(), found.copy())
    (m4, f4), (m16, f16) = snap[STEP0], snap[STEP0 + STEP_A]
    q = r - dist if up else r + dist
    length = np.where(found, m, FAR | m)
    pos = np.where(found & (m > 0), sap[q + pad], NONE)
    pend0 = active & ~f4 & (m4 != 0)
    over = np.zeros(n, dtype=bool)
    if form == RC:      # the work list of a wavefront and kind holds 128 searches
        for w0 in range(0, n, WAVE):
            idx = np.flatnonzero(pend0[w0:w0 + WAVE])[LIST_CAP_RC:]
            over[w0 + idx] = True
    pend_a = pend0 & ~over & ~f16 & (m16 != 0)
    dead = (~f4 & (m4 == 0)) | (~over & ~f16 & (m16 == 0))
    length = np.where(dead, 0, length)
    pos = np.where(dead, NONE, pos)
    length, pos = np.where(over, OVERFLOW, length), np.where(over, NONE, pos)
    length, pos = np.where(active, length, 0), np.where(active, pos, NONE)
    return Walk(length.astype(np.uint32), pos.astype(np.uint32), pend0, pend_a, found & pend_a, dist, m16, true_dist, reach)


def answers(sa, lcp, form=PLAIN, strand=0):
    """(len, pos) as nolzss_debug_lds_search returns them: (searches, n) and (2, n) u32"""
    walks = [walk(sa, lcp, k, form, strand) for k in range(searches(form))]
    return np.stack([w.length for w in walks]), np.stack([w.pos for w in walks[:2]])


# ---- rounds B + C as a group of lanes runs them --------------------------------------------------------------------------
def staged(sa, lcp, tile):
    """the staged tile and its block tables (entry B + 1 of a table is block B: one padded entry at either end)"""
    n = len(sa)
    first = tile * TILE - REACH
    g = np.arange(first, first + SPAN + 1)
    s_sa = np.where((g >= 0) & (g < n), np.asarray(sa, dtype=np.int64)[np.clip(g, 0, n - 1)], 0)[:SPAN]
    s_lcp = np.where((g >= 0) & (g <= n), np.asarray(lcp, dtype=np.int64)[np.clip(g, 0, n)], 0)
    blocks = s_sa.reshape(NUM_BLK, BLK)
    big = 0xffffffff
    mn = np.concatenate([[big], blocks.min(axis=1), [big]])
    mx = np.concatenate([[0], blocks.max(axis=1), [0]])
    ldn = np.concatenate([[big], s_lcp[:SPAN].reshape(NUM_BLK, BLK).min(axis=1), [big]])
    lup = np.concatenate([[big], s_lcp[1:SPAN + 1].reshape(NUM_BLK, BLK).min(axis=1), [big]])
    return s_sa, s_lcp, mn, mx, lup, ldn


def lane_scan(cs, quals, start_excl=True):
    """one lane's share: (minimum in front of its first qualifying entry -- through it if not start_excl --, or over all
    its entries; index of that entry or None)"""
    m = 0xffffffff
    for j, (c, q) in enumerate(zip(cs, quals)):
        if q and start_excl:
            return m, j
        m = min(m, c)
        if q:
            return m, j
    return m, None


def group_combine(carry, shares, per, rule=None):
    """the group's (running minimum, index of the stopping entry or None) from its lanes' shares: the carry, the
    minima of the lanes in front of the first lane that holds a stop, and that lane's partial minimum"""
    holders = [q for q, (_, j) in enumerate(shares) if j is not None]
    lane = len(shares) - 1 if not holders else (holders[-1] if rule == "later_stop" else holders[0])
    run = carry
    for q in range(lane + 1):
        run = min(run, shares[q][0])
    return run, (lane * per + shares[lane][1] if holders else None)


Tail = namedtuple("Tail", "length pos block rank_in_block stop_block tie zero_in_front")


def grouped_search(st, li, x, carry, greater, up, lanes=1, rule=None):
    """rounds B + C of one search that is still going after 16 steps"""
    s_sa, s_lcp, mn, mx, lup, ldn = st
    tv, tc = (mx if greater else mn), (lup if up else ldn)
    hit = (lambda v: v > x) if greater else (lambda v: v < x)
    per = BLK // lanes
    b0 = (li - (STEP0 + STEP_A + 1)) >> 4 if up else (li + (STEP0 + STEP_A + 1)) >> 4
    blocks = [b0 - j if up else b0 + j for j in range(BLK)]
    cs, quals = [int(tc[B + 1]) for B in blocks], [bool(hit(int(tv[B + 1]))) for B in blocks]
    shares = []
    for q in range(lanes):
        part = slice(q * per, (q + 1) * per)
        m, j = lane_scan(cs[part], quals[part])
        if rule == "partial_with_stop" and j is not None:
            m = min(m, cs[q * per + j])
        shares.append((m, j))
    run, jstar = group_combine(0xffffffff if rule == "carry_dropped" else carry, shares, per, rule)
    if jstar is None:
        return Tail(FAR | (run & 0x7fffffff), NONE, None, None, None, False, False)
    front = cs[:jstar]
    tie = front.count(min(front + [carry])) >= 2           # the minimum in front of the stop lies in two blocks
    zero_in_front = jstar >= 1 and cs[jstar - 1] == 0 and carry != 0 and all(c != 0 for c in cs[:jstar - 1])
    Bs = blocks[jstar]
    ranks = [BLK * Bs + BLK - 1 - e if up else BLK * Bs + e for e in range(BLK)]
    rc_, rq = [int(s_lcp[p + 1 if up else p]) for p in ranks], [bool(hit(int(s_sa[p]))) for p in ranks]
    shares = [lane_scan(rc_[q * per:(q + 1) * per], rq[q * per:(q + 1) * per], start_excl=False) for q in range(lanes)]
    if rule == "wrong_lane":      # the first lane writes what it saw itself
        m, e = min(run, shares[0][0]), shares[0][1]
    else:
        m, e = group_combine(run, shares, per)
        assert e is not None or rule is not None      # the stopping block holds a qualifying rank
    ok = e is not None and m != 0
    return Tail(m, int(s_sa[ranks[e]]) if ok else NONE, jstar, e, Bs, tie, zero_in_front)


def grouped(sa, lcp, form=PLAIN, strand=0, lanes=1, rule=None, want_tails=False, walks=None):
    """answers() with every search that is still going after 16 steps finished by grouped_search (walks: those of the
    same arrays, form and strand, if the caller has them)"""
    walks = walks or [walk(sa, lcp, k, form, strand) for k in range(searches(form))]
    length, pos = np.stack([w.length for w in walks]), np.stack([w.pos for w in walks])
    tiles, tails = {}, {}
    for k, w in enumerate(walks):
        greater, up = kind(k)
        for r in np.flatnonzero(w.pend_a).tolist():
            tile = r // TILE
            if tile not in tiles:
                tiles[tile] = staged(sa, lcp, tile)
            xv = int(sa[r])
            t = grouped_search(tiles[tile], r % TILE + REACH, (2 * strand - xv) & 0xffffffff if greater else xv,
                               int(w.carry[r]), greater, up, lanes, rule)
            length[k, r], pos[k, r] = t.length, t.pos
            tails[(k, r)] = t
    out = (length.astype(np.uint32), pos[:2].astype(np.uint32))
    return out + (tails,) if want_tails else out


# ---- the inputs -------------------------------------------------------------------------------------------------------
# One design of 8 * 1024 + 300 ranks; the case of size n is its first n ranks.  Background ranks end every search within
# 4 steps (an LCP entry 0 at every fourth rank).  A RUN is a stretch without such zeros: one target rank q and R searching
# ranks beside it whose values fall towards q's far side, so that the search of the rank at offset j passes j - 1 ranks
# that do not qualify and ends at q, distance j; LCP entries 0 close the stretch at both ends.
#   up runs: q at Q, searchers at Q + 1 .. Q + R (search towards smaller ranks); down runs: q at Q, searchers Q - R .. Q - 1
#   less runs: q holds a tiny value; greater runs (reverse-complement form): q holds 2 * STRAND - tiny
# (Q, R, up, greater, zero): zero = offset of an extra LCP entry 0 inside the run, or 0
DENSE = MAX_DIST
W = WAVE
RUNS = [
    # distances 1 .. 272 towards smaller ranks; Q % 16 == 0: offsets 257 .. 272 end exactly at the last rank in reach
    (0, DENSE, True, False, 0),
    (343, 40, False, False, 0),              # (q in the middle of its block: the block's minimum reaches beyond q)
    (639, DENSE, False, False, 0),           # the same towards larger ranks (Q % 16 == 15), half a wavefront off
    (654, 40, True, False, 0),
    (768, DENSE, True, False, 0),            # ends in the FIRST block of the span staged for tile 1 (ranks 768 .. 783)
    (1152, DENSE, True, False, 0),           # half a wavefront off (the work list of 128 of the RC form holds the other
                                             # offsets); wavefront 5 holds 145 of its searches and nothing else
    (6 * W + 28, 17, True, False, 0), (6 * W + 105, 17, False, False, 0),
    (2303, DENSE, False, False, 0),          # ends in the LAST block of the span staged for tile 1 (ranks 2288 .. 2303);
                                             # wavefront 7 holds 17 of its searches and nothing else
    # Pending counts.  The target q of a run is itself pending once, the other way (nothing is smaller than q and the run
    # has no LCP zero), so a wavefront with searches in ONE direction has its q in the wavefront next to it, and a
    # wavefront with P in BOTH directions holds two runs of P - 1 long searches and their targets.
    (10 * W, 31, False, False, 0),           # wavefront 9: 15, downwards only
    (11 * W - 1, 32, True, False, 0),        # wavefront 10: the two targets, 1 + 1; wavefront 11: 16, upwards only
    (13 * W, 48, False, False, 0),           # wavefront 12: 32 downwards (the case of 3 * 1024 + 17 ranks ends inside)
    (13 * W + 63, 60, True, False, 5),       # the minimum reaches 0 one block in front of q's block
    (14 * W - 1, 49, True, False, 0),        # wavefront 14: 33, upwards only
    (16 * W, 17, False, False, 0),           # wavefront 15: 1, downwards only
    (16 * W + 96, 60, False, False, 5),      # as in wavefront 13, downwards
    (17 * W - 1, 17, True, False, 0),        # wavefront 17: 1, upwards only
    (18 * W + 4, 30, True, False, 0), (18 * W + 100, 30, False, False, 0),     # 15 + 15
    (19 * W + 5, 31, True, False, 0), (19 * W + 124, 31, False, False, 0),      # 16 + 16
    (20 * W + 7, 32, True, False, 0), (20 * W + 133, 32, False, False, 0),      # 17 + 17
    (21 * W + 9, 47, True, False, 0), (21 * W + 150, 47, False, False, 0),      # 32 + 32
    (22 * W + 13, 48, True, False, 0), (22 * W + 160, 48, False, False, 0),     # 33 + 33
    (23 * W + 1, 100, True, False, 0), (23 * W + 250, 100, False, False, 0),    # 85 + 85
    # wavefront 24: background only, nothing pending
    (25 * W, DENSE, True, True, 0), (26 * W + 128, DENSE, True, True, 0),       # greater, upwards
    (29 * W - 1, DENSE, False, True, 0), (30 * W + 127, DENSE, False, True, 0),  # greater, downwards
    (7823, 290, True, False, 0),             # Q % 16 == 15: offsets 258 .. 273 end at the FIRST rank beyond the reach
    (8416, 290, False, False, 0),            # the same downwards (Q % 16 == 0)
    (8448 + 2, 40, True, False, 0),          # the last tile: 300 ranks, the rest lies beyond n
]
N_DESIGN = SIZES[-1]
_design = None


def design():
    global _design
    if _design is None:
        n, half = N_DESIGN, STRAND // 2
        rng = np.random.default_rng(20261019)
        sa = half + rng.permutation(half)[:n].astype(np.int64)              # background: original strand, above every searcher
        other = np.arange(n) % 3 == 0
        sa[other] = STRAND + (1 << 18) + np.arange(n)[other]                  # ... and the other strand
        lcp = rng.integers(1, 6, size=n + 1).astype(np.int64)
        lcp[::4] = 0
        lcp[n] = 0
        taken = np.zeros(n + 2, dtype=bool)
        for idx, (Q, R, up, greater, zero) in enumerate(RUNS):
            lo, hi = (Q, Q + R) if up else (Q - R, Q)
            assert 0 <= lo and hi < n and not taken[lo:hi + 2].any(), (Q, R)
            taken[lo:hi + 1] = True
            tiny = 1 + idx
            sa[Q] = 2 * STRAND - tiny if greater else tiny
            j = np.arange(1, R + 1)
            sa[Q + j if up else Q - j] = half - 1 - 1000 * idx - j          # falls with the offset: nobody in between qualifies
            # LCP entry crossed between offsets j - 1 and j: multiples of 10 (ties), drifting down or up with the offset,
            # so that the minimum lies near the searcher in one run and near q in the next
            drift = -10 * j if idx % 2 == 0 else 10 * j
            e = 5000 + drift + 10 * rng.integers(0, 150, size=R)
            lcp[Q + j if up else Q - j + 1] = e
            if zero:
                lcp[Q + zero if up else Q - zero + 1] = 0
            lcp[lo], lcp[hi + 1] = 0, 0
        assert len(np.unique(sa)) == n
        _design = (sa.astype(np.uint32), lcp.astype(np.uint32))
    return _design


Case = namedtuple("Case", "n sa lcp")


def case(n):
    sa, lcp = design()
    lcp = lcp[:n + 1].copy()
    lcp[n] = 0
    return Case(n, sa[:n].copy(), lcp)


_walks = {}


def case_walks(c, form):
    """the brute-force walks of a case (computed once per size and form)"""
    if (c.n, form) not in _walks:
        _walks[(c.n, form)] = [walk(c.sa, c.lcp, k, form, STRAND) for k in range(searches(form))]
    return _walks[(c.n, form)]


def wave_counts(walks_up, walks_down, n):
    """per wavefront: (searches pending after round A upwards, downwards)"""
    return [(int(walks_up.pend_a[w:w + WAVE].sum()), int(walks_down.pend_a[w:w + WAVE].sum())) for w in range(0, n, WAVE)]


def features(c, form=PLAIN):
    """what the searches of a case exercise, from the model (test_gpu_lds_search.py asserts these against EXPECT)"""
    walks = case_walks(c, form)
    _, _, tails = grouped(c.sa, c.lcp, form, STRAND, want_tails=True, walks=walks)
    f = {"distances": [], "round_b_blocks": set(), "round_c_ranks": set(), "stop_blocks": set(), "last_in_reach": 0,
         "first_beyond": 0, "far_with_bound": 0, "zero_in_front": 0, "ties": 0, "overflow": 0}
    for k, w in enumerate(walks):
        f["distances"].append(set(w.dist[w.found].tolist()))
        f["last_in_reach"] += int((w.found & (w.dist == w.reach)).sum())
        gone = w.pend_a & ~w.found
        f["first_beyond"] += int((gone & (w.true_dist == w.reach + 1)).sum())
        f["far_with_bound"] += int((gone & ((w.length & 0x7fffffff) != 0)).sum())
        f["overflow"] += int((w.length == OVERFLOW).sum())
    for t in tails.values():
        if t.block is not None:
            f["round_b_blocks"].add(t.block)
            f["round_c_ranks"].add(t.rank_in_block)
            f["stop_blocks"].add(t.stop_block)
            f["ties"] += int(t.tie)
            f["zero_in_front"] += int(t.zero_in_front)
    counts = wave_counts(walks[0], walks[1], c.n)
    f["one_direction"] = {max(a, b) for a, b in counts if min(a, b) == 0}
    f["both_directions"] = {a for a, b in counts if a == b and a > 0} | {min(a, b) for a, b in counts if min(a, b) >= 64}
    f["wave_counts"] = counts
    f["ranks_beyond_n"] = c.n % TILE != 0
    return f


def covers(have, need):
    """the pending counts `need` (64 stands for 64 or more) are among `have`"""
    return all(any(h >= 64 for h in have) if p == 64 else p in have for p in need)


# What the searches of each case hold, by size (features() of the case must give exactly the distances and at least the
# rest).  distances: per search, the intervals of distances at which searches still going after 16 steps end inside the
# reach -- everything from 17 to 272 that fits the array, less what the 128-entry work lists of the reverse-complement
# form turn away in the two smaller sizes.  pending: searches of a wavefront still going after round A (64: or more).
ALL = [(17, MAX_DIST)]
EXPECT = {
    1: {"distances": {PLAIN: [[], []], RC: [[], [], [], []]}},
    # (255 downwards: rank 0 holds the smallest value but 0, which is what the kernel stages behind rank n - 1)
    255: {"distances": {PLAIN: [[(17, 254)], [(255, 255)]], RC: [[(17, 132)], [(255, 255)], [], []]}},
    1024: {"distances": {PLAIN: [ALL, ALL], RC: [[(17, 132), (256, 272)], [(17, 127), (181, 272)], [], []]},
           "last_in_reach": True},
    1025: {"distances": {PLAIN: [ALL, ALL], RC: [[(17, 132), (256, 272)], [(17, 127), (181, 272)], [], []]},
           "stop_blocks": {0}, "last_in_reach": True, "one_direction": [1]},
    3 * 1024 + 17: {"distances": {PLAIN: [ALL, ALL], RC: [ALL, ALL, [], []]}, "round_b_blocks": set(range(16)),
                    "stop_blocks": {0, NUM_BLK - 1}, "last_in_reach": True, "ties": True,
                    "one_direction": [0, 15, 16, 17, 64], "both_directions": [1]},
    8 * 1024 + 300: {"distances": {PLAIN: [ALL, ALL], RC: [ALL, ALL, ALL, ALL]}, "round_b_blocks": set(range(16)),
                     "round_c_ranks": set(range(16)), "stop_blocks": {0, NUM_BLK - 1}, "last_in_reach": True,
                     "first_beyond": True, "far_with_bound": True, "zero_in_front": True, "ties": True,
                     "one_direction": [0, 1, 15, 16, 17, 32, 33, 64], "both_directions": [1, 15, 16, 17, 32, 33, 64]},
}


def intervals(values):
    out = []
    for v in sorted(values):
        if out and out[-1][1] == v - 1:
            out[-1] = (out[-1][0], v)
        else:
            out.append((v, v))
    return out


def check_features(c, form):
    """assert that the case holds what EXPECT lists for its size; returns the features"""
    f, e = features(c, form), EXPECT[c.n]
    assert [intervals(d) for d in f["distances"]] == e["distances"][form], (c.n, form)
    for name in ("round_b_blocks", "round_c_ranks", "stop_blocks"):
        assert e.get(name, set()) <= f[name], (c.n, form, name, sorted(f[name]))
    for name in ("last_in_reach", "first_beyond", "far_with_bound", "zero_in_front", "ties"):
        assert not e.get(name) or f[name] > 0, (c.n, form, name)
    for name in ("one_direction", "both_directions"):
        assert covers(f[name], e.get(name, [])), (c.n, form, name, sorted(f[name]))
    assert f["ranks_beyond_n"] == (c.n % TILE != 0)
    if form == RC and c.n >= 255:
        assert f["overflow"] > 0      # some work list of 128 is full
    return f
