"""The two arithmetic passes of the suffix-array construction over repetitive texts (sa_repeats.hip: the pair-run pass and
the periodic pass, with the regroup<false> behind the latter) and the counts in front of them, in plain numpy -- TEST
INFRASTRUCTURE ONLY.  Four things:

  * (a) the definition: group_sort_model.Text.compare, the order and the LCP of two suffixes symbol by symbol.  The true
    suffix array and LCP array of a text (true_arrays) are computed by prefix doubling and Kasai's walk -- or in closed
    form for A^p C A^q -- and tests/test_sa_repeats_model_host.py checks them against Text.compare;
  * a state builder (build_state): the true arrays cut into groups at a depth h, a chosen share of the groups refined to
    random deeper depths, the members of every group laid out in text, reversed or shuffled order, the boundaries inside
    groups holding kLcpPending, kLcpPendingCompared or a mix of the two: a consistent partial state, as it stands behind
    write_all_ranks;
  * (b) round-level models of count_large_groups, one pair_run_pass and periodic_pass, written from the comments and the
    code of the kernels, kernel by kernel.  Both passes are deterministic (a member's place in the pair-run pass is
    below + same_before; the radix sorts of the periodic pass are stable over (group, position), and a group that is left
    alone comes out in ascending position), so the models give the exact sa, lcp, rank, next active list, counts, return
    value, per_hint and per_attempts that nolzss_debug_repeat_pass must return; `bug` switches one named mistake on;
  * (c) the inputs (CASES) and check_refinement, the model-independent property of every output: a refinement of the
    state that went in, under the true arrays.

Three of the named mistakes cannot change the output on any state the hook accepts (NEUTRAL_BUGS: the code they touch is
a shortcut or a defence, see there); the host test shows that they change nothing.
"""
import functools
from collections import namedtuple

import numpy as np

import group_sort_model as G
from group_sort_model import Text  # noqa: F401  (reused, not copied)

RUN_MAX, VERIFY_MAX = 16, 4096            # kRunGroupMax, kPerVerifyMax
PENDING, COMPARED = G.PENDING, G.COMPARED  # kLcpPending, kLcpPendingCompared
PENDING_MIN = PENDING - 64                 # kLcpPendingMin
DEFERRED = NONE = 0xffffffff               # kRunDeferred, kPerNone
BAD = 0x80000000                           # kPerBad
M32 = 0xffffffff
BIG = 1 << 40
COUNTS, PERIODIC, PAIR_RUNS = 0, 1, 2      # the hook's `which`
ORDERS = G.ORDERS

BUGS = (
    # pair runs
    "group_limit_17",        # run_group_size takes groups of 17
    "still_tied_limit_15",   # still_tied_kernel walks back only for the first 15 members (the observable neighbour of the next)
    "off_end_own_only",      # group_end_kernel: "the text ends behind a member" seen by that member alone
    "own_chain",             # the steps of a group taken from the member's own chain, not the shortest of the group
    "end_lcp_no_steps",      # group_members_kernel: end_lcp without + steps
    "no_same_before",        # group_end_kernel: same_before ignored (place and the LCP condition)
    # periodic runs
    "q_lt_depth",            # q <= depth taken as q < depth (the verify filter, the limit without verify, the run check)
    "verify_4097",           # kPerVerifyMax = 4097
    "no_short_run_check",    # per_rho_kernel: the (E - pos) + lam < need check dropped
    "no_text_end",           # per_rho_kernel: the E + q >= n branch dropped
    "tied_E_not_flagged",    # per_rho_kernel: c1 == c2 goes on (lam = 0)
    "down_up_swapped",       # per_rho_kernel: rho / ~rho the wrong way round
    "lcp_max_across",        # per_view_kernel: the LCP between a down and an up member as the larger rho
    "cand_gate_m8",          # the early exit at cand < m / 8
    "hint_not_lowered",      # per_flags_kernel: the hint stored, not lowered (the last flagged group's q)
    # counts
    "near_4097",             # count_large_groups: neighbours up to 4097 apart
)
# Mistakes that no output can show on a state the hook accepts:
#   still_tied_walk_past_16  the guard s - g0 < kRunGroupMax only spares the walk: a group of more than 16 members is not
#                            touched, every entry inside it is pending, and the walk ends at g0 as the guard says;
#   q_apart_not_excused      a pair exactly q apart that the text check flags is flagged by per_rho_kernel too:
#                            (E - pos) + lam IS lcp(pos, pos + q) when the decided LCP entries are true;
#   pending_lam_accepted     the range minimum between two groups ends at the head entry of the upper one, which is
#                            decided in every state whose ranks are the head slots by lcp: the exit is a defence.
NEUTRAL_BUGS = ("still_tied_walk_past_16", "q_apart_not_excused", "pending_lam_accepted")
BRANCHES = ("link:block", "link:wave", "link:mixed", "link:padding", "rho:flagged", "rho:text_end", "rho:tied_E",
            "rho:short_run", "rho:down", "rho:up", "end:off_end", "end:off_end_other", "end:classes_tied",
            "gate:first_call", "gate:candidates", "gate:attempts", "verify:text", "flags:hint")


# ---- the true arrays ---------------------------------------------------------------------------------------------------------
def _symbols(text):
    """one integer per position and one for the end, ordered as Text.compare orders: terminators by index (the end of
    the text is the last of them) below every symbol"""
    nt = text.terms.size
    sym = text.codes[:text.n].astype(np.int64) + nt
    sym[text.terms[:-1]] = np.arange(nt - 1)
    return np.concatenate([sym, [nt - 1]])


def _common(buf, w, a, b, h, n1):
    """symbols suffixes a and b of buf (w bytes per symbol, n1 symbols) share from offset h on, plus h"""
    step = 32
    while True:
        x, y = buf[(a + h) * w:(a + h + step) * w], buf[(b + h) * w:(b + h + step) * w]
        if x != y or not x:
            break
        h += step
        step *= 2
    lo, hi = 0, min(step, n1 - max(a, b) - h)  # the first difference lies in [h + lo, h + hi]
    while lo < hi:
        mid = (lo + hi + 1) // 2
        if buf[(a + h) * w:(a + h + mid) * w] == buf[(b + h) * w:(b + h + mid) * w]:
            lo = mid
        else:
            hi = mid - 1
    return h + lo


def true_arrays(text):
    """-> (sa[n], lcp[n + 1]) of the text under Text.compare, lcp[0] = lcp[n] = 0: prefix doubling, then Kasai's walk"""
    n = text.n
    sym = _symbols(text)
    n1 = n + 1
    rank = np.unique(sym, return_inverse=True)[1].astype(np.int64).ravel() + 1
    k = 1
    while True:
        r2 = np.zeros(n1, dtype=np.int64)
        r2[:n1 - k] = rank[k:]
        order = np.lexsort((r2, rank))
        a, b = rank[order], r2[order]
        new = np.concatenate([[True], (a[1:] != a[:-1]) | (b[1:] != b[:-1])])
        rank = np.empty(n1, dtype=np.int64)
        rank[order] = np.cumsum(new)
        if rank.max() == n1 or k >= n1:
            break
        k *= 2
    sa1 = np.argsort(rank, kind="stable")
    sa = sa1[sa1 != n]
    isa = np.empty(n, dtype=np.int64)
    isa[sa] = np.arange(n)
    buf = sym.astype(np.uint16).tobytes()
    lcp = np.zeros(n + 1, dtype=np.int64)
    h = 0
    sal = sa.tolist()
    for i, r in enumerate(isa.tolist()):
        if r == 0:
            h = 0
            continue
        h = _common(buf, 2, i, sal[r - 1], max(h - 1, 0), n1)
        lcp[r] = h
    return sa, lcp


def true_arrays_apcaq(p, q):
    """the same in closed form for A^p C A^q: the suffixes A^j (j = 1 .. q), shorter first, then A^i C A^q, i = p .. 0"""
    n = p + 1 + q
    sa = np.concatenate([np.arange(n - 1, p, -1), np.arange(0, p + 1)]).astype(np.int64)
    lcp = np.concatenate([np.arange(0, q), [min(p, q)], np.arange(p - 1, -1, -1), [0]]).astype(np.int64)
    if q == 0:
        lcp = np.concatenate([[0], np.arange(p - 1, -1, -1), [0]]).astype(np.int64)
    return sa, lcp


# ---- the state builder ---------------------------------------------------------------------------------------------------------
State = namedtuple("State", "sa lcp rank slot grp")


def _heads_of(lcp, n):
    """per slot the head slot of its group: the nearest slot at or in front of it whose LCP entry is decided"""
    dec = lcp[:n] < PENDING_MIN
    return np.maximum.accumulate(np.where(dec, np.arange(n), 0))


def _listed(lcp, n):
    hs = _heads_of(lcp, n)
    size = np.bincount(hs, minlength=n)
    slot = np.nonzero(size[hs] >= 2)[0]
    return slot, hs[slot]


def build_state(text, truth, h, order="text", deeper=0.0, code="pending", lcp_n=PENDING, seed=0):
    """the true arrays cut into groups at depth h; a share `deeper` of the groups of three and more cut again at a depth
    that one of their boundaries decides (h stays the least depth); members in `order`; boundaries inside groups hold
    `code`: "pending", "compared" or "mixed" (one of the two, slot by slot)"""
    sa_t, lcp_t = truth
    n = text.n
    rng = np.random.default_rng(seed)
    inner = lcp_t[:n] >= h
    inner[0] = False
    if deeper > 0:
        hs = np.maximum.accumulate(np.where(~inner, np.arange(n), 0))
        size = np.bincount(hs, minlength=n)
        for g in np.nonzero(size >= 3)[0]:
            if rng.random() < deeper:
                inside = lcp_t[g + 1:g + size[g]]
                d = int(inside[rng.integers(inside.size)]) + 1
                inner[g + 1:g + size[g]] &= inside >= d
    pend = {"pending": np.full(n, PENDING), "compared": np.full(n, COMPARED),
            "mixed": np.where(rng.random(n) < 0.5, PENDING, COMPARED)}[code]
    lcp = np.concatenate([np.where(inner, pend, lcp_t[:n]), [lcp_n]]).astype(np.int64)
    hs = _heads_of(lcp, n)
    key = {"text": sa_t, "reversed": -sa_t, "shuffle": rng.random(n)}[order]
    sa = sa_t[np.lexsort((key, hs))]
    rank = np.empty(n, dtype=np.int64)
    rank[sa] = hs + 1
    slot, grp = _listed(lcp, n)
    return State(sa, lcp, rank, slot, grp)


# ---- range minima over the LCP array (pyr_range<false>: pending codes are +infinity by their value) -----------------------------
class RangeMin:
    def __init__(self, a):
        self.lv = [np.asarray(a, dtype=np.int64)]
        k = 1
        while 2 * k <= self.lv[0].size:
            p = self.lv[-1]
            self.lv.append(np.minimum(p[:-k], p[k:]))
            k *= 2

    def query(self, a, b):
        """min of entries a .. b inclusive, a <= b (arrays)"""
        a, b = np.asarray(a, dtype=np.int64), np.asarray(b, dtype=np.int64)
        assert (a <= b).all() and (a >= 0).all() and (b < self.lv[0].size).all(), "a range minimum over no range"
        length = b - a + 1
        j = np.floor(np.log2(length)).astype(np.int64)
        j = np.where((1 << (j + 1)) <= length, j + 1, j)
        j = np.where((1 << j) > length, j - 1, j)
        out = np.empty(a.shape, dtype=np.int64)
        for lev in np.unique(j):
            sel = j == lev
            t = self.lv[lev]
            out[sel] = np.minimum(t[a[sel]], t[b[sel] - (1 << lev) + 1])
        return out


# ---- (b) count_large_groups --------------------------------------------------------------------------------------------------
def count_large(st, limit=RUN_MAX, bug=None):
    """per_count_large_kernel: members beyond the first `limit` of their group, groups of more than `limit`, groups,
    members whose successor in the list is of their group and at most kPerVerifyMax symbols away"""
    slot, grp = st.slot, st.grp
    if slot.size == 0:
        return [0, 0, 0, 0]
    near = VERIFY_MAX + (1 if bug == "near_4097" else 0)
    j = slot - grp
    pos = st.sa[slot]
    same = grp[1:] == grp[:-1]
    d = np.abs(pos[1:] - pos[:-1])
    return [int((j >= limit).sum()), int((j == limit).sum()), int((j == 0).sum()), int((same & (d <= near)).sum())]


# ---- (b) one pair-run pass ----------------------------------------------------------------------------------------------------
def pair_run_pass(st, bug=None, branches=None):
    """pair_run_pass: group_link_kernel .. group_members_kernel, still_tied_kernel, the compaction -> (State, progress)"""
    assert bug is None or bug in BUGS + NEUTRAL_BUGS
    branches = set() if branches is None else branches
    sa, lcp, rank = st.sa.copy(), st.lcp.copy(), st.rank.copy()
    n, m = sa.size, st.slot.size
    limit = RUN_MAX + (1 if bug == "group_limit_17" else 0)
    hs = _heads_of(lcp, n)
    size = np.bincount(hs, minlength=n)
    ksz = np.where((size >= 2) & (size <= limit), size, 0)    # run_group_size, by head slot
    ar = np.arange(n)
    # group_link_kernel
    g_all = rank - 1
    act = np.nonzero(ksz[g_all] > 0)[0]                       # positions in a group of 2 .. 16
    g, K = g_all[act], ksz[g_all[act]]
    cols = np.arange(limit)
    valid = cols[None, :] < K[:, None]
    mem = np.where(valid, sa[np.minimum(g[:, None] + cols, n - 1)], BIG)
    above = np.where(mem > act[:, None], mem, BIG).min(axis=1)
    lowest = mem.min(axis=1)
    d = np.where(above < BIG, above, lowest) - act
    assert bug is not None or (d != 0).all()
    if (d == 0).any():  # (only a state that a mistake has spoilt: gsz = 0, the position takes no part)
        act, g, K, valid, mem, d = (x[d != 0] for x in (act, g, K, valid, mem, d))
    link, gsz = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
    link[act], gsz[act] = d & M32, K
    # run_breaks_kernel and the scan: where the chain of every position ends
    on = np.zeros(n, dtype=bool)
    on[:-1] = (link[:-1] != 0) & (link[1:] == link[:-1]) & (gsz[1:] == gsz[:-1])
    chain_end = np.minimum.accumulate(np.where(on, BIG, ar)[::-1])[::-1]
    own = chain_end - ar
    # group_run_kernel / run_steps: the shortest chain of the group (a pair: its own)
    togo = np.where(valid, own[np.minimum(mem, n - 1)], BIG).min(axis=1)
    steps = own[act] if bug == "own_chain" else np.where(K > 2, togo, own[act])
    # group_end_kernel
    end_place, end_head, end_lcp = np.full(n, -1, dtype=np.int64), np.full(n, -1, dtype=np.int64), np.full(n, -1, dtype=np.int64)
    at_end = np.nonzero(steps == 0)[0]
    t = act[at_end]
    tm, tv = mem[at_end], valid[at_end]
    other = tv & (tm != t[:, None])
    past = other & (tm + 1 >= n)
    off = t + 1 >= n
    if off.any():
        branches.add("end:off_end")
    if bug != "off_end_own_only":
        if (past.any(axis=1) & ~off).any():
            branches.add("end:off_end_other")
        off = off | past.any(axis=1)
    mine = np.where(t + 1 < n, rank[np.minimum(t + 1, n - 1)], 0)
    seen = other & ~past
    c = np.where(seen, rank[np.minimum(tm + 1, n - 1)], BIG)
    lower = seen & (c < mine[:, None])
    below = lower.sum(axis=1)
    pred = np.where(lower, c, 0).max(axis=1) if t.size else np.zeros(0, dtype=np.int64)
    same_before = (seen & (c == mine[:, None]) & (tm < t[:, None])).sum(axis=1)
    if ((seen & (c == mine[:, None])).any(axis=1) & ~off).any():
        branches.add("end:classes_tied")
    if bug == "no_same_before":
        same_before = np.zeros_like(same_before)
    first_of_class = ~off & (same_before == 0) & (below > 0)
    le = np.full(t.size, DEFERRED, dtype=np.int64)
    if first_of_class.any():
        rm = RangeMin(lcp)
        f = np.nonzero(first_of_class)[0]
        le[f] = (1 + rm.query(pred[f], mine[f] - 1)) & M32
    end_place[t] = np.where(off, DEFERRED, below + same_before)
    end_head[t], end_lcp[t] = below, le
    # group_members_kernel
    e = act + steps
    place = end_place[np.minimum(e, n - 1)]
    assert bug is not None or (place >= 0).all(), "a member reads the place of a position that is no member of an end group"
    place = np.where(place < 0, DEFERRED, place)
    go = place != DEFERRED
    i, gi, pl, st_i, e_i = act[go], g[go], place[go], steps[go], np.minimum(e, n - 1)[go]
    if bug is None:  # the places of a group are a permutation of its slots
        assert np.unique(gi + pl).size == i.size and np.array_equal(np.sort(gi + pl), np.nonzero(np.isin(hs, np.unique(gi)))[0])
    sa[gi + pl] = i
    wl = end_lcp[e_i] != DEFERRED
    lcp[(gi + pl)[wl]] = (end_lcp[e_i][wl] + (0 if bug == "end_lcp_no_steps" else st_i[wl])) & M32
    rank[i] = gi + end_head[e_i] + 1
    # still_tied_kernel and the compaction
    s, g0 = st.slot, st.grp
    walk = RUN_MAX - 1 if bug == "still_tied_limit_15" else (BIG if bug == "still_tied_walk_past_16" else RUN_MAX)
    head = np.where(s - g0 < walk, np.maximum(_heads_of(lcp, n)[s], g0), g0) if m else g0
    keep = (head + 1 < n) & (lcp[np.minimum(head + 1, n - 1)] >= PENDING_MIN) if m else np.zeros(0, dtype=bool)
    out = State(sa, lcp, rank, s[keep], head[keep])
    left = int(keep.sum())
    return out, left < m - m // 8


# ---- (b) the periodic pass ---------------------------------------------------------------------------------------------------
def periodic_pass(text, st, h, per_attempts, counts, bug=None, branches=None):
    """periodic_pass with its gates and the regroup<false> behind it -> (State, return value, per_hint, per_attempts)"""
    assert bug is None or bug in BUGS + NEUTRAL_BUGS
    branches = set() if branches is None else branches
    n, m = st.sa.size, st.slot.size
    in_large, near_members = counts[0], counts[3]
    if m == 0 or per_attempts >= 3:
        branches.add("gate:attempts")
        return st, False, 0, per_attempts
    if per_attempts == 0 and (in_large < m // 8 or near_members < m // 32):
        branches.add("gate:first_call")
        return st, False, 0, 3
    per_attempts += 1
    vmax = VERIFY_MAX + (1 if bug == "verify_4097" else 0)
    slot, grp = st.slot, st.grp
    pos = st.sa[slot]
    o1 = np.lexsort((pos, grp))                       # per_keys_kernel and the first sort: (group, position)
    kg, kp = grp[o1], pos[o1]
    first = np.concatenate([[True], kg[1:] != kg[:-1]])
    gstart = np.nonzero(first)[0]
    gid = np.cumsum(first) - 1
    same_next = np.concatenate([kg[1:] == kg[:-1], [False]])
    nxt = np.concatenate([kp[1:], [0]])
    link = np.where(same_next, nxt - kp, NONE)
    qg = np.minimum.reduceat(link, gstart)            # per_link_kernel (every group has two members: a distance exists)
    for b0 in range(0, m, 256):                        # ... and which of its reductions ran
        blk = kg[b0:b0 + 256]
        if blk.size == 256 and (blk == blk[0]).all():
            branches.add("link:block")
            continue
        if blk.size < 256:
            branches.add("link:padding")
        for w0 in range(0, 256, 64):
            wv = blk[w0:w0 + 64]
            if wv.size == 64 and (wv == wv[0]).all():
                branches.add("link:wave")
            elif wv.size:
                branches.add("link:mixed")
    q = qg[gid]
    depth = min(h, 0x7ffffffe)
    verify = text.terms.size == 1 and depth < vmax
    low = depth - 1 if bug == "q_lt_depth" else depth  # q <= low: the depth compared so far covers the period
    qmax = vmax if verify else low
    cand = int((q <= qmax).sum())                      # per_candidates_kernel
    if cand < m // (8 if bug == "cand_gate_m8" else 16):
        branches.add("gate:candidates")
        return st, False, 0, 3
    bad = np.zeros(gstart.size, dtype=bool)
    if verify:                                         # per_verify_kernel
        chk = same_next & (q > low) & (q <= vmax)
        if bug != "q_apart_not_excused":
            chk &= link != q
        for j in np.nonzero(chk)[0]:
            a, b, qq = int(kp[j]), int(nxt[j]), int(q[j])
            branches.add("verify:text")
            if min(text.lcp(a, b), qq) < min(qq, n - b):
                bad[gid[j]] = True
    over = qg > qmax                                   # per_flags_kernel
    hint = NONE
    if over.any():
        branches.add("flags:hint")
        hint = int(qg[over][-1]) if bug == "hint_not_lowered" else int(qg[over].min())
    bad |= over
    PQ = np.zeros(n, dtype=np.int64)
    run = ~over[gid] & (link == q)
    PQ[kp[run]] = q[run]
    on = np.zeros(n, dtype=bool)                       # per_breaks_kernel and the scan
    on[:-1] = (PQ[:-1] != 0) & (PQ[1:] == PQ[:-1])
    ar = np.arange(n)
    end_of = np.minimum.accumulate(np.where(on, BIG, ar)[::-1])[::-1]
    # per_rho_kernel
    kraw = np.zeros(m, dtype=np.int64)
    live = ~bad[gid]
    if (~live).any():
        branches.add("rho:flagged")
    E = np.where(PQ[kp] == q, end_of[kp] + 1, kp)
    assert bug is not None or (E[live] < n).all()
    text_end = live & (E + q >= n)
    if bug == "no_text_end":
        text_end[:] = False
    if text_end.any():
        branches.add("rho:text_end")
    kraw[text_end] = np.minimum((E - kp) + q, n - kp)[text_end]
    go = live & ~text_end
    c1 = st.rank[np.minimum(E, n - 1)]
    e2 = E + q
    c2 = np.where(e2 < n, st.rank[np.minimum(e2, n - 1)], 0)
    tied_E = go & (c1 == c2)
    if tied_E.any():
        branches.add("rho:tied_E")
    lam = np.zeros(m, dtype=np.int64)
    ask = go & ~tied_E & (c2 != 0)
    if ask.any():
        rm = RangeMin(st.lcp)
        lam[ask] = rm.query(np.minimum(c1, c2)[ask], np.maximum(c1, c2)[ask] - 1)
    flag = tied_E & (bug != "tied_E_not_flagged")
    if bug != "pending_lam_accepted":
        flag = flag | (go & (lam >= PENDING_MIN))
    need = np.minimum(q, n - (kp + q))
    short = go & ~flag & (q > low) & (E != kp) & ((E - kp) + lam < need)
    if short.any():
        branches.add("rho:short_run")
    if bug != "no_short_run_check":
        flag = flag | short
    np.logical_or.at(bad, gid[flag], True)
    rho = ((E - kp) + lam + q) & M32
    down = c2 < c1
    if bug == "down_up_swapped":
        down = ~down
    keyed = go & ~flag
    kraw[keyed] = np.where(down, rho, ~rho & M32)[keyed]
    if (keyed & ~bad[gid] & down).any():
        branches.add("rho:down")
    if (keyed & ~bad[gid] & ~down).any():
        branches.add("rho:up")
    # per_keys2_kernel, the second sort (stable), per_view_kernel
    K = np.where(bad[gid], 0, kraw)
    o2 = np.lexsort((K, kg))
    g2, K2, v2 = kg[o2], K[o2], kp[o2]
    same_prev = np.concatenate([[False], g2[1:] == g2[:-1]])
    Kp = np.concatenate([[0], K2[:-1]])
    r_of = lambda x: np.where(x & BAD, ~x & M32, x)  # noqa: E731
    ra, rb = r_of(Kp), r_of(K2)
    l_new = np.minimum(ra, rb)
    if bug == "lcp_max_across":
        l_new = np.where((Kp & BAD) != (K2 & BAD), np.maximum(ra, rb), l_new)
    # regroup<false>: heads, the new order, the LCP of the boundaries that appeared, ranks, the next list
    sa, lcp, rank = st.sa.copy(), st.lcp.copy(), st.rank.copy()
    head = ~same_prev | (K2 != Kp)
    sa[slot] = v2
    cut = head & same_prev
    lcp[slot[cut]] = l_new[cut]
    head_of = slot[np.maximum.accumulate(np.where(head, np.arange(m), 0))]
    rank[v2] = head_of + 1
    keep = ~(head & np.concatenate([head[1:], [True]]))
    out = State(sa, lcp, rank, slot[keep], head_of[keep])
    left = int(keep.sum())
    return out, left < m - m // 8, (0 if hint == NONE else hint), per_attempts


# ---- one hook call ---------------------------------------------------------------------------------------------------------------
def model(text, st, h, which, arg, bug=None):
    """what nolzss_debug_repeat_pass must return for the state: {"sa", "lcp", "rank", "new_slot", "new_grp", "new_m",
    "counts", "ret", "per_hint", "per_attempts"} and "branches", what ran"""
    branches = set()
    counts = count_large(st, RUN_MAX, bug) if st.slot.size else [0, 0, 0, 0]
    ret, hint, attempts = False, 0, 0
    out = st
    if which == PERIODIC:
        attempts = arg
        if st.slot.size:
            out, ret, hint, attempts = periodic_pass(text, st, h, arg, counts, bug, branches)
    elif which == PAIR_RUNS:
        for _ in range(arg):
            if out.slot.size == 0:
                break
            out, _progress = pair_run_pass(out, bug, branches)
    u32 = lambda x: np.asarray(x, dtype=np.int64).astype(np.uint32)  # noqa: E731
    return {"sa": u32(out.sa), "lcp": u32(out.lcp), "rank": u32(out.rank), "new_slot": u32(out.slot), "new_grp": u32(out.grp),
            "new_m": int(out.slot.size), "counts": counts, "ret": bool(ret), "per_hint": int(hint), "per_attempts": int(attempts),
            "branches": branches}


# ---- the model-independent property ----------------------------------------------------------------------------------------------
def check_refinement(truth, before, got, where=""):
    """what every output must be, whatever the passes do inside: a refinement of the state that went in.  Each group (by
    the decided LCP entries) holds exactly the suffixes of the same slots of the true suffix array, every decided LCP
    entry is the true one, every entry that was decided before still is, ranks are head slot + 1, and the list holds
    exactly the slots of the groups of two and more, in slot order, with their head slots."""
    sa_t, lcp_t = truth
    n = sa_t.size
    sa, lcp, rank = (np.asarray(got[k]).astype(np.int64) for k in ("sa", "lcp", "rank"))
    assert sa.size == n and lcp.size == n + 1 and rank.size == n, where
    assert lcp[n] == before.lcp[n], (where, "lcp[n] was written")
    dec = lcp[:n] < PENDING_MIN
    was = before.lcp[:n] < PENDING_MIN
    assert dec[was].all() and np.array_equal(lcp[:n][was], before.lcp[:n][was]), (where, "a decided entry changed")
    wrong = np.nonzero(dec & (lcp[:n] != lcp_t[:n]))[0]
    assert wrong.size == 0, (where, "decided LCP entries that are not true", wrong[:8].tolist(), lcp[wrong[:8]].tolist(), lcp_t[wrong[:8]].tolist())
    still = ~dec
    assert np.array_equal(lcp[:n][still], before.lcp[:n][still]), (where, "a pending code changed into another")
    hs = _heads_of(lcp, n)
    a, b = sa[np.lexsort((sa, hs))], sa_t[np.lexsort((sa_t, hs))]
    wrong = np.nonzero(a != b)[0]
    assert wrong.size == 0, (where, "groups that are no ranges of the true suffix array", hs[wrong[:8]].tolist())
    assert np.array_equal(rank[sa], hs + 1), (where, "ranks that are not head slot + 1")
    slot, grp = _listed(lcp, n)
    assert got["new_m"] == slot.size and np.array_equal(got["new_slot"], slot) and np.array_equal(got["new_grp"], grp), (where, "the list")


# ---- (c) the inputs ----------------------------------------------------------------------------------------------------------------
def rnd(k, seed, alphabet=b"ACGT"):
    rng = np.random.default_rng(seed)
    return bytes(np.frombuffer(bytes(alphabet), dtype=np.uint8)[rng.integers(0, len(alphabet), k)])


def unit(k, seed, alphabet=b"ACGT"):
    """a primitive word of k symbols (no shorter period, and not all one letter unless k == 1)"""
    for s in range(seed, seed + 1000):
        u = rnd(k, s, alphabet)
        if k == 1 or all(u != u[d:] + u[:d] for d in range(1, k)):
            return u
    raise ValueError("no primitive word")


A16 = b"ACGTBDEFHIKLMNPQ"            # 4 bits per symbol
A40 = bytes(range(48, 88))           # 8 bits per symbol

Case = namedtuple("Case", "name make h which arg orders deeper code lcp_n bits note")
_CASES = {}


def case(name, make, h, which, arg=0, orders=("text",), deeper=0.0, code="pending", lcp_n=PENDING, bits=2, note=""):
    assert name not in _CASES
    _CASES[name] = Case(name, make, h, which, arg, orders, deeper, code, lcp_n, bits, note)


def _copies(k, length, seed, tails=None, alphabet=b"ACGT"):
    """k copies of one word, each behind a random spacer; tails[j]: what follows copy j (default: nothing in common)"""
    def make():
        x = rnd(length, seed, alphabet)
        out = b""
        for j in range(k):
            out += rnd(7 + j % 3, seed + 100 + j, alphabet) + x + (tails[j] if tails else b"")
        return out + rnd(9, seed + 99, alphabet)
    return make


def _periodic(periods, seed, reps=30, alphabet=b"ACGT", tail=b"", flank=40):
    """runs of `reps` periods of a fresh unit per period length, between random flanks; every second run is followed by
    the symbol that makes it break upwards, the others by the lowest one"""
    def make():
        out = b""
        for j, p in enumerate(periods):
            u = unit(p, seed + 10 * j, alphabet)
            brk = bytes([max(alphabet)]) if j % 2 else bytes([min(alphabet)])
            out += rnd(flank, seed + 10 * j + 1, alphabet) + u * reps + u[:j % max(p, 1)] + brk
        return out + rnd(flank, seed + 5, alphabet) + tail
    return make


def _build_cases():
    P, Q, Z = PAIR_RUNS, PERIODIC, COUNTS
    all3 = ORDERS
    # ---- pair runs
    perm = bytes(np.random.default_rng(1).permutation(np.arange(40, 240)).astype(np.uint8))
    case("pr_xx_deferred", lambda: perm + perm, 1, P, 1, all3, bits=8, note="XX, every symbol of X once: the run ends with the text, everything is deferred")
    case("pr_xx_deferred_3", lambda: perm + perm, 1, P, 3, ("shuffle",), bits=8, note="... and stays so over three passes")
    case("pr_xxc", lambda: perm + perm + b"\x01", 1, P, 1, all3, bits=8, note="XX and one more symbol: finished from the end")
    case("pr_xx_dna", lambda: rnd(300, 2) * 2, 20, P, 1, all3, note="XX of DNA at depth 20: the run ends where the groups end")
    case("pr_xyx", lambda: rnd(250, 3) + rnd(90, 4) + rnd(250, 3) + rnd(20, 5), 14, P, 1, all3, note="XYX")
    x, p = rnd(120, 6), rnd(60, 7)
    three = lambda: rnd(11, 8) + x + p + b"A" + rnd(13, 9) + x + p + b"C" + rnd(9, 10) + x + b"G" + rnd(15, 11)  # noqa: E731
    for passes in (1, 2, 3):
        case(f"pr_three_{passes}", three, 12, P, passes, all3 if passes == 1 else ("shuffle",),
             note="three copies, one differs behind the run: a pass splits 3 into 2 + 1, the next finishes the pairs")
    for k in (2, 3, 15, 16, 17):
        case(f"pr_copies_{k}", _copies(k, 48, 20 + k), 12, P, 2, ("text", "shuffle"), note=f"{k} copies" + (": nothing may change" if k == 17 else ""))
    w = rnd(200, 30)
    case("pr_nested", lambda: rnd(30, 31) + w + rnd(25, 32) + w[80:] + rnd(33, 33) + w[:120] + rnd(21, 34), 12, P, 3, all3,
         note="copies A, B = W[80:], C = W[:120]: the group size and the link distance change mid-run")
    v = rnd(70, 35)
    case("pr_overlap", lambda: rnd(20, 36) + v + v[:50] + v[10:] + rnd(15, 37) + v[30:] + v + rnd(10, 38), 10, P, 4, all3,
         note="overlapping repeats")
    pp, qq = rnd(80, 40), rnd(80, 41)
    case("pr_partly", _copies(4, 60, 42, [pp + b"A", pp + b"C", qq + b"G", qq + b"T"]), 12, P, 1, all3,
         note="the end group of four separates into two classes of two that stay tied")
    case("pr_partly_3", _copies(4, 60, 42, [pp + b"A", pp + b"C", qq + b"G", qq + b"T"]), 12, P, 3, ("reversed",))
    tails16 = [(pp if j % 2 else qq) + rnd(5, 50 + j) for j in range(16)]
    case("pr_16_splits", lambda: _copies(16, 40, 43, tails16)() + _copies(3, 50, 44)(), 12, P, 2, ("text", "shuffle"),
         note="a group of exactly 16 that splits into classes of 8, next to other groups")
    tails17 = [(pp if j % 2 else qq) + rnd(5, 50 + j) for j in range(17)]
    case("pr_17_splits", lambda: _copies(17, 40, 43, tails17)() + _copies(3, 50, 44)(), 12, P, 2, ("shuffle",),
         note="17: left alone; the classes of 9 and 8 behind the run are taken")
    case("pr_only_large", lambda: b"".join(bytes([100 + j]) + rnd(30, 45, A16) for j in range(20)) + b"\x7f", 10, P, 2, ("shuffle",),
         bits=8, note="20 copies between symbols that occur once: only groups of more than 16, nothing may change")
    mut = lambda: _mutated(1500, 46)  # noqa: E731
    case("pr_mixed_depth", mut, 10, P, 3, all3, deeper=0.5, note="mutated copies, half the groups refined to deeper depths")
    case("pr_compared", mut, 12, P, 2, ("shuffle",), deeper=0.3, code="mixed", lcp_n=0, note="kLcpPendingCompared inside groups")
    case("pr_compared_all", _copies(3, 48, 47), 12, P, 1, ("reversed",), code="compared", lcp_n=12345)
    case("pr_w4", _copies(5, 60, 48, alphabet=A16), 6, P, 4, all3, bits=4, note="4 bits per symbol")
    case("pr_w8", _copies(6, 60, 49, alphabet=A40), 4, P, 5, all3, bits=8, note="8 bits per symbol")
    case("pr_periodic_text", _periodic((2, 5), 50, reps=12), 4, P, 2, ("shuffle",), deeper=0.4,
         note="a periodic text under the pair-run pass: chains of groups whose members lie a period apart")
    # ---- periodic runs
    for per in (1, 2, 3, 7, 23):
        case(f"per_p{per}", _periodic((per, per, per), 60 + per, tail=unit(per, 99 + per) * 25), 17 if per < 23 else 20, Q, 1, all3,
             note=f"period {per}: a run that breaks downwards, one that breaks upwards, one at the end of the text")
    u5 = unit(5, 70)
    case("per_two_runs", lambda: rnd(40, 71) + u5 * 30 + b"A" + rnd(40, 72) + u5 * 22 + b"T" + rnd(30, 73), 17, Q, 1, all3,
         note="two runs of one unit in one group: members whose link is not q")
    u7 = unit(7, 74)
    seven = lambda: rnd(60, 75) + u7 * 25 + b"C" + rnd(60, 76)  # noqa: E731
    case("per_q_eq_depth", seven, 7, Q, 1, all3, note="q == depth")
    case("per_q_depth_plus_1", seven, 6, Q, 1, all3, note="q == depth + 1: taken because the text confirms it")
    for qq_ in (4096, 4097):
        uq = rnd(qq_, 77)
        case(f"per_q{qq_}", lambda uq=uq: rnd(30, 78) + b"AC" * 450 + b"G" + rnd(30, 178) + uq * 3, 17, Q, 1, ("shuffle",),
             note="three periods of %d up to the end of the text (and 900 members of a short period, for the candidate gate): %s"
                  % (qq_, "taken, confirmed by the runs of positions" if qq_ == 4096 else "flagged, the hint is 4097"))
    case("per_q4096_tail", lambda: rnd(4096, 77) * 3 + rnd(50, 78), 17, Q, 1, ("shuffle",),
         note="... and random symbols behind them: the middle copies agree with the last on fewer than q symbols, flagged by the run check")
    sh = rnd(30, 79)
    uu, vv, vw = sh + rnd(11, 80), sh + rnd(11, 81), sh + rnd(14, 181)
    case("per_lookalike", lambda: rnd(30, 82) + uu * 40 + vv * 40 + rnd(30, 83), 17, Q, 1, all3,
         note="U^40 V^40, U and V alike on 30 symbols and equally long: the pairs that join the runs are q apart and fail the run check")
    case("per_lookalike_len", lambda: rnd(30, 82) + uu * 40 + vw * 40 + rnd(30, 83), 17, Q, 1, all3,
         note="... with |V| = |U| + 3: the pairs that join the runs go through the text check")
    case("per_tied_E", lambda: rnd(20, 84) + b"AAAAAC" * 30 + rnd(20, 85), 3, Q, 1, all3,
         note="period 6 at depth 3: E and E + q both start with AAA, tied with each other in a group of period 1")
    case("per_tied_E_q_le_depth", lambda: rnd(20, 184) + b"AACG" * 15 + rnd(20, 185) + b"ACG" * 10 + rnd(20, 186), 4, Q, 1, all3,
         note="... with q = 4 = depth: the run of AACG ends at ACGA, which is tied with the ACGA four behind it in a group that "
              "the run of ACG gives the period 3 -- no other check would stop the group")
    case("per_short_run", lambda: rnd(250, 3) + rnd(90, 4) + rnd(250, 3) + rnd(20, 5), 14, Q, 1, ("shuffle",),
         note="XYX: pairs q = 340 apart that agree on fewer than q symbols -- the run check of per_rho_kernel flags them")
    case("per_text_end", lambda: rnd(40, 86) + unit(9, 87) * 20 + unit(9, 87)[:4], 17, Q, 1, all3,
         note="the text ends inside a period")
    case("per_text_end_q_gt", lambda: rnd(40, 86) + unit(30, 88) * 6 + unit(30, 88)[:11], 17, Q, 1, all3,
         note="... with q > depth: members without a next member and E + q > n")
    case("per_link_paths", lambda: b"A" * 700 + rnd(30, 89) + b"CG" * 180 + rnd(30, 90) + unit(3, 91) * 40 + b"T" + rnd(50, 92), 17, Q, 1,
         ("text", "shuffle"), note="groups of 684 and of 2 x 172 members and small ones: block, wavefront and mixed reductions of per_link_kernel")
    for m_ in (255, 256, 257):
        case(f"per_m{m_}", lambda m_=m_: b"A" * (m_ + 16) + b"C", 17, Q, 1, ("reversed",), note=f"a list of {m_} entries")
    case("per_first_gate", lambda: rnd(300, 2) * 2, 20, Q, 0, ("shuffle",), note="the first call on pairs: in_large < m / 8, never again")
    case("per_first_pass", _periodic((1, 4), 93, reps=60), 17, Q, 0, ("shuffle",), note="the first call passes its gate")
    far = lambda extra: rnd(1000, 94) + rnd(3200, 95) + rnd(1000, 94) + rnd(20, 96) + extra  # noqa: E731
    case("per_cand_none", lambda: far(b""), 17, Q, 1, ("shuffle",), note="pairs 4200 apart only: cand = 0 < m / 16, skipped")
    case("per_cand_between", lambda: far(b"AC" * 100 + b"A"), 17, Q, 1, ("shuffle",), note="m / 16 <= cand < m / 8: the pass runs")
    case("per_attempts_3", _periodic((3,), 97), 17, Q, 3, ("text",), note="per_attempts already 3")
    case("per_mixed_depth", _periodic((1, 2, 6, 11), 98, reps=40), 8, Q, 1, all3, deeper=0.6, code="mixed",
         note="the second call: groups refined to mixed depths, compared codes")
    case("per_w4", _periodic((1, 3, 10), 101, alphabet=A16), 8, Q, 1, all3, bits=4)
    case("per_w8", _periodic((2, 5, 9), 102, alphabet=A40), 4, Q, 1, all3, bits=8)
    seg = lambda: (rnd(40, 103) + unit(7, 104) * 20 + b"N" + rnd(30, 105) + unit(8, 106) * 20 + b"#" + unit(2, 107) * 30 + b"$"  # noqa: E731
                   + rnd(25, 108) + unit(7, 104) * 12 + b"%" + rnd(20, 109))
    case("per_segmented", seg, 7, Q, 1, all3, note="terminators: no text check, qmax = depth; period 7 taken, period 8 flagged with the hint 8")
    case("per_big", lambda: b"A" * (1 << 20) + b"C" + b"A" * 299, 17, Q, 1, ("shuffle",),
         note="n = 2^20 + 300, closed-form arrays: the stride loops of the list kernels")
    # ---- counts
    case("cnt_16", _copies(16, 30, 110), 12, Z, note="groups of 16")
    case("cnt_17", _copies(17, 30, 111), 12, Z, note="groups of 17")
    for dist in (4096, 4097):
        xx = rnd(100, 112)
        case(f"cnt_near_{dist}", lambda dist=dist, xx=xx: xx + rnd(dist - 100, 113) + xx + rnd(10, 114), 17, Z, orders=("text", "reversed"),
             note=f"neighbours {dist} apart")


def _mutated(n, seed):
    """copies of a few words with point mutations, in random order"""
    rng = np.random.default_rng(seed)
    words = [rnd(int(rng.integers(30, 120)), seed + 1 + j) for j in range(4)]
    out = bytearray()
    while len(out) < n:
        wd = bytearray(words[int(rng.integers(4))])
        for _ in range(int(rng.integers(0, 3))):
            wd[int(rng.integers(len(wd)))] = b"ACGT"[int(rng.integers(4))]
        out += wd + rnd(int(rng.integers(0, 4)), int(rng.integers(1 << 30)))
    return bytes(out[:n])


_build_cases()
CASES = _CASES


@functools.lru_cache(maxsize=None)
def made(name):
    """-> (Text, (true sa, true lcp)), built once and shared, never written"""
    data = CASES[name].make()
    text = Text(data)
    assert text.bits == CASES[name].bits, (name, text.bits)
    if name == "per_big":
        truth = true_arrays_apcaq(1 << 20, 299)
    else:
        truth = true_arrays(text)
    for a in truth:
        a.setflags(write=False)
    return text, truth


@functools.lru_cache(maxsize=None)
def state(name, order):
    c = CASES[name]
    text, truth = made(name)
    st = build_state(text, truth, c.h, order, c.deeper, c.code, c.lcp_n, seed=len(name) + ORDERS.index(order))
    for a in st:
        a.setflags(write=False)
    return st


def runs():
    return [(name, order) for name in CASES for order in CASES[name].orders]


@functools.lru_cache(maxsize=None)
def expected(name, order):
    """the model's answer, computed once and shared among the tests that need it"""
    c = CASES[name]
    return model(made(name)[0], state(name, order), c.h, c.which, c.arg)


def expected_with(name, order, bug):
    """the same with a mistake switched on; None where the mistake spoils the state of a pass so far that the next one
    cannot be modelled (two suffixes in one slot, a place behind the array)"""
    c = CASES[name]
    try:
        return model(made(name)[0], state(name, order), c.h, c.which, c.arg, bug)
    except (AssertionError, IndexError):
        assert bug is not None
        return None
