"""The greedy cursor on arbitrary length codes (chain.hip) and the widening of 16-bit codes (lpnf.hip: widened_lstar) in
plain numpy / Python -- TEST INFRASTRUCTURE ONLY.  Three things:

  * (a) the definition (cursor): the reference's cursor, lambda = next_leaf(lambda, l)
    (/root/reference/src/cpp/factorizer_core.hpp:113-115, restated in the header of chain.hip), over a bare code array:
    p = start_pos; while p < n: mark(p); p += max(1, code[p] & 0x7fffffff) -- and what follows from the marks (expected):
    z, the ascending starts, the lengths, the histogram with its tail, the counts per range; the widening (widen);
  * (b) a stage-level restatement of what the kernels are documented to do (staged): exits per 4096-position tile by
    pointer doubling, the distinct exit targets with their duplicate suppression, the node list, its edges, the Wyllie
    rounds with the reached flag, the tile entries, the walk per entered tile.  Without a `bug` it must give the marks
    of (a); `bug` switches one named mistake on, so that tests/test_chain_model_host.py can show which input is there
    for which mistake;
  * the inputs (CASES, by family in FAMILIES) of tests/test_gpu_chain_direct.py.
"""
import functools
from collections import namedtuple

import numpy as np

TILE = 4096            # kTile
T = 2048               # kLengthHistBins
MASK = 0x7fffffff      # kLenMask
FLAG = 0x80000000
NONE = 0xffffffff      # kNone
NARROW_TOP = 0xfffe    # the largest code the 16-bit form of the cursor takes
MAX_N = 33 * TILE + 1  # no input is larger
POISONS = (0x0000, 0xffff)
BUGS = ("no_mask", "narrow_exit_full_tile", "odd_second_dropped", "last_target_dropped", "start_no_node",
        "wyllie_round_short", "eleven_rounds", "widen_last_wins", "dense_T", "mark_full_tile_end")


# ---- (a) the definition ------------------------------------------------------------------------------------------------------
def cursor(codes, start_pos):
    """the marked positions, ascending"""
    code = [int(c) for c in codes]
    n, p, marks = len(code), start_pos, []
    while p < n:
        marks.append(p)
        p += max(1, code[p] & MASK)
    return np.array(marks, dtype=np.uint32)


def widen(narrow, items, listed, bug=None):
    """wide[i] = max(narrow[i], the first `listed` entries (position | code << 32) whose position is i and < n)"""
    wide = np.array(narrow, dtype=np.uint32)
    for e in [int(x) for x in items[:listed]]:
        i, c = e & 0xffffffff, e >> 32
        if i < wide.size:
            wide[i] = c if bug == "widen_last_wins" else max(int(wide[i]), c)
    return wide


def outputs(codes, starts, with_strand, bounds=None, bug=None):
    """what the length kernels and the per-range count make of the marks"""
    codes = np.asarray(codes, dtype=np.uint32)
    c = codes[starts].astype(np.uint64)
    length = np.maximum(c & np.uint64(MASK), np.uint64(1))
    strand = (c >> np.uint64(31)) if with_strand else np.zeros_like(c)
    dense = length <= T if bug == "dense_T" else length < T
    bins = 2 * T if with_strand else T
    hist = np.bincount((strand * np.uint64(T) + length)[dense].astype(np.int64), minlength=bins + 1)[:bins].astype(np.uint32)
    tail = np.sort((length | (strand << np.uint64(32)))[~dense])
    out = {"z": int(starts.size), "starts": starts, "lengths": length.astype(np.uint32), "hist": hist, "tail": tail,
           "counts": None}
    if bounds is not None:
        b = np.asarray(bounds, dtype=np.int64).reshape(-1, 2)
        out["counts"] = np.array([np.count_nonzero((starts >= lo) & (starts < hi)) for lo, hi in b], dtype=np.uint32)
    return out


# ---- (b) the stages ----------------------------------------------------------------------------------------------------------
def staged(codes, start_pos, width=32, bug=None):
    """-> {"starts", "K" (nodes), "rounds" (Wyllie), "exit_rounds" (doubling rounds that moved a pointer), "entries"}"""
    codes = np.asarray(codes, dtype=np.uint32)
    n = codes.size
    empty = {"starts": np.zeros(0, dtype=np.uint32), "K": 0, "rounds": 0, "exit_rounds": 0, "entries": 0}
    if start_pos >= n:
        return empty
    p = np.arange(n, dtype=np.int64)
    length = codes.astype(np.int64) & (0xffffffff if bug == "no_mask" else MASK)
    nxt = np.minimum(p + np.maximum(length, 1), n)
    if bug == "odd_second_dropped" and width == 16 and n % 2 and n >= 2:
        nxt[n - 2] = n  # the last full pair of an odd text loses its second half
    base = p // TILE * TILE
    tile_end = np.minimum(base + TILE, n)
    # 1. chain_exit_kernel: pointer doubling inside the tile, twelve rounds at the most (2^12 positions)
    own, exit_rounds = nxt.copy(), 0
    for _ in range(11 if bug == "eleven_rounds" else 12):
        inside = own < tile_end
        if not inside.any():
            break
        jump = np.append(own, n)
        own = np.where(inside, jump[own], own)
        exit_rounds += 1
    last = (p % TILE == TILE - 1) | (p + 1 >= n)
    same_next = np.append(own[1:] == own[:-1], False)
    record = (own < n) & (last | ~same_next)
    if bug == "last_target_dropped":
        same_prev = np.append(False, own[1:] == own[:-1]) & (p % TILE != 0)
        record &= ~(last & same_prev)
    bits = np.zeros(n + 1, dtype=bool)
    bits[own[record]] = True
    if bug != "start_no_node":
        bits[start_pos] = True
    # 2. the node list and its edges; node_id is a rank in the bitmap, whatever the bit of the position says
    node_pos = np.nonzero(bits)[0]
    K = node_pos.size
    ex = own[node_pos]
    if width == 16:  # the exit travels as a half-word, counted from the end of the node's tile
        stored_from = (base + TILE if bug == "narrow_exit_full_tile" else tile_end)[node_pos]
        ex = ((ex - stored_from) & 0xffff) + tile_end[node_pos]
    nx = np.append(np.where(ex >= n, K, np.searchsorted(node_pos, ex)), K)
    reach = np.append(node_pos == start_pos, False)
    rounds = 1
    while (1 << rounds) < K + 1:
        rounds += 1
    if bug == "wyllie_round_short":
        rounds -= 1
    # 3. wyllie_kernel: (the device's races on the flag only add true chain nodes; here every round reads the last one's flags)
    for _ in range(rounds):
        w = nx[:K]
        live = w < K
        flagged = w[live & reach[:K]]
        nx[:K] = np.where(live, nx[w], K)
        reach[flagged] = True
    entry = np.full((n + TILE - 1) // TILE, NONE, dtype=np.int64)
    for q in node_pos[reach[:K]]:  # (in a race of two nodes of one tile the later one is taken here)
        entry[q // TILE] = q
    # 4. chain_mark_kernel: one walk per entered tile
    step, marks = nxt.tolist(), []
    for t in np.nonzero(entry != NONE)[0]:
        q, end = int(entry[t]), min((int(t) + 1) * TILE, n)
        if bug == "mark_full_tile_end":
            end = (int(t) + 1) * TILE
        while q < end:
            marks.append(q)
            if q >= n:
                break
            q = step[q]
    return {"starts": np.array(marks, dtype=np.uint32), "K": int(K), "rounds": rounds, "exit_rounds": exit_rounds,
            "entries": int(np.count_nonzero(entry != NONE))}


# ---- the inputs --------------------------------------------------------------------------------------------------------------
# codes: what the hook is given (widening: the narrow codes); compare: "all", or "starts" (z and the starts only: a code
# that runs past n is returned raw by the length kernels, which is no contract); widening: (items, listed, list_max)
Case = namedtuple("Case", "family codes start with_strand compare widening bounds")


def _case(family, codes, start=0, with_strand=False, compare="all", widening=None, bounds=None):
    codes = np.ascontiguousarray(codes, dtype=np.uint32)
    assert codes.size <= MAX_N
    return Case(family, codes, int(start), with_strand, compare, widening, bounds)


def clipped(codes):
    codes = np.asarray(codes, dtype=np.int64)
    return np.minimum(codes, codes.size - np.arange(codes.size))


@functools.lru_cache(maxsize=None)
def realistic(n, seed):
    """copies of random lengths (geometric, heavy tail up to 20 000) laid over literals as ramps: code[i + 1] >= code[i] - 1"""
    rng = np.random.default_rng(seed)
    code = np.zeros(n, dtype=np.int64)
    m = max(1, n // 24)
    where = rng.integers(0, n, m)
    lens = rng.geometric(1 / 24, m)
    heavy = rng.random(m) < 0.004
    lens[heavy] = (200 * 100 ** rng.random(int(heavy.sum()))).astype(np.int64)  # 200 .. 20 000, log-uniform
    lens[0] = 20000
    for i, l in zip(where.tolist(), lens.tolist()):
        l = min(l, n - i)
        code[i:i + l] = np.maximum(code[i:i + l], l - np.arange(l))
    return clipped(code)


def uniform(n, lo, hi, seed):
    return clipped(np.random.default_rng(seed).integers(lo, hi + 1, n))


def with_flags(codes, seed):
    """bit 31 on a random half of the non-zero codes, never on a zero"""
    codes = np.asarray(codes, dtype=np.int64)
    on = (np.random.default_rng(seed).random(codes.size) < 0.5) & (codes != 0)
    return codes | (on.astype(np.int64) << 31)


def planted(n, plants):
    """hand-placed codes on a background of literals"""
    code = np.zeros(n, dtype=np.int64)
    for i, c in plants:
        code[i] = c
    return code


SIZES = (1, 2, 3, 63, 64, 65, 4095, 4096, 4097, 8191, 8192, 8193, 3 * TILE + 1)


def starts_for(n):
    """0, 1, 2, 4095, 4096, 4097, an odd position inside, n - 1 where they lie inside; then n and n + 5"""
    inside = sorted({s for s in (0, 1, 2, 4095, 4096, 4097, (n // 3) | 1, n - 1) if 0 <= s < n})
    return inside + [n, n + 5]


TILE_COUNTS = (1, 3, 4, 7, 8, 15, 16, 31, 32)
WIDEN_KINDS = ("one", "two_small_first", "two_large_first", "beyond_n", "listed_short", "listed_zero")


def _widening(n, list_max, kind):
    rng = np.random.default_rng(1000 * n + list_max)
    if n >= TILE and list_max < n:  # clipped codes, of which many reach the saturation value
        true = realistic(n, 5).copy()
        compare = "all"
    else:  # the saturated codes run past n
        true = realistic(n, 5).copy() if n >= TILE else rng.integers(0, 4, n)
        for i in sorted({0, n // 2, n - 1} if n < TILE else {5, TILE - 1, TILE, n - 1}):
            true[i] = list_max + 1 + 3 * i
        compare = "starts"
    sat = np.nonzero(true >= list_max)[0]
    narrow = np.minimum(true, list_max)
    entry = lambda i, c: int(i) | (int(c) << 32)  # noqa: E731
    one = [entry(i, true[i]) for i in rng.permutation(sat)]
    items, listed = one, None
    if kind == "two_small_first":
        items = [e for i in sat for e in (entry(i, list_max), entry(i, true[i]))]
    elif kind == "two_large_first":
        items = [e for i in sat for e in (entry(i, true[i]), entry(i, list_max))]
    elif kind == "beyond_n":
        items = one[:1] + [entry(n, 777), entry(n + 7, 99)] + one[1:] + [entry(0xffffffff, 5)]
    elif kind == "listed_short":  # the entries behind `listed` would raise two saturated codes and one that is not
        other = int(np.nonzero(true < list_max)[0][0]) if (true < list_max).any() else int(sat[0])
        items, listed = one + [entry(i, true[i] + 1000) for i in sat[:2]] + [entry(other, 5000)], len(one)
    elif kind == "listed_zero":
        listed = 0
    items = np.array(items, dtype=np.uint64)
    return _case("widening", narrow, 0, compare=compare,
                 widening=(items, len(items) if listed is None else listed, list_max))


def _ranges(kind):
    codes = realistic(5 * TILE + 1, 11)
    n, s = codes.size, cursor(codes, 0).astype(np.int64)
    a = int(s[3])
    marked = set(s.tolist())
    q = next(x for x in range(a + 1, n) if x not in marked)  # a position inside a factor
    b = int(s[s > q + 1][4])
    bounds = {"k0": [], "whole": [(0, n)], "touching": [(0, b), (b, n)],
              "mixed": [(0, 0), (a, a + 1), (q, q + 1), (b, b), (b, n), (n, n)]}[kind]
    return _case("ranges", codes, 0, bounds=np.array(bounds, dtype=np.uint32).reshape(-1))


def _builders():
    b = {}
    for n in SIZES:
        for s in starts_for(n):
            b[f"size_{n}_s{s}"] = lambda n=n, s=s: _case("sizes", realistic(n, 3), s)
    for tiles in TILE_COUNTS:
        for plus in (0, 1):
            for name, value in (("lit", 0), ("ones", 1)):
                b[f"{name}_t{tiles}_p{plus}"] = lambda t=tiles, p=plus, v=value: _case("literals", np.full(t * TILE + p, v))
    b["const_2_even"] = lambda: _case("constant", clipped(np.full(2 * TILE + 3, 2)), 0)
    b["const_2_odd"] = lambda: _case("constant", clipped(np.full(2 * TILE + 3, 2)), 1)
    for L in (4095, 4096, 4097):
        for s in (0, 1):
            b[f"const_{L}_s{s}"] = lambda L=L, s=s: _case("constant", clipped(np.full(9 * TILE, L)), s)
    # tile seams: the chain walks the literals of tile 0 to its last position, or enters tile 1 at offset 0
    for c in (1, TILE + 1, 2 * TILE + 1):
        b[f"seam_4095_c{c}"] = lambda c=c: _case("seams", planted(4 * TILE + 5, [(TILE - 1, c)]))
    for c in (TILE, 3 * TILE):
        b[f"seam_0_c{c}"] = lambda c=c: _case("seams", planted(6 * TILE, [(TILE, c)]))
    for at in (TILE - 1, TILE):
        target = at + NARROW_TOP
        b[f"seam_fffe_from{at}"] = lambda at=at: _case("seams", planted(18 * TILE, [(at, NARROW_TOP)]))
        b[f"seam_fffe_from{at}_partial"] = lambda at=at, t=target: _case("seams", planted(t + 1, [(at, NARROW_TOP)]))
    b["seam_whole_16"] = lambda: _case("seams", planted(2 * TILE + 7, [(3, 2 * TILE + 4)]), 3)
    b["seam_whole_32"] = lambda: _case("seams", planted(17 * TILE + 1, [(0, 17 * TILE + 1)]), 0)
    for n in (5 * TILE + 1, 20 * TILE + 4097):
        for seed in (1, 2, 3):
            for s in (0, 4097):
                b[f"real_{n}_seed{seed}_s{s}"] = lambda n=n, seed=seed, s=s: _case("realistic", realistic(n, seed), s)
    for n in (5 * TILE + 1, 12 * TILE + 3):
        for lo, hi in ((0, 8), (0, 5000), (TILE, 2 * TILE - 1), (0, NARROW_TOP)):
            for s in (0, 1):
                b[f"adv_{n}_{lo}_{hi}_s{s}"] = lambda n=n, lo=lo, hi=hi, s=s: _case("adversarial", uniform(n, lo, hi, n + hi), s)
    for n in (5 * TILE + 1, 20 * TILE + 4097):
        b[f"strand_real_{n}"] = lambda n=n: _case("strand", with_flags(realistic(n, 2), 7), 0, with_strand=True)
    for n in (5 * TILE + 1, 12 * TILE + 3):
        b[f"strand_adv_{n}"] = lambda n=n: _case("strand", with_flags(uniform(n, 0, 5000, n), 8), 1, with_strand=True)
    # lengths at the boundary of the dense bins: every code of the chain is the factor's length, literals elsewhere
    for n in (8 * T, 8 * T + 1):
        for name, cycle in (("2047", (T - 1,)), ("2048", (T,)), ("alt", (T - 1, T, 1))):
            def build(n=n, cycle=cycle):
                plants, q, k = [], 0, 0
                while q < n:
                    c = min(cycle[k % len(cycle)], n - q)
                    plants.append((q, c))
                    q, k = q + c, k + 1
                return _case("bins", planted(n, plants))
            b[f"bins_{name}_n{n}"] = build
    b["overshoot_32"] = lambda: _case("overshoot", planted(TILE + 9, [(TILE + 7, 0xffffffff)]), 0, with_strand=True, compare="starts")
    b["overshoot_32_sum"] = lambda: _case("overshoot", planted(2 * TILE + 1, [(2 * TILE - 1, MASK)]), 1, compare="starts")
    b["overshoot_16"] = lambda: _case("overshoot", planted(TILE + 9, [(TILE + 6, NARROW_TOP)]), 0, compare="starts")
    for n in (1, 2, 7, 4097):
        for list_max in (0xffff, 64):
            for kind in WIDEN_KINDS:
                b[f"widen_{n}_m{list_max}_{kind}"] = lambda n=n, m=list_max, kind=kind: _widening(n, m, kind)
    for kind in ("k0", "whole", "touching", "mixed"):
        b[f"ranges_{kind}"] = lambda kind=kind: _ranges(kind)
    return b


CASES = _builders()


@functools.lru_cache(maxsize=None)
def case(name):
    return CASES[name]()


FAMILY_NAMES = ("sizes", "literals", "constant", "seams", "realistic", "adversarial", "strand", "bins", "overshoot",
                "widening", "ranges")
_PREFIX = {"size": "sizes", "lit": "literals", "ones": "literals", "const": "constant", "seam": "seams", "real": "realistic",
           "adv": "adversarial", "strand": "strand", "bins": "bins", "overshoot": "overshoot", "widen": "widening",
           "ranges": "ranges"}
FAMILIES = {f: [name for name in CASES if _PREFIX[name.split("_")[0]] == f] for f in FAMILY_NAMES}


def widths_of(name):
    """every case runs with 32-bit codes, and with 16-bit codes wherever they all lie below 0xffff and none carries the
    strand; the widening runs from 16-bit codes only"""
    c = case(name)
    if c.widening is not None:
        return (16,)
    return (32, 16) if int(c.codes.max(initial=0)) <= NARROW_TOP else (32,)


def cursor_codes(name, bug=None):
    """the array the cursor runs on: the case's codes, or their widened form"""
    c = case(name)
    return c.codes if c.widening is None else widen(c.codes, c.widening[0], c.widening[1], bug)


@functools.lru_cache(maxsize=None)
def expected(name, width=32, bug=None):
    """what nolzss_debug_chain must return for the case: from the definition, or with `bug` from the stages"""
    c = case(name)
    codes = cursor_codes(name, bug)
    if bug is None:
        starts = cursor(codes, c.start)
    else:
        starts = staged(codes, c.start, 32 if c.widening is not None else width, bug)["starts"]
    out = outputs(codes, starts[starts < codes.size], c.with_strand, c.bounds, bug)
    out.update(z=int(starts.size), starts=starts, widened=codes if c.widening is not None else None)
    return out


COMPARED = {"all": ("z", "starts", "lengths", "hist", "tail", "counts", "widened"), "starts": ("z", "starts", "counts", "widened")}


def differs(name, width, bug):
    """does the named mistake change something the GPU test compares on this case"""
    good, bad = expected(name, width), expected(name, width, bug)
    for key in COMPARED[case(name).compare]:
        if good[key] is None:
            continue
        if np.ndim(good[key]) == 0:
            if good[key] != bad[key]:
                return True
        elif not np.array_equal(good[key], bad[key]):
            return True
    return False
