"""The speculative cursor (chain.hip: chain_spec_walk_kernel, the tile path, chain_spec_fix_kernel, the fall-back of
mark_chain) in plain numpy / Python -- TEST INFRASTRUCTURE ONLY.  Two things:

  * staged(codes, start_pos, bug): a restatement of the three steps as they are documented -- 1. the walk of every tile
    from its first position (from start_pos in its tile) with its exit; 2. the path over the tiles by pointer doubling
    with a reached flag, and the entries it scatters; 3. the walk from the entry until it lands on a mark of step 1 --
    with the number of tiles that failed, and run(): the marks of step 3, or on a failure the definition
    (chain_model.cursor: what the exact stages deliver).  `bug` switches one named mistake on, so that
    tests/test_chain_spec_host.py can show which input is there for which mistake;
  * the inputs (CASES) of tests/test_gpu_chain_spec.py, each with the path it must take and the tiles that must fail,
    stated by hand.
"""
import functools
from collections import namedtuple

import numpy as np

import chain_model as M

TILE, MASK, NONE = M.TILE, M.MASK, M.NONE
MAX_N = 32 * TILE + 1  # no input is larger (131 073 positions)
BUGS = ("keep_below_m", "accept_any_exit", "follow_unreached")


def _next(codes):
    codes = np.asarray(codes, dtype=np.uint32)
    n = codes.size
    length = np.maximum(codes.astype(np.int64) & MASK, 1)
    return np.minimum(np.arange(n, dtype=np.int64) + length, n).tolist()


def staged(codes, start_pos, bug=None):
    """-> {"starts" (the marks behind step 3), "failed" (tiles), "reached" (tiles), "merges": {tile: (hops walked from
    the entry, offset of m in the tile or None: left the tile at the speculative exit)} of the reached tiles that were
    entered elsewhere than where step 1 began, "cleared" (marks of step 1 that step 3 took away)}"""
    n = len(codes)
    out = {"starts": np.zeros(0, dtype=np.uint32), "failed": 0, "reached": 0, "merges": {}, "cleared": 0}
    if start_pos >= n:
        return out
    nxt = _next(codes)
    nt = (n + TILE - 1) // TILE
    start_tile = start_pos // TILE
    # 1. the speculative walk
    spec = np.zeros(n, dtype=bool)
    ex = [n] * nt
    for t in range(start_tile, nt):
        end = min((t + 1) * TILE, n)
        p = max(start_pos, t * TILE)
        while p < end:
            spec[p] = True
            p = nxt[p]
        ex[t] = p
    # 2. the tile path: pointer doubling with a reached flag (every round reads the flags of the round before)
    hop = np.array([nt if e >= n else e // TILE for e in ex] + [nt], dtype=np.int64)
    reach = np.zeros(nt + 1, dtype=bool)
    reach[start_tile] = True
    rounds = 1
    while (1 << rounds) < nt + 1:
        rounds += 1
    for _ in range(rounds):
        w = hop[:nt]
        live = w < nt
        flagged = w[live & reach[:nt]]
        hop[:nt] = np.where(live, hop[w], nt)
        reach[flagged] = True
    entry = [NONE] * nt
    entry[start_tile] = start_pos
    for t in range(start_tile, nt):
        if (reach[t] or bug == "follow_unreached") and ex[t] < n:
            entry[ex[t] // TILE] = ex[t]
    # 3. the head fix
    final = np.zeros(n, dtype=bool)
    for t in range(nt):
        base, end = t * TILE, min((t + 1) * TILE, n)
        if entry[t] == NONE:
            continue
        out["reached"] += 1
        if entry[t] == max(start_pos, base):
            final[base:end] = spec[base:end]
            continue
        p, hops, mine = entry[t], 0, []
        while p < end and not spec[p]:
            mine.append(p)
            p = nxt[p]
            hops += 1
        final[mine] = True
        if p < end:  # landed on a mark: m = p
            lo = base if bug == "keep_below_m" else p
            final[lo:end] |= spec[lo:end]
            out["merges"][t] = (hops, p - base)
        else:
            if bug == "keep_below_m":
                final[base:end] |= spec[base:end]
            if p != ex[t] and bug != "accept_any_exit":
                out["failed"] += 1
            out["merges"][t] = (hops, None)
    out["starts"] = np.nonzero(final)[0].astype(np.uint32)
    out["cleared"] = int(np.count_nonzero(spec & ~final))
    return out


def run(codes, start_pos, bug=None):
    """what mark_chain delivers: (starts, path, failed tiles)"""
    if start_pos >= len(codes):
        return np.zeros(0, dtype=np.uint32), "none", 0
    st = staged(codes, start_pos, bug)
    if st["failed"]:
        return M.cursor(codes, start_pos), "failed_over", st["failed"]
    return st["starts"], "speculative", 0


# ---- the inputs --------------------------------------------------------------------------------------------------------------
# path / failed: what the call must report (stated here by hand; the host test holds the model against them)
Case = namedtuple("Case", "codes start path failed")


def _case(codes, start, path, failed=0):
    codes = np.ascontiguousarray(M.clipped(codes), dtype=np.uint32)
    assert codes.size <= MAX_N
    return Case(codes, int(start), path, failed)


def twos(n, plants=()):
    """L = 2 everywhere (two interleaved chains, one over the even and one over the odd positions), then the plants"""
    code = np.full(n, 2, dtype=np.int64)
    for i, c in plants:
        code[i] = c
    return code


def dense_ramps(n, seed):
    """copies that overlap everywhere, as on a text of random bases: one begins at a third of the positions, about a dozen
    positions long, and the code is what is left of the copy that reaches furthest (code[i + 1] >= code[i] - 1) -- walks
    from neighbouring positions take several hops to meet"""
    rng = np.random.default_rng(seed)
    reach = np.where(rng.random(n) < 1 / 3, np.arange(n) + 8 + rng.geometric(1 / 5, n), 0)
    return np.maximum(np.maximum.accumulate(reach) - np.arange(n), 0)


N3 = 3 * TILE + 5


def merge_at(x, first_hop):
    """Tile 1 is entered from a factor that starts at start_pos = 5, and its walk lands on the mark at offset x.  Even x:
    step 1 marks the even offsets, the entry is odd, and the code 1 at x - 1 changes chains.  Odd x: a code 1 at the tile
    start makes step 1 mark the odd offsets, the entry is even.  first_hop: the entry is x - 1; else offset 1 or 2.
    Tile 2 is entered at its first position (even x) or at offset 1, where a code 1 changes chains again (odd x)."""
    plants = [(TILE + x - 1, 1)]
    if x % 2:
        plants += [(TILE, 1), (2 * TILE + 1, 1)]
    a = x - 1 if first_hop else (2 if x % 2 else 1)
    plants.append((5, TILE + a - 5))
    return _case(twos(N3, plants), 5, "speculative")


def _builders():
    b = {}
    # the entry is where step 1 began: nothing to fix
    b["entry_is_tile_start_twos"] = lambda: _case(twos(N3), 0, "speculative")
    b["entry_is_tile_start_literals"] = lambda: _case(np.zeros(4 * TILE + 1), 0, "speculative")
    # the entry carries a mark of step 1 (every position does), elsewhere than at the tile start
    b["merge_hop0_offset1"] = lambda: _case(M.planted(N3, [(5, TILE + 1 - 5)]), 5, "speculative")
    b["merge_hop0_offset777"] = lambda: _case(M.planted(N3, [(5, TILE + 777 - 5)]), 5, "speculative")
    for x in (63, 64, 1023, 1024, 4095):
        b[f"merge_first_hop_{x}"] = lambda x=x: merge_at(x, True)
        b[f"merge_far_{x}"] = lambda x=x: merge_at(x, False)
    # the walk over the odd offsets of tile 1 never meets a mark: the code 1 at offset 4095 makes it leave at the
    # speculative exit (the start of tile 2), which is accepted, and every mark of step 1 in tile 1 goes
    b["leaves_at_spec_exit"] = lambda: _case(twos(N3, [(5, TILE + 1 - 5), (2 * TILE - 1, 1)]), 5, "speculative")
    # ... without it the walk leaves one position behind that exit
    b["leaves_beside_spec_exit"] = lambda: _case(twos(N3, [(5, TILE + 1 - 5)]), 5, "failed_over", 1)
    b["twos_from_odd_start"] = lambda: _case(twos(2 * TILE + 3), 1, "failed_over", 1)
    b["twos_from_odd_start_5_tiles"] = lambda: _case(twos(5 * TILE + 2), 4097, "failed_over", 1)
    # two interleaved chains whose exits lie tiles apart: the odd one leaves tile 1 into the middle of tile 3
    b["interleaved_far_exits"] = lambda: _case(twos(6 * TILE, [(5, TILE + 1 - 5), (2 * TILE - 1, TILE + 2001)]), 5,
                                               "failed_over", 1)
    # one long factor over tiles 1 .. 4, which step 1 has marked
    b["jumped_tiles_literals"] = lambda: _case(M.planted(8 * TILE, [(0, 5 * TILE + 3)]), 0, "speculative")
    b["jumped_tiles_ramps"] = lambda: _case(np.maximum(M.realistic(8 * TILE + 9, 21), M.planted(8 * TILE + 9, [(7, 5 * TILE + 3)])),
                                            7, "speculative")
    b["lands_20_tiles_on"] = lambda: _case(M.planted(24 * TILE + 1, [(3, 20 * TILE + 11)]), 3, "speculative")  # (32-bit codes)
    b["whole_text_16"] = lambda: _case(M.planted(2 * TILE + 7, [(0, 2 * TILE + 7)]), 0, "speculative")
    b["whole_text_32"] = lambda: _case(M.planted(17 * TILE + 1, [(0, 17 * TILE + 1)]), 0, "speculative")
    # start positions: inside a tile with tiles in front of it, the last position; n around 1, 64 and the tile
    b["start_mid_tile"] = lambda: _case(M.realistic(6 * TILE + 1, 22), 2 * TILE + 1234, "speculative")
    b["start_mid_tile_twos"] = lambda: _case(twos(6 * TILE + 1), 2 * TILE + 1233, "failed_over", 1)
    b["start_last_position"] = lambda: _case(M.realistic(3 * TILE + 1, 23), 3 * TILE, "speculative")
    b["start_last_position_full_tile"] = lambda: _case(M.realistic(3 * TILE, 23), 3 * TILE - 1, "speculative")
    for n in (1, 2, 3, 63, 64, 65, TILE - 1, TILE, TILE + 1):
        b[f"n_{n}"] = lambda n=n: _case(M.realistic(n, 24), 0, "speculative")
        b[f"n_{n}_from_last"] = lambda n=n: _case(twos(n), n - 1, "speculative")
    # a partial last tile (100 positions) entered at its last position, which step 1 has not marked: it leaves at n,
    # the speculative exit, and the tile keeps that one mark
    b["partial_tile_last_position"] = lambda: _case(twos(2 * TILE + 100, [(0, 2 * TILE + 99)]), 0, "speculative")
    b["partial_tile_last_position_marked"] = lambda: _case(M.planted(2 * TILE + 100, [(0, 2 * TILE + 99)]), 0, "speculative")
    # ramps as the pipeline's codes are (code[i + 1] >= code[i] - 1): the fast path with no failed tile
    for seed in (31, 32, 33):
        for s in (0, 4097):
            b[f"ramps_seed{seed}_s{s}"] = lambda seed=seed, s=s: _case(M.realistic(32 * TILE + 1, seed), s, "speculative")
    for seed in (34, 35):
        for s in (0, 4097):
            b[f"dense_ramps_seed{seed}_s{s}"] = lambda seed=seed, s=s: _case(dense_ramps(32 * TILE + 1, seed), s, "speculative")
    # independent uniform codes: whatever the model says (stated from its one run: these are no ramps)
    b["uniform_0_8"] = lambda: _case(M.uniform(12 * TILE + 3, 0, 8, 41), 1, "speculative")
    b["uniform_0_5000"] = lambda: _case(M.uniform(12 * TILE + 3, 0, 5000, 42), 1, "failed_over", 10)
    b["uniform_0_fffe"] = lambda: _case(M.uniform(32 * TILE + 1, 0, M.NARROW_TOP, 43), 0, "failed_over", 4)
    return b


CASES = _builders()


@functools.lru_cache(maxsize=None)
def case(name):
    return CASES[name]()


def widths_of(name):
    return (32, 16) if int(case(name).codes.max(initial=0)) <= M.NARROW_TOP else (32,)


@functools.lru_cache(maxsize=None)
def expected(name):
    """the definition: what the call must return, whichever path it takes"""
    c = case(name)
    starts = M.cursor(c.codes, c.start)
    return M.outputs(c.codes, starts, False)
