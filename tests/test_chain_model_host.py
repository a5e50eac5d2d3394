"""The model of the greedy cursor (tests/chain_model.py) without a GPU: the definition and what follows from its marks
against plain Python on tiny arrays, the stage-level restatement against the definition on every input of
tests/test_gpu_chain_direct.py, what every input family is there for, the named mistakes against the inputs that are there
to see them, and the refusals of the debug hook that need no device."""
import random
from pathlib import Path

import numpy as np
import pytest

import chain_model as M
from nolzss_amd import _lib

TILE, T = M.TILE, M.T


# ---- the model against plain Python ------------------------------------------------------------------------------------------
def test_the_outputs_match_a_python_walk_on_tiny_arrays():
    rng = random.Random(20261020)
    long_ones = 0
    for _ in range(300):
        n = rng.choice([1, 2, 3, 5, 8, 13, 40])
        strand = rng.random() < 0.5
        codes = [rng.choice([0, 0, 1, 1, 2, 3, 7, T - 1, T, T + 1, 50000]) | (M.FLAG if strand and rng.random() < 0.4 else 0)
                 for _ in range(n)]
        start = rng.randrange(0, n + 2)
        bounds = sorted(rng.randrange(0, n + 3) for _ in range(2 * rng.randrange(0, 4)))
        marks, hist, tail, lengths, p = [], {}, [], [], start
        while p < n:
            marks.append(p)
            length, flag = max(1, codes[p] % (1 << 31)), (codes[p] >> 31) if strand else 0
            lengths.append(length)
            if length < T:
                hist[flag * T + length] = hist.get(flag * T + length, 0) + 1
            else:
                tail.append(length + (flag << 32))
            p += length
        starts = M.cursor(codes, start)
        got = M.outputs(codes, starts, strand, bounds)
        assert got["z"] == len(marks) and got["starts"].tolist() == marks and got["lengths"].tolist() == lengths
        assert got["hist"].size == (2 * T if strand else T) and got["tail"].tolist() == sorted(tail)
        assert {int(b): int(c) for b, c in enumerate(got["hist"]) if c} == hist
        assert got["counts"].tolist() == [sum(lo <= m < hi for m in marks) for lo, hi in zip(bounds[::2], bounds[1::2])]
        assert np.array_equal(M.staged(codes, start)["starts"], starts)
        long_ones += len(tail)
    assert long_ones >= 80


def test_the_widening_matches_a_python_dictionary():
    rng = random.Random(7)
    for _ in range(200):
        n = rng.choice([1, 2, 7, 30])
        narrow = [rng.randrange(0, 65) for _ in range(n)]
        items = [(rng.randrange(0, n + 3), rng.randrange(0, 1 << 20)) for _ in range(rng.randrange(0, 12))]
        listed = rng.randrange(0, len(items) + 1)
        best = {}
        for i, c in items[:listed]:
            best[i] = max(best.get(i, 0), c)
        exp = [max(narrow[i], best.get(i, 0)) for i in range(n)]
        got = M.widen(narrow, np.array([i | (c << 32) for i, c in items], dtype=np.uint64), listed)
        assert got.tolist() == exp


# ---- the restatement of the stages against the definition, on every input ----------------------------------------------------
@pytest.mark.parametrize("family", M.FAMILY_NAMES)
def test_the_stages_give_the_definition(family):
    assert M.FAMILIES[family]
    for name in M.FAMILIES[family]:
        c = M.case(name)
        assert c.family == family and c.codes.size <= M.MAX_N
        for width in M.widths_of(name):
            exp = M.expected(name, width)
            got = M.staged(M.cursor_codes(name), c.start, 32 if c.widening is not None else width)
            assert np.array_equal(got["starts"], exp["starts"]), (name, width)
            if width == 16 and c.widening is None:
                assert int(c.codes.max(initial=0)) < 0xffff, name
        if c.compare == "all":  # the tail list holds floor(n / T) + 1 entries: no input comes near its assert
            assert np.count_nonzero(M.expected(name)["lengths"] >= T) <= c.codes.size // T, name


def test_every_input_is_named_once_and_sized_as_listed():
    assert sorted(sum(M.FAMILIES.values(), [])) == sorted(M.CASES)
    assert max(M.case(name).codes.size for name in M.CASES) == 32 * TILE + 1
    assert {M.case(name).codes.size for name in M.FAMILIES["sizes"]} == set(M.SIZES)
    for n in M.SIZES:
        assert M.starts_for(n)[-2:] == [n, n + 5] and {0, n - 1} <= set(M.starts_for(n))
        assert M.expected(f"size_{n}_s{n}")["z"] == 0 and M.expected(f"size_{n}_s{n + 5}")["z"] == 0
    assert {1, 2, 4095, 4096, 4097} <= set(M.starts_for(8193)) and 8193 // 3 | 1 in M.starts_for(8193)
    both = [name for name in M.CASES if M.widths_of(name) == (32, 16)]
    assert len(both) >= 170 and all(M.case(name).widening is None for name in both)


# ---- what every family is there for ------------------------------------------------------------------------------------------
def test_literals_make_one_node_per_tile_and_need_every_round():
    rounds_at = {}
    for name in M.FAMILIES["literals"]:
        c = M.case(name)
        n = c.codes.size
        tiles, plus = n // TILE, n % TILE
        assert plus in (0, 1) and tiles in M.TILE_COUNTS
        for width in (32, 16):
            st = M.staged(c.codes, 0, width)
            # the start and the end of every tile but the last: exactly one node per tile
            assert st["K"] == tiles + plus == st["entries"] == (n + TILE - 1) // TILE, name
            assert st["exit_rounds"] == (12 if tiles else 0), name       # all twelve doubling rounds
            assert M.expected(name, width)["z"] == n, name                 # every bitmap word is full
        rounds_at[st["K"]] = st["rounds"]
    # K + 1 on both sides of the powers of two that decide the Wyllie round count
    for r in range(1, 6):
        assert rounds_at[2 ** r - 1] == r and rounds_at[2 ** r] == r + 1
    assert rounds_at[1] == 1 and rounds_at[33] == 6


def test_constant_lengths_and_seams_do_what_they_are_listed_for():
    for start in (0, 1):  # the chain of twos lives on one half-word of every pair
        s = M.expected("const_2_even" if start == 0 else "const_2_odd")["starts"]
        assert (s % 2 == start).all() and s.size > TILE
    offsets = {L: M.expected(f"const_{L}_s1")["starts"] % TILE for L in (4095, 4096, 4097)}
    assert np.array_equal(offsets[4095], (1 - np.arange(10)) % TILE) and (offsets[4096] == 1).all() and offsets[4096].size == 9
    assert np.array_equal(offsets[4097], 1 + np.arange(offsets[4097].size)) and offsets[4097].size == 9
    assert M.staged(M.case("const_4097_s0").codes, 0)["entries"] == 9                  # every tile is entered
    seam = M.expected("seam_4095_c4097")["starts"]
    assert TILE - 1 in seam and 2 * TILE in seam and not ((seam >= TILE) & (seam < 2 * TILE)).any()
    for name, skipped in (("seam_4095_c1", 0), ("seam_4095_c4097", 1), ("seam_4095_c8193", 2), ("seam_0_c4096", 0), ("seam_0_c12288", 2)):
        c = M.case(name)
        st = M.staged(c.codes, 0)
        assert st["entries"] == (c.codes.size + TILE - 1) // TILE - skipped, name     # entry == kNone in between
    for at, stored in ((TILE - 1, 0xfffd), (TILE, 0xfffe - TILE)):
        for tag in ("", "_partial"):
            c = M.case(f"seam_fffe_from{at}{tag}")
            n, target = c.codes.size, at + 0xfffe
            assert target < n and target in M.expected(f"seam_fffe_from{at}{tag}")["starts"]   # no overshoot
            assert target - (at // TILE + 1) * TILE == stored                                  # the exit as the half-word holds it
            assert (n - target // TILE * TILE < TILE) == bool(tag)                             # the target tile is the partial last one
    for name, start in (("seam_whole_16", 3), ("seam_whole_32", 0)):
        assert M.expected(name)["starts"].tolist() == [start] and M.expected(name)["lengths"][0] == M.case(name).codes.size - start
    assert M.widths_of("seam_whole_16") == (32, 16) and M.widths_of("seam_whole_32") == (32,)


def test_realistic_codes_obey_the_ramp_and_adversarial_ones_do_not():
    for name in M.FAMILIES["realistic"] + M.FAMILIES["sizes"]:
        code = M.case(name).codes.astype(np.int64)
        assert (code[1:] >= code[:-1] - 1).all() and (code <= code.size - np.arange(code.size)).all(), name
    assert max(int(M.case(name).codes.max()) for name in M.FAMILIES["realistic"]) > 10000     # the heavy tail
    for name in M.FAMILIES["adversarial"]:
        code = M.case(name).codes.astype(np.int64)
        assert np.count_nonzero(code[1:] < code[:-1] - 1) > code.size // 8, name
        assert (code <= code.size - np.arange(code.size)).all(), name
        if "_4096_8191_" in name:  # nearly every position leaves its tile at once, for an exit of its own
            for width in (32, 16):
                assert M.staged(code, M.case(name).start, width)["K"] > code.size // 4, name
    real = M.staged(M.case("real_86017_seed1_s0").codes, 0)
    assert real["K"] < 86017 // 100   # (what the stage sees on a text: a handful of nodes per tile)


def test_strand_bins_and_overshoot_inputs():
    for name in M.FAMILIES["strand"]:
        c = M.case(name)
        flagged = (c.codes >> 31) == 1
        assert c.with_strand and not (flagged & ((c.codes & M.MASK) == 0)).any()
        assert 0.4 < flagged.sum() / np.count_nonzero(c.codes) < 0.6
        exp = M.expected(name)
        if "real" in name:  # (uniform draws up to 5000 leave a dozen factors, half of them in the tail list)
            assert exp["hist"][:T].sum() > 100 and exp["hist"][T:].sum() > 100
        assert exp["tail"].size >= 2
        assert M.differs(name, 32, "no_mask")
    tails = np.concatenate([M.expected(name)["tail"] for name in M.FAMILIES["strand"]]) >> np.uint64(32)
    assert np.count_nonzero(tails == 0) >= 3 and np.count_nonzero(tails == 1) >= 3   # the strand split of the tail list
    for n in (8 * T, 8 * T + 1):
        a, b, alt = (M.expected(f"bins_{k}_n{n}") for k in ("2047", "2048", "alt"))
        assert a["hist"][T - 1] == 8 and a["tail"].size == 0
        assert b["tail"].tolist() == [T] * 8 and b["hist"].sum() == n - 8 * T
        assert alt["hist"][T - 1] == 4 and alt["tail"].tolist() == [T] * 4 and alt["lengths"][:4].tolist() == [T - 1, T, 1, T - 1]
    for name in M.FAMILIES["overshoot"]:
        c, exp = M.case(name), M.expected(name)
        assert c.compare == "starts" and int(exp["starts"][-1]) + int(exp["lengths"][-1]) > c.codes.size
    assert M.widths_of("overshoot_16") == (32, 16) and M.widths_of("overshoot_32") == (32,)


def test_widening_and_range_inputs():
    for name in M.FAMILIES["widening"]:
        c = M.case(name)
        items, listed, list_max = c.widening
        n, pos, code = c.codes.size, (items & np.uint64(0xffffffff)).astype(np.int64), (items >> np.uint64(32)).astype(np.int64)
        kind = name.split("_", 3)[3]
        assert int(c.codes.max()) == list_max and (c.codes <= list_max).all(), name     # some code is saturated
        wide = M.expected(name, 16)["widened"]
        if kind != "listed_zero":
            assert (wide[c.codes == list_max] >= list_max).all() and (wide > list_max).any(), name
        if kind.startswith("two_"):
            pp, cc = pos.reshape(-1, 2), code.reshape(-1, 2)   # every saturated position is listed twice
            assert (pp[:, 0] == pp[:, 1]).all() and (cc[:, 0] != cc[:, 1]).any(), name
            assert (cc[:, 0] <= cc[:, 1]).all() if kind == "two_small_first" else (cc[:, 0] >= cc[:, 1]).all(), name
        if kind == "beyond_n":
            assert set(pos[pos >= n].tolist()) == {n, n + 7, 0xffffffff}
        if kind == "listed_short":
            assert 0 < listed < items.size and not np.array_equal(M.widen(c.codes, items, items.size), wide)
        if kind == "listed_zero":
            assert listed == 0 and items.size > 0 and np.array_equal(wide, c.codes)
        assert (c.compare == "all") == (n == 4097 and list_max == 64), name
    assert {M.case(name).codes.size for name in M.FAMILIES["widening"]} == {1, 2, 7, 4097}
    n, starts = M.case("ranges_mixed").codes.size, set(M.expected("ranges_mixed")["starts"].tolist())
    b = M.case("ranges_mixed").bounds.reshape(-1, 2).tolist()
    assert M.expected("ranges_mixed")["counts"].tolist()[:4] == [0, 1, 0, 0] and b[1][0] in starts and b[2][0] not in starts
    assert b[3][1] == b[4][0] and b[4][0] in starts and b[4][1] == n              # touching at a factor start
    t = M.case("ranges_touching").bounds.tolist()
    assert t[1] == t[2] and t[1] in starts and M.expected("ranges_touching")["counts"].sum() == len(starts)
    assert M.expected("ranges_whole")["counts"].tolist() == [len(starts)] and M.expected("ranges_k0")["counts"].size == 0
    for name in M.FAMILIES["ranges"]:
        assert (np.diff(M.case(name).bounds.astype(np.int64)) >= 0).all()


# ---- the named mistakes ------------------------------------------------------------------------------------------------------
# mistake -> (input of tests/test_gpu_chain_direct.py, code width) whose expected output it changes
SEEN_BY = {
    "no_mask": ("strand_real_20481", 32),
    "odd_second_dropped": ("ones_t1_p1", 16),
    "last_target_dropped": ("lit_t3_p0", 32),
    "start_no_node": ("size_4097_s1", 16),
    "wyllie_round_short": ("lit_t3_p0", 16),
    "eleven_rounds": ("lit_t1_p0", 32),
    "widen_last_wins": ("widen_4097_m64_two_large_first", 16),
    "dense_T": ("bins_2048_n16384", 32),
    "mark_full_tile_end": ("lit_t1_p1", 16),
    # The 16-bit exit counted from base + 4096 instead of from n in a partial last tile cannot show in any output: every
    # position of the last tile exits to n (next_pos clamps), so the half-word holds n - (base + 4096) mod 2^16, and
    # node_edges_kernel adds n to it -- a value in [n, n + 0xffff], which is "beyond the text" like n itself.  The same
    # bound taken in chain_mark_kernel is the mistake that shows (mark_full_tile_end: position n gets a mark).
    "narrow_exit_full_tile": None,
}


def test_every_named_mistake_changes_a_named_case():
    assert set(SEEN_BY) == set(M.BUGS)
    for bug, seen in SEEN_BY.items():
        if seen is None:
            continue
        name, width = seen
        assert name in M.CASES and width in M.widths_of(name), bug
        assert M.differs(name, width, bug), bug
        assert not M.differs(name, width, None), bug


def test_the_wyllie_rounds_and_the_doubling_rounds_are_needed_where_they_are_listed():
    """a round less shows wherever K exceeds the power of two below K + 1, and nowhere else"""
    for name in M.FAMILIES["literals"]:
        K = M.staged(M.case(name).codes, 0)["K"]
        assert M.differs(name, 32, "wyllie_round_short") == (K & (K - 1) != 0), name
        assert M.differs(name, 32, "eleven_rounds"), name


def test_the_narrow_exit_mistake_is_silent_on_every_input():
    partial = 0
    for name in M.CASES:  # (the inputs with a partial last tile, up to five tiles)
        n = M.case(name).codes.size
        if 16 in M.widths_of(name) and M.case(name).widening is None and n % TILE and n <= 5 * TILE + 1:
            assert not M.differs(name, 16, "narrow_exit_full_tile"), name
            partial += 1
    assert partial >= 100


# ---- what needs no device ----------------------------------------------------------------------------------------------------
def test_symbol_is_exported_and_declared():
    header = (Path(__file__).resolve().parents[1] / "include" / "nolzss_hip.h").read_text()
    assert "nolzss_debug_chain" in _lib.EXPORTED_SYMBOLS and hasattr(_lib.lib, "nolzss_debug_chain")
    assert "int nolzss_debug_chain(" in header


def test_the_hook_refuses_bad_arguments_before_any_device_work():
    lib, bad = _lib.lib, _lib.ERR_INVALID_ARGUMENT
    codes = np.array([3, 0, 0, 2, 0, 1, 0], dtype=np.uint32)
    z, tc = np.zeros(1, dtype=np.uint32), np.zeros(1, dtype=np.uint32)
    starts, lengths = np.zeros(7, dtype=np.uint32), np.zeros(7, dtype=np.uint32)
    hist, tail = np.zeros(2 * T, dtype=np.uint32), np.zeros(1, dtype=np.uint64)
    items = np.array([3 | (70000 << 32)], dtype=np.uint64)
    bounds, counts = np.array([0, 3, 3, 7], dtype=np.uint32), np.zeros(2, dtype=np.uint32)

    def call(codes_=codes, n=7, start=0, width=32, poison=0, list_=None, list_len=0, listed=0, list_max=0, bounds_=None, k=0,
             z_=z, hist_=hist, tail_=tail, tc_=tc, widened=None, counts_=None):
        p = lambda a: a.ctypes.data if a is not None else None  # noqa: E731
        return lib.nolzss_debug_chain(p(codes_), n, start, width, poison, p(list_), list_len, listed, list_max, 0, p(bounds_), k,
                                      0, p(z_), starts.ctypes.data, lengths.ctypes.data, p(hist_), p(tail_), p(tc_), p(widened),
                                      p(counts_))

    assert call(n=0) == 0 and z[0] == 0                                       # no codes: returns at once
    assert call(codes_=None) == bad and b"null" in lib.nolzss_last_error()
    assert call(z_=None) == bad
    for width in (0, 8, 17, 64, -16):
        assert call(width=width) == bad and b"16 or of 32" in lib.nolzss_last_error()
    for big in (0xffff, 0x10000, 0x80000001):
        wide = codes.copy()
        wide[6] = big
        assert call(codes_=wide, width=16) == bad and b"0xffff" in lib.nolzss_last_error()
    assert call(width=16, poison=0x10000) == bad
    assert call(tail_=None) == bad and call(tc_=None) == bad
    assert call(bounds_=bounds, k=2) == bad and call(counts_=counts, k=2) == bad          # one of the two arrays is missing
    assert call(bounds_=np.array([0, 3, 2, 7], dtype=np.uint32), k=2, counts_=counts) == bad and b"ascend" in lib.nolzss_last_error()
    assert call(width=32, list_=items, list_len=1, listed=1, list_max=64) == bad          # a list with 32-bit codes
    assert call(width=16, list_=items, list_len=1, listed=2, list_max=64) == bad          # listed beyond the list
    assert call(width=16, list_=None, list_len=1, listed=1, list_max=64) == bad
    assert call(width=16, list_=items, list_len=1, listed=1, list_max=0x10000) == bad
    assert call(width=16, list_=items, list_len=1, listed=1, list_max=2) == bad           # a code above list_max
    assert call(width=16, list_=items, list_len=1, listed=1) == bad                       # a list without list_max
    assert call(width=16, widened=starts) == bad
