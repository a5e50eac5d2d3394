"""The model of the base-level alignments (tests/rlz_align_model.py) against helpers that share nothing with it, the
rules that ties make observable, and everything nolzss_rlz_index_align decides before any device work.  No GPU."""
import ctypes as C
import random

import numpy as np
import pytest

import rlz_align_model as am
import rlz_seed_chain_model as cm
from nolzss_amd import _lib
from nolzss_amd import _noLZSS as native

I, D, EQ, X = am.I, am.D, am.EQ, am.X
PLANTED_SEED = 7


def edited(rng, s, edits):
    s = bytearray(s)
    for _ in range(edits):
        p = rng.randrange(len(s) + 1)
        kind = rng.choice("sid")
        if kind == "s" and p < len(s):
            s[p] = rng.choice(b"ACGT")
        elif kind == "i":
            s[p:p] = bytes([rng.choice(b"ACGT")])
        elif p < len(s) and len(s) > 1:
            del s[p]
    return bytes(s)


def test_the_banded_cost_is_the_unbanded_distance_when_that_fits_the_band():
    rng, checked = random.Random(1), 0
    for case in range(300):
        alphabet = b"ACGT" if case % 3 else b"AC"
        q = bytes(rng.choice(alphabet) for _ in range(rng.randrange(1, 60)))
        r = edited(rng, q, rng.randrange(0, 7))
        band = rng.randrange(0, 9)
        dist = am.wagner_fischer(q, r)
        if dist > band or abs(len(r) - len(q)) + 2 * band + 1 > am.LANES:
            continue
        cost, codes = am.gap(q, r, band)
        assert cost == dist == sum(c != EQ for c in codes)
        ops = [(n << 4) | c for n, c in am.merged(codes)]
        assert am.replay(ops, q, r, 0, len(q), 0, len(r), False) == (q, dist)
        checked += 1
    assert checked >= 100


def test_a_flank_costs_the_best_prefix_of_the_reference():
    rng = random.Random(2)
    for case in range(120):
        q = bytes(rng.choice(b"ACGT") for _ in range(rng.randrange(1, 30)))
        avail = edited(rng, q, rng.randrange(0, 4)) + bytes(rng.choice(b"ACGT") for _ in range(rng.randrange(0, 40)))
        band = rng.randrange(3, 12)
        got = am.flank(q, avail, band)
        reach = range(max(0, len(q) - band), min(len(avail), len(q) + band) + 1)
        if not len(reach):
            assert got is None
            continue
        cost, j, codes = got
        best = min(am.wagner_fischer(q, avail[:w]) for w in reach)
        if best <= band:  # (the band then holds an optimal path)
            assert cost == best
        assert j in reach and cost == sum(c != EQ for c in codes)
        ops = [(n << 4) | c for n, c in am.merged(codes)]
        assert am.replay(ops, q, avail, 0, len(q), 0, j, False) == (q, cost)
    assert am.flank(b"", b"ACGT", 4) is None and am.flank(b"ACGT" * 3, b"ACGT" * 9, 4, max_flank=11) is None
    assert am.flank(b"ACGT" * 3, b"ACGT" * 9, 4, max_flank=12)[:2] == (0, 12)
    assert am.flank(b"ACGTACGT", b"ACG", 4) is None and am.flank(b"ACGTACGT", b"ACGT", 4)[:2] == (4, 4)
    assert am.flank(b"ACG", b"", 4) == (3, 0, [I, I, I])


def test_low_complexity_pairs_make_the_tie_rule_observable():
    """diagonal first puts the indel of a run at its low end; another order puts it elsewhere at the same cost"""
    assert am.gap(b"AA", b"AAA", 1) == (1, [D, EQ, EQ])
    assert am.gap(b"AA", b"AAA", 1, rule=("left", "up", "diag")) == (1, [EQ, EQ, D])
    assert am.gap(b"AAA", b"AA", 1) == (1, [I, EQ, EQ])
    assert am.gap(b"AAA", b"AA", 1, rule=("up", "diag", "left")) == (1, [EQ, EQ, I])
    assert am.gap(b"ACAC", b"ACACAC", 2) == (2, [D, D, EQ, EQ, EQ, EQ])
    assert am.gap(b"ACAC", b"ACACAC", 2, rule=("left", "diag", "up")) == (2, [EQ, EQ, EQ, EQ, D, D])
    # up before left: AC against CA is two mismatches by the diagonal, an I and a D by the others
    assert am.gap(b"AC", b"CA", 1) == (2, [X, X])
    assert am.gap(b"AC", b"CA", 1, rule=("up", "left", "diag"))[1] != [X, X]
    assert am.gap(b"", b"ACG", 3) == (3, [D, D, D]) and am.gap(b"AC", b"", 3) == (2, [I, I])
    # a left flank is the job on the reversed strings, its ops reversed: the indel of a run goes to its HIGH end
    assert am.job(am.LEFT, b"CAA", b"GAAA", 3, 2, 4, 3, 1) == (0, 2, [EQ, EQ])
    assert am.job(am.RIGHT, b"AAC", b"AAAG", 0, 2, 0, 4, 1) == (0, 2, [EQ, EQ])
    assert am.job(am.GAP, b"TAAT", b"GAAAG", 1, 2, 1, 3, 1) == (1, 3, [D, EQ, EQ])


def test_flank_ties_go_to_the_nearest_end_column_then_to_the_smaller():
    # A against C, CA: D[1][0] = D[1][1] = D[1][2] = 1 -- the nearest is j = fq = 1, the smallest is 0
    assert am.flank(b"A", b"CA", 1) == (1, 1, [X])
    assert am.flank(b"A", b"CA", 1, tie="smallest")[:2] == (1, 0)
    # AC against C, CA, CAC: 1, 2, 1 -- both best columns are one away: the smaller wins
    assert [am.wagner_fischer(b"AC", b"CAC"[:w]) for w in (1, 2, 3)] == [1, 2, 1]
    assert am.flank(b"AC", b"CAC", 1)[:2] == (1, 1)
    # AAAA against AAAAAA: only j = fq = 4 costs nothing
    assert am.flank(b"AAAA", b"AAAAAA", 2) == (0, 4, [EQ] * 4)


def planted_alignments(seed=PLANTED_SEED):
    refs, targets, truth = am.planted(random.Random(seed))
    params = dict(am.DEFAULTS)
    band, max_flank = params.pop("band"), params.pop("max_flank")
    chains = cm.expected(refs, targets, True, **params)
    return refs, targets, truth, chains, am.expected(refs, targets, chains, band, max_flank)


def test_every_model_cigar_replays_and_every_planted_read_is_recovered():
    refs, targets, truth, chains, exp = planted_alignments()
    block = b"\x01".join(refs)
    assert len(exp["target"]) == len(chains["target"]) >= len(targets)
    for key in ("target", "record", "is_rc", "score", "primary"):
        assert np.array_equal(exp[key], chains[key])
    for c in range(len(exp["target"])):
        ops = exp["ops"][int(exp["op_offsets"][c]):int(exp["op_offsets"][c + 1])]
        target = targets[int(exp["target"][c])]
        t0, t1, r0, r1 = (int(exp[k][c]) for k in ("t_start", "t_end", "r_start", "r_end"))
        rebuilt, cost = am.replay(ops, target, block, t0, t1, r0, r1, bool(exp["is_rc"][c]))
        assert rebuilt == target[t0:t1] and cost == int(exp["edit_distance"][c])
        codes = [int(o) & 15 for o in ops]
        assert all(a != b for a, b in zip(codes, codes[1:])) and len(ops) == int(exp["num_ops"][c])
        assert sum(int(o) >> 4 for o in ops) == int(exp["columns"][c])
    for j, (record, is_rc, edits) in enumerate(truth):
        sel = np.flatnonzero((exp["target"] == j) & exp["primary"])
        assert len(sel) == 1, j
        c = sel[0]
        assert (int(exp["record"][c]), bool(exp["is_rc"][c])) == (record, is_rc), j
        assert int(exp["t_start"][c]) == 0 and int(exp["t_end"][c]) == len(targets[j]), j
        assert int(exp["edit_distance"][c]) <= edits, j
    assert any(int(o) & 15 == X for o in exp["ops"]) and any(int(o) & 15 == I for o in exp["ops"])
    assert any(int(o) & 15 == D and int(o) >> 4 == 20 for o in exp["ops"]) or any(int(o) & 15 == I and int(o) >> 4 == 20 for o in exp["ops"])


def test_symbols_layouts_and_exports():
    for name in ("nolzss_rlz_index_align", "nolzss_free_rlz_align_result", "nolzss_debug_rlz_align_jobs"):
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(_lib.lib, name)
    assert native.ALIGN_DTYPE.itemsize == 80 and native.ALIGN_LANES == 64
    assert native.ALIGN_DTYPE.names == ("target", "t_start", "t_end", "r_start", "r_end", "score", "edit_distance", "columns",
                                        "record", "is_rc", "num_ops", "primary")
    assert C.sizeof(_lib.RlzAlignParams) == 56 and C.sizeof(_lib.RlzAlignResult) == 7 * C.sizeof(C.c_void_p)
    import noLZSS.genomics.rlz as shim
    from nolzss_amd.genomics import rlz
    for name in ("ALIGN_DTYPE", "cigar_string"):
        assert name in rlz.__all__ and name in shim.__all__
        assert getattr(shim, name) is getattr(rlz, name)
    assert rlz.ALIGN_DTYPE is native.ALIGN_DTYPE and hasattr(native, "debug_rlz_align_jobs")
    assert rlz.cigar_string(np.array([(12 << 4) | EQ, (1 << 4) | X, (3 << 4) | I, (20 << 4) | D], dtype=np.uint32)) == "12=1X3I20D"
    assert rlz.cigar_string([]) == ""


def test_more_than_64_diagonals_raise_before_the_native_layer_is_touched():
    from nolzss_amd.genomics import rlz
    ix = rlz.RlzIndex.__new__(rlz.RlzIndex)  # no handle: anything that reached for one would raise "closed"
    ix._handle = None
    for bad in (dict(bandwidth=31, band=17), dict(bandwidth=63, band=1), dict(bandwidth=64, band=0), dict(bandwidth=0, band=32)):
        with pytest.raises(ValueError, match="64 diagonals"):
            ix.align([b"ACGT"], **bad)
        with pytest.raises(ValueError, match="64 diagonals"):
            native._align_params(15, 64, 5000, bad["bandwidth"], 40, bad["band"], 256)
    with pytest.raises(ValueError, match="closed"):
        ix.align([b"ACGT"], bandwidth=31, band=16)  # 64 exactly: passes the rule and reaches for the handle
    for name in ("min_length", "max_hits", "max_gap", "bandwidth", "min_score", "band", "max_flank"):
        with pytest.raises(ValueError, match=name):
            ix.align([b"ACGT"], **{name: -1})
        with pytest.raises(ValueError, match=name):
            native._align_params(**dict(dict(am.DEFAULTS), **{name: 1 << 64}))
    p = native._align_params(15, 64, 1 << 33, 31, 40, 16, 1 << 40)
    assert (p.max_gap, p.bandwidth, p.band, p.max_flank) == (1 << 33, 31, 16, 1 << 40)


def test_refusals_before_any_device_work():
    lib, bad = _lib.lib, _lib.ERR_INVALID_ARGUMENT
    pt, ln = (C.c_char_p * 1)(b"ACGT"), (C.c_size_t * 1)(4)
    params, res = _lib.RlzAlignParams(15, 64, 5000, 31, 40, 16, 256), _lib.RlzAlignResult()
    assert lib.nolzss_rlz_index_align(None, pt, ln, 1, C.byref(params), None) == bad
    assert b"output pointer is null" in lib.nolzss_last_error()
    res.num_alignments = 7
    assert lib.nolzss_rlz_index_align(None, pt, ln, 1, C.byref(params), C.byref(res)) == bad
    assert b"handle is null" in lib.nolzss_last_error() and res.num_alignments == 0 and not res.op_offsets
    # the next ones are decided before the handle is read: a block of zero bytes stands in for one
    stand_in = C.create_string_buffer(4096)
    assert lib.nolzss_rlz_index_align(stand_in, pt, ln, 1, None, C.byref(res)) == bad
    assert b"params is null" in lib.nolzss_last_error()
    for bandwidth, band in ((31, 17), (64, 0), (0, 32), (1 << 63, 1 << 63)):
        wide = _lib.RlzAlignParams(15, 64, 5000, bandwidth, 40, band, 256)
        assert lib.nolzss_rlz_index_align(stand_in, pt, ln, 1, C.byref(wide), C.byref(res)) == bad
        assert b"at most 64 diagonals" in lib.nolzss_last_error() and not res.op_offsets
    long_one = (C.c_size_t * 1)(1 << 28)  # the length alone decides: no base is read
    assert lib.nolzss_rlz_index_align(stand_in, pt, long_one, 1, C.byref(params), C.byref(res)) == bad
    assert b"below 2^28 bases" in lib.nolzss_last_error()
    k = (1 << 24) + 1  # empty targets: neither array is read
    ptrs, lens = np.zeros(k, dtype=np.uintp), np.zeros(k, dtype=np.uintp)
    assert lib.nolzss_rlz_index_align(stand_in, ptrs.ctypes.data_as(C.POINTER(C.c_char_p)),
                                      lens.ctypes.data_as(C.POINTER(C.c_size_t)), k, C.byref(params), C.byref(res)) == bad
    assert b"at most 2^24 targets" in lib.nolzss_last_error() and not res.alignments and not res.op_offsets
    lib.nolzss_free_rlz_align_result(None)
    lib.nolzss_free_rlz_align_result(C.byref(res))
    assert res.num_alignments == 0 and res.num_ops == 0


def test_the_debug_hook_refuses_bad_jobs_before_any_launch():
    q, r = b"ACGTACGTAC", b"ACGTTACGTACG"

    def run(jobs, band=2, query=q, reference=r):
        cols = [np.array([j[k] for j in jobs], dtype=np.uint32) for k in range(5)]
        return native.debug_rlz_align_jobs(query, reference, *cols, band)

    for jobs, band, text in (([(3, 0, 1, 0, 1)], 2, "kind"), ([(0, 8, 3, 0, 3)], 2, "leaves a text"),
                             ([(0, 0, 3, 10, 3)], 2, "leaves a text"), ([(1, 11, 0, 0, 0)], 2, "leaves a text"),
                             ([(2, 3, 4, 5, 2)], 2, "leaves a text"), ([(2, 3, 2, 5, 6)], 2, "leaves a text"),
                             ([(0, 0, 1, 0, 1)], 32, "64 diagonals"), ([(0, 0, 2, 0, 12)], 27, "64 diagonals")):
        with pytest.raises(ValueError, match=text):
            run(jobs, band)
    with pytest.raises(ValueError, match="invalid base"):
        run([(0, 0, 1, 0, 1)], query=b"ACNT")
    with pytest.raises(ValueError, match="one entry per job"):
        native.debug_rlz_align_jobs(q, r, [0, 0], [0], [1], [0], [1], 2)
    got = run([])  # no job: no launch, no device
    assert got["col_offsets"].tolist() == [0] and len(got["cols"]) == 0 and len(got["cost"]) == 0
