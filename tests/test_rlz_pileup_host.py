"""The model of the pileup (tests/rlz_pileup_model.py) against counts written out by hand and against helpers that share
nothing with it, and everything nolzss_rlz_pileup_* and its debug hook decide before any device work.  No GPU."""
import ctypes as C
import functools
import random

import numpy as np
import pytest

import rlz_align_model as am
import rlz_pileup_model as pm
import rlz_seed_chain_model as cm
from nolzss_amd import _lib
from nolzss_amd import _noLZSS as native

I, D, EQ, X = pm.I, pm.D, pm.EQ, pm.X
PLANTED_SEED = 7  # the set tests/test_rlz_align_host.py checks the alignments of

#        0123456789 0123
BLOCK = b"ACGTTGCAAGGCTA"
FWD = b"GTTACAG"          # block[2:10] = GTTGCAAG with G>A at 5, CA deleted at 6..7 and a C inserted in front of 8
OPS = [(3, EQ), (1, X), (2, D), (1, I), (2, EQ)]


def op_words(ops):
    return [(n << 4) | code for n, code in ops]


def aln(target, t_start, t_end, r_start, r_end, is_rc, primary=1):
    return dict(target=target, t_start=t_start, t_end=t_end, r_start=r_start, r_end=r_end, is_rc=is_rc, primary=primary)


def run(alignments, ops_per_alignment, targets, block=BLOCK, primary_only=False):
    ops, offsets = [], [0]
    for mine in ops_per_alignment:
        ops += op_words(mine)
        offsets.append(len(ops))
    return pm.pileup(len(block), alignments, ops, offsets, targets, block, primary_only)


def table(rows, B=len(BLOCK)):
    out = np.zeros((B, 8), dtype=np.uint32)
    for p, channel, n in rows:
        out[p, pm.CHANNELS.index(channel)] = n
    return out


def test_one_forward_alignment_against_counts_written_by_hand():
    got = run([aln(0, 0, 7, 2, 10, 0)], [OPS], [FWD])
    assert np.array_equal(got, table([(2, "G", 1), (3, "T", 1), (4, "T", 1), (5, "A", 1), (6, "DEL", 1), (7, "DEL", 1),
                                      (7, "INS", 1), (8, "A", 1), (9, "G", 1)]))


def test_both_strands_of_one_stretch_count_alike_and_rev_counts_the_reverse_one():
    rev = am.revcomp(FWD)
    fwd = run([aln(0, 0, 7, 2, 10, 0)], [OPS], [FWD])
    back = run([aln(0, 0, 7, 2, 10, 1)], [OPS[::-1]], [rev])  # the ops ascend in the read: back to front in the block
    for channel in ("A", "C", "G", "T", "DEL", "INS", "BREAK"):
        k = pm.CHANNELS.index(channel)
        assert np.array_equal(fwd[:, k], back[:, k]), channel
    assert not fwd[:, pm.REV].any() and back[:, pm.REV].tolist() == [0, 0] + [1] * 8 + [0] * 4
    both = run([aln(0, 0, 7, 2, 10, 0), aln(1, 0, 7, 2, 10, 1)], [OPS, OPS[::-1]], [FWD, rev])
    assert np.array_equal(both, fwd + back)
    assert np.array_equal(both[:, :5].sum(axis=1), np.array([0, 0] + [2] * 8 + [0] * 4))  # depth


def test_an_insertion_as_first_and_as_last_op_clamps_into_the_alignment():
    # forward: in front of the first block base there is no base of the alignment -> r_start; behind the last -> r_end - 1
    got = run([aln(0, 0, 6, 4, 8, 0)], [[(1, I), (4, EQ), (1, I)]], [b"CTGCAC"])
    assert got[:, pm.INS].tolist() == [0] * 4 + [1, 0, 0, 1] + [0] * 6
    # reverse: the read's first op is the walk's last
    got = run([aln(0, 0, 7, 4, 8, 1)], [[(2, I), (4, EQ), (1, I)]], [b"CCTGCAG"])
    assert got[:, pm.INS].tolist() == [0] * 4 + [1, 0, 0, 1] + [0] * 6
    # an insertion of any length counts once, anchored at the base in front of it
    got = run([aln(0, 0, 7, 4, 8, 0)], [[(2, EQ), (3, I), (2, EQ)]], [b"TGAAACA"])
    assert got[:, pm.INS].tolist() == [0] * 5 + [1] + [0] * 8


def test_break_marks_the_clipped_end_in_block_orientation():
    read = b"TTTT" + BLOCK[4:9] + b"GG"  # four bases clipped in front, two behind
    fwd = run([aln(0, 4, 9, 4, 9, 0)], [[(5, EQ)]], [read])
    assert fwd[:, pm.BREAK].tolist() == [0] * 4 + [1, 0, 0, 0, 1] + [0] * 5
    front_only = run([aln(0, 4, 11, 4, 9, 0)], [[(5, EQ), (2, I)]], [read])
    assert front_only[:, pm.BREAK].tolist() == [0] * 4 + [1] + [0] * 9
    rc = am.revcomp(BLOCK[4:9]) + b"GG"  # on the reverse strand a clip behind the read's aligned part lies at r_start
    back = run([aln(0, 0, 5, 4, 9, 1)], [[(5, EQ)]], [rc])
    assert back[:, pm.BREAK].tolist() == [0] * 4 + [1] + [0] * 9
    rc = b"GG" + am.revcomp(BLOCK[4:9])
    back = run([aln(0, 2, 7, 4, 9, 1)], [[(5, EQ)]], [rc])
    assert back[:, pm.BREAK].tolist() == [0] * 8 + [1] + [0] * 5


def test_primary_only_skips_the_others_and_a_separator_stays_zero():
    block = b"ACGT\x01TGCA"
    alns = [aln(0, 0, 4, 0, 4, 0, primary=1), aln(0, 0, 4, 5, 9, 1, primary=0)]
    ops = [[(4, EQ)], [(4, EQ)]]
    every = run(alns, ops, [b"ACGT"], block)
    assert every[:, :4].sum() == 8 and not every[4].any() and every[:, pm.REV].sum() == 4
    assert np.array_equal(run(alns, ops, [b"ACGT"], block, primary_only=True)[5:], np.zeros((4, 8), dtype=np.uint32))


def test_variants_of_a_hand_made_table():
    block = b"AC\x01GT"
    counts = np.zeros((5, 8), dtype=np.uint32)
    counts[0, :5] = (6, 3, 0, 0, 1)      # A ref: C 3 of 10, DEL 1 of 10
    counts[0, pm.INS] = 5
    counts[3, :5] = (0, 0, 1, 0, 0)      # G ref, nothing else
    counts[4, :5] = (0, 0, 2, 2, 0)      # T ref: G 2 of 4
    counts[4, pm.REV] = 3
    assert pm.variants(counts, block, [0, 3], 1, 0, 1) == [(0, 0, 0, 0, 1, 3, 10, 0), (0, 0, 0, 0, 4, 1, 10, 0),
                                                           (0, 0, 0, 0, 5, 5, 10, 0), (4, 1, 1, 3, 2, 2, 4, 3)]
    assert pm.variants(counts, block, [0, 3], 2, 1, 2) == [(0, 0, 0, 0, 5, 5, 10, 0), (4, 1, 1, 3, 2, 2, 4, 3)]
    assert pm.variants(counts, block, [0, 3], 3, 3, 10) == [(0, 0, 0, 0, 1, 3, 10, 0), (0, 0, 0, 0, 5, 5, 10, 0)]
    assert pm.variants(counts, block, [0, 3], 3, 9, 10) == []


@functools.lru_cache(maxsize=None)
def planted_alignments():
    refs, targets, truth = am.planted(random.Random(PLANTED_SEED))
    params = dict(am.DEFAULTS)
    band, max_flank = params.pop("band"), params.pop("max_flank")
    chains = cm.expected(refs, targets, True, **params)
    return refs, targets, am.expected(refs, targets, chains, band, max_flank)


def test_every_planted_alignment_adds_one_depth_per_block_column():
    refs, targets, exp = planted_alignments()
    block = b"\x01".join(refs)
    B, recs = len(block), pm.records(exp)
    assert len(recs) >= len(targets)
    total = np.zeros((B, 8), dtype=np.uint64)
    for c, a in enumerate(recs):
        ops = exp["ops"][int(exp["op_offsets"][c]):int(exp["op_offsets"][c + 1])]
        alone = pm.pileup(B, [a], ops, [0, len(ops)], targets, block, False)
        n, code = ops >> 4, ops & 15
        columns = int(n[(code == EQ) | (code == X) | (code == D)].sum())
        assert int(alone[:, :5].sum()) == columns
        # replay consumes block[r_start:r_end] exactly, with an ordinary reverse complement: the same number again
        rebuilt, cost = am.replay(ops, targets[a["target"]], block, a["t_start"], a["t_end"], a["r_start"], a["r_end"],
                                  bool(a["is_rc"]))
        assert columns == a["r_end"] - a["r_start"] == len(rebuilt) - int(n[code == I].sum()) + int(n[code == D].sum())
        assert not alone[:a["r_start"]].any() and not alone[a["r_end"]:].any()
        assert int(alone[:, pm.REV].sum()) == (columns if a["is_rc"] else 0) and int(alone[:, pm.INS].sum()) == int((code == I).sum())
        total += alone
    whole = pm.pileup(B, recs, exp["ops"], exp["op_offsets"], targets, block, False)
    assert np.array_equal(whole, total)
    assert not whole[[len(refs[0]), len(refs[0]) + 1 + len(refs[1])]].any()  # the separators
    primary = pm.pileup(B, recs, exp["ops"], exp["op_offsets"], targets, block, True)
    others = sum(int(total_of.sum()) for total_of in
                 (pm.pileup(B, [a], exp["ops"][int(exp["op_offsets"][c]):int(exp["op_offsets"][c + 1])], [0, int(exp["num_ops"][c])],
                            targets, block, False) for c, a in enumerate(recs) if not a["primary"]))
    assert (primary <= whole).all() and int(whole.sum()) - int(primary.sum()) == others


SAMPLE_SEED = 3  # tests/test_gpu_rlz_pileup.py runs the same sample on the device


def test_the_planted_substitutions_are_the_base_alleles_the_model_reports():
    """the condition of the end-to-end test for the all-CPU path: seed-chain model, align model, pileup model, variants"""
    ref, reads, substitutions = pm.planted_sample(random.Random(SAMPLE_SEED))
    assert len(ref) == 4000 and len(substitutions) == 5 and len(reads) >= 970 and all(len(r) == 100 for r in reads)
    params = dict(am.DEFAULTS)
    band, max_flank = params.pop("band"), params.pop("max_flank")
    exp = am.expected([ref], reads, cm.expected([ref], reads, True, **params), band, max_flank)
    counts = pm.pileup(len(ref), pm.records(exp), exp["ops"], exp["op_offsets"], reads, ref, True)
    found = pm.variants(counts, ref, [0], 3, 1, 2)
    assert sorted((v[0], v[4]) for v in found if v[4] < 4) == substitutions
    # (where the deletion and the insertion fall inside a run of equal bases is the aligner's: not asserted here)
    assert counts[:, pm.REV].sum() > 0 and (counts[300:3700, :5].sum(axis=1) >= 20).all()


def test_symbols_layouts_and_exports():
    header = open(_lib.__file__.replace("nolzss_amd/_lib.py", "include/nolzss_hip.h")).read()
    for name in ("nolzss_rlz_pileup_open", "nolzss_rlz_pileup_add", "nolzss_rlz_pileup_counts", "nolzss_rlz_pileup_variants",
                 "nolzss_free_rlz_variants_result", "nolzss_rlz_pileup_info", "nolzss_rlz_pileup_close", "nolzss_debug_rlz_pileup"):
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(_lib.lib, name) and f"{name}(" in header
    assert native.VARIANT_DTYPE.itemsize == C.sizeof(_lib.RlzVariant) == 40
    assert native.VARIANT_DTYPE.names == tuple(name for name, _ in _lib.RlzVariant._fields_) == pm.VARIANT_FIELDS
    assert C.sizeof(_lib.RlzPileupAddInfo) == 32 and C.sizeof(_lib.RlzPileupSummary) == 64 + C.sizeof(_lib.RlzAlignParams)
    assert native.PILEUP_CHANNELS == ("A", "C", "G", "T", "DEL", "INS", "REV", "BREAK") == pm.CHANNELS
    import noLZSS.genomics.rlz as shim
    from nolzss_amd.genomics import rlz
    for name in ("VARIANT_DTYPE", "PILEUP_CHANNELS", "RlzPileup"):
        assert name in rlz.__all__ and name in shim.__all__
        assert getattr(shim, name) is getattr(rlz, name)
    assert rlz.VARIANT_DTYPE is native.VARIANT_DTYPE and hasattr(rlz.RlzIndex, "pileup") and hasattr(native, "debug_rlz_pileup")
    for method in ("add", "counts", "variants", "info", "close"):
        assert hasattr(rlz.RlzPileup, method)


def test_bad_parameters_raise_before_the_native_layer_is_touched():
    from nolzss_amd.genomics import rlz
    ix = rlz.RlzIndex.__new__(rlz.RlzIndex)  # no handle: anything that reached for one would raise "closed"
    ix._handle = None
    for bad in (dict(bandwidth=31, band=17), dict(bandwidth=64, band=0), dict(bandwidth=0, band=32)):
        with pytest.raises(ValueError, match="64 diagonals"):
            ix.pileup(**bad)
    with pytest.raises(ValueError, match="min_score"):
        ix.pileup(min_score=-1)
    with pytest.raises(ValueError, match="the index is closed"):
        ix.pileup()  # the defaults pass the rule and reach for the handle
    pile = rlz.RlzPileup(None, ix, True)  # closed
    for count, fraction in ((0, (1, 2)), (2, (3, 2)), (2, (1, 0)), (2, (-1, 2)), (2, 0.5), (1 << 32, (1, 2))):
        with pytest.raises(ValueError, match="min_count|min_fraction"):
            pile.variants(count, fraction)
    for call in (lambda: pile.variants(), lambda: pile.counts(), lambda: pile.add([b"ACGT"]), lambda: pile.info):
        with pytest.raises(ValueError, match="the pileup is closed"):
            call()
    pile.close()


def test_refusals_before_any_device_work():
    lib, bad = _lib.lib, _lib.ERR_INVALID_ARGUMENT
    pt, ln = (C.c_char_p * 1)(b"ACGT"), (C.c_size_t * 1)(4)
    params, out = _lib.RlzAlignParams(15, 64, 5000, 31, 40, 16, 256), C.c_void_p(5)
    stand_in = C.create_string_buffer(4096)  # zero bytes stand in for a handle where it is not read, or read as empty
    assert lib.nolzss_rlz_pileup_open(stand_in, C.byref(params), None) == bad
    assert b"output pointer is null" in lib.nolzss_last_error()
    assert lib.nolzss_rlz_pileup_open(None, C.byref(params), C.byref(out)) == bad
    assert b"handle is null" in lib.nolzss_last_error() and not out.value
    assert lib.nolzss_rlz_pileup_open(stand_in, None, C.byref(out)) == bad
    assert b"params is null" in lib.nolzss_last_error()
    for bandwidth, band in ((31, 17), (64, 0), (0, 32), (1 << 63, 1 << 63)):
        wide = _lib.RlzAlignParams(15, 64, 5000, bandwidth, 40, band, 256)
        assert lib.nolzss_rlz_pileup_open(stand_in, C.byref(wide), C.byref(out)) == bad
        assert b"at most 64 diagonals" in lib.nolzss_last_error() and not out.value
    info = _lib.RlzPileupAddInfo(1, 2, 3, 4)
    assert lib.nolzss_rlz_pileup_add(stand_in, pt, ln, 1, 1, None) == bad
    assert b"output pointer is null" in lib.nolzss_last_error()
    assert lib.nolzss_rlz_pileup_add(None, pt, ln, 1, 1, C.byref(info)) == bad
    assert b"handle is null" in lib.nolzss_last_error() and (info.alignments, info.targets) == (0, 0)
    long_one = (C.c_size_t * 1)(1 << 28)  # the length alone decides: neither the handle nor a base is read
    assert lib.nolzss_rlz_pileup_add(stand_in, pt, long_one, 1, 1, C.byref(info)) == bad
    assert b"below 2^28 bases" in lib.nolzss_last_error()
    k = (1 << 24) + 1  # empty targets: neither array is read
    ptrs, lens = np.zeros(k, dtype=np.uintp), np.zeros(k, dtype=np.uintp)
    assert lib.nolzss_rlz_pileup_add(stand_in, ptrs.ctypes.data_as(C.POINTER(C.c_char_p)),
                                     lens.ctypes.data_as(C.POINTER(C.c_size_t)), k, 1, C.byref(info)) == bad
    assert b"at most 2^24 targets" in lib.nolzss_last_error()
    words = np.zeros(8, dtype=np.uint32)
    assert lib.nolzss_rlz_pileup_counts(None, 0, 0, words.ctypes.data) == bad
    assert lib.nolzss_rlz_pileup_counts(stand_in, 0, 1, words.ctypes.data) == bad  # end > B: the stand-in's block is empty
    assert b"0 <= start <= end <= block length" in lib.nolzss_last_error()
    assert lib.nolzss_rlz_pileup_counts(stand_in, 1, 0, words.ctypes.data) == bad
    assert lib.nolzss_rlz_pileup_counts(stand_in, 0, 0, None) == _lib.OK  # nothing asked for
    res = _lib.RlzVariantsResult(7, None)
    assert lib.nolzss_rlz_pileup_variants(stand_in, 2, 1, 2, None) == bad
    assert lib.nolzss_rlz_pileup_variants(None, 2, 1, 2, C.byref(res)) == bad
    assert b"handle is null" in lib.nolzss_last_error() and res.num_variants == 0
    for min_count, num, den in ((2, 1, 0), (2, 3, 2), (0, 1, 2), (2, 1, 1 << 32)):
        assert lib.nolzss_rlz_pileup_variants(stand_in, min_count, num, den, C.byref(res)) == bad, (min_count, num, den)
        assert b"rlz pileup: " in lib.nolzss_last_error() and not res.variants
    assert lib.nolzss_rlz_pileup_info(None, None) == bad
    assert lib.nolzss_rlz_pileup_close(None) == _lib.OK
    lib.nolzss_free_rlz_variants_result(None)
    lib.nolzss_free_rlz_variants_result(C.byref(res))
    assert res.num_variants == 0 and not res.variants


def test_the_debug_hook_refuses_bad_alignments_before_any_launch():
    def hook(alignments, ops_per_alignment, targets=(FWD,), block=BLOCK, offsets=None):
        recs = np.zeros(len(alignments), dtype=native.ALIGN_DTYPE)
        ops, off = [], [0]
        for c, (a, mine) in enumerate(zip(alignments, ops_per_alignment)):
            for key, v in a.items():
                recs[key][c] = v
            ops += op_words(mine)
            off.append(len(ops))
        return native.debug_rlz_pileup(block, list(targets), recs, off if offsets is None else offsets, ops)

    good = aln(0, 0, 7, 2, 10, 0)
    for a, mine, text in ((dict(good, target=1), OPS, "beyond the batch"), (dict(good, t_end=8), OPS, "leaves its target"),
                          (dict(good, r_start=7, r_end=15), OPS, "leaves the block"), (dict(good, r_end=11), OPS, "consume exactly"),
                          (dict(good, t_start=1), OPS, "consume exactly"), (good, OPS[:-1] + [(2, 3)], "unknown code"),
                          (good, OPS[:-1] + [(0, EQ), (2, EQ)], "length 0"), (good, [], "no ops")):
        with pytest.raises(ValueError, match=text):
            hook([a], [mine])
    with pytest.raises(ValueError, match="covers a separator"):
        hook([aln(0, 0, 6, 2, 8, 0)], [[(6, EQ)]], block=b"ACGT\x01TGCA")
    with pytest.raises(ValueError, match="invalid base"):
        hook([good], [OPS], targets=(b"GTTNCAG",))
    with pytest.raises(ValueError, match="from 0 to num_ops"):
        hook([good], [OPS], offsets=[1, 5])
    with pytest.raises(ValueError, match="one entry per alignment"):
        hook([good], [OPS], offsets=[0, 2, 5])
    got = hook([], [])  # no alignment: no launch, no device
    assert got.shape == (len(BLOCK), 8) and got.dtype == np.uint32 and not got.any()
