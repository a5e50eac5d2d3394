"""The model of the normalised walk, the insertion alleles and the consensus (tests/rlz_consensus_model.py) against
counts and texts written out by hand and against the un-normalised model, the condition of the end-to-end test on the
all-CPU path, and everything the new entry points decide before any device work.  No GPU."""
import ctypes as C
import functools
import random

import numpy as np
import pytest

import rlz_align_model as am
import rlz_consensus_model as km
import rlz_pileup_model as pm
import rlz_seed_chain_model as cm
from nolzss_amd import _lib
from nolzss_amd import _noLZSS as native
from nolzss_amd._noLZSS import CONSENSUS_STATS, INSERTION_DTYPE, PILEUP_INS_BASES, insertion_bases  # (the feature: none without it)

assert CONSENSUS_STATS == km.STATS and PILEUP_INS_BASES == km.INS_BASES and km.MAX_SHIFT == 1024  # the model's constants are the ABI's
I, D, EQ, X = pm.I, pm.D, pm.EQ, pm.X
SAMPLE_SEEDS = (3, 11)  # tests/test_gpu_rlz_consensus.py runs the same samples on the device
PLANTED_SEED = 7


def op_words(ops):
    return [(n << 4) | code for n, code in ops]


def aln(target, t_start, t_end, r_start, r_end, is_rc, primary=1):
    return dict(target=target, t_start=t_start, t_end=t_end, r_start=r_start, r_end=r_end, is_rc=is_rc, primary=primary)


def run(block, alignments, ops_per_alignment, targets, normalize=True, primary_only=False):
    ops, offsets = [], [0]
    for mine in ops_per_alignment:
        ops += op_words(mine)
        offsets.append(len(ops))
    return km.walk(block, alignments, ops, offsets, targets, primary_only, normalize)


def channel(counts, name):
    return counts[:, pm.CHANNELS.index(name)].tolist()


@functools.lru_cache(maxsize=None)
def sample_alignments(seed):
    ref, reads, substitutions, sample = km.planted_sample_with_truth(random.Random(seed))
    params = dict(am.DEFAULTS)
    band, max_flank = params.pop("band"), params.pop("max_flank")
    exp = am.expected([ref], reads, cm.expected([ref], reads, True, **params), band, max_flank)
    return ref, reads, sample, exp


def test_the_truth_generator_makes_the_draws_of_the_planted_sample():
    for seed in SAMPLE_SEEDS:
        ref, reads, substitutions, sample = km.planted_sample_with_truth(random.Random(seed))
        assert (ref, reads, substitutions) == pm.planted_sample(random.Random(seed))
        assert len(sample) == len(ref) - 3 + 2 and reads[0] == sample[:100]


def test_without_the_flag_the_walk_is_the_pileup_model():
    refs, targets, truth = am.planted(random.Random(PLANTED_SEED))
    params = dict(am.DEFAULTS)
    band, max_flank = params.pop("band"), params.pop("max_flank")
    exp = am.expected(refs, targets, cm.expected(refs, targets, True, **params), band, max_flank)
    block = b"\x01".join(refs)
    recs = pm.records(exp)
    for primary_only in (False, True):
        counts, events = km.walk(block, recs, exp["ops"], exp["op_offsets"], targets, primary_only, False)
        assert np.array_equal(counts, pm.pileup(len(block), recs, exp["ops"], exp["op_offsets"], targets, block, primary_only))
        assert len(events) == int(counts[:, pm.INS].sum())
        normal, moved = km.walk(block, recs, exp["ops"], exp["op_offsets"], targets, primary_only, True)
        # the depth invariant: a shift moves columns between channels and positions of one alignment, never the depth
        assert np.array_equal(normal[:, :5].sum(axis=1), counts[:, :5].sum(axis=1))
        for name in ("REV", "BREAK"):
            assert channel(normal, name) == channel(counts, name)
        assert len(moved) == len(events) and int(normal[:, pm.INS].sum()) == len(events)


def test_a_deletion_inside_a_homopolymer_moves_to_its_left_end_on_both_strands():
    #         0123456789
    block = b"CGAAAATCGT"  # the sample lost one A of the run 2 .. 5
    fwd = b"CGAAATCG"      # the aligner deletes the LAST A on the forward strand ...
    got, events = run(block, [aln(0, 0, 8, 0, 9, 0)], [[(5, EQ), (1, D), (3, EQ)]], [fwd])
    assert channel(got, "DEL") == [0, 0, 1, 0, 0, 0, 0, 0, 0, 0] and channel(got, "A") == [0, 0, 0, 1, 1, 1, 0, 0, 0, 0]
    assert not events
    # ... and, read on the reverse strand, the FIRST one in block coordinates: ops ascend in the read, back to front here
    rev = am.revcomp(fwd)
    back, _ = run(block, [aln(0, 0, 8, 0, 9, 1)], [[(6, EQ), (1, D), (2, EQ)]], [rev])
    assert np.array_equal(back[:, :6], got[:, :6]) and channel(back, "REV") == [1] * 9 + [0]
    # without the flag the two strands disagree
    plain_f, _ = run(block, [aln(0, 0, 8, 0, 9, 0)], [[(5, EQ), (1, D), (3, EQ)]], [fwd], normalize=False)
    plain_r, _ = run(block, [aln(0, 0, 8, 0, 9, 1)], [[(6, EQ), (1, D), (2, EQ)]], [rev], normalize=False)
    assert channel(plain_f, "DEL").index(1) == 5 and channel(plain_r, "DEL").index(1) == 2
    # the whole preceding `=` run is given up: it counts no position
    got, _ = run(b"AAAAC", [aln(0, 0, 3, 0, 5, 0)], [[(2, EQ), (2, D), (1, EQ)]], [b"AAC"])
    assert channel(got, "DEL") == [1, 1, 0, 0, 0] and channel(got, "A") == [0, 0, 1, 1, 0] and channel(got, "C") == [0, 0, 0, 0, 1]


def test_an_insertion_inside_a_tandem_repeat_rotates_as_it_moves():
    #         0123456789
    block = b"GACACACTTG"  # the sample has one more AC
    read = b"GACACACACTTG"
    got, events = run(block, [aln(0, 0, 12, 0, 10, 0)], [[(7, EQ), (2, I), (3, EQ)]], [read])
    assert events == [(0, 2, b"AC")] and channel(got, "INS") == [1] + [0] * 9  # six steps: three whole turns
    got, events = run(block, [aln(0, 0, 12, 0, 10, 0)], [[(6, EQ), (2, I), (4, EQ)]], [read])
    assert events == [(0, 2, b"AC")]                                        # five steps from one base earlier: CA -> AC
    rev = am.revcomp(read)
    back, events_r = run(block, [aln(0, 0, 12, 0, 10, 1)], [[(9, EQ), (2, I), (1, EQ)]], [rev])
    assert events_r == [(0, 2, b"AC")] and channel(back, "INS") == channel(got, "INS")
    # one step only: the rotation by one (TG inserted behind ..T: the shift stops at the C)
    got, events = run(b"ACTGA", [aln(0, 0, 7, 0, 5, 0)], [[(3, EQ), (2, I), (2, EQ)]], [b"ACTGTGA"])
    assert events == [(1, 2, b"TG")] and channel(got, "INS") == [0, 1, 0, 0, 0]
    # a shift of n + 1 wraps: AAA inserted in AAAA, capped by the `=` run of 4
    got, events = run(b"AAAAC", [aln(0, 0, 8, 0, 5, 0)], [[(4, EQ), (3, I), (1, EQ)]], [b"AAAAAAAC"])
    assert events == [(0, 3, b"AAA")]
    # what cannot shift: behind an X, behind another gap, as the first op
    got, events = run(b"CAAG", [aln(0, 0, 5, 0, 4, 0)], [[(1, EQ), (1, X), (1, I), (2, EQ)]], [b"CTAAG"])
    assert events == [(1, 1, b"A")]
    got, events = run(b"CAAAG", [aln(0, 0, 5, 0, 5, 0)], [[(2, EQ), (1, D), (1, I), (2, EQ)]], [b"CAAAG"])
    assert events == [(2, 1, b"A")] and channel(got, "DEL") == [0, 1, 0, 0, 0]  # the D moved, the I behind it did not
    got, events = run(b"AAAG", [aln(0, 0, 5, 0, 4, 0)], [[(1, I), (4, EQ)]], [b"AAAAG"])
    assert events == [(0, 1, b"A")]


def test_alleles_and_the_consensus_of_a_hand_made_table():
    block = b"ACG\x01TT"
    counts = np.zeros((6, 8), dtype=np.uint32)
    counts[0, :5] = (4, 0, 0, 0, 0)
    counts[1, :5] = (0, 1, 0, 3, 0)      # C -> T
    counts[2, :5] = (0, 0, 1, 0, 3)      # deleted
    counts[4, :5] = (0, 0, 0, 2, 0)
    counts[5, :5] = (0, 0, 2, 0, 2)      # a tie between G and DEL: the smaller channel, G
    events = [(0, 2, b"GT")] * 2 + [(0, 2, b"GA")] * 2 + [(0, 1, b"T")] + [(2, 3, b"CCC")] * 3 + [(4, 70, b"A" * 64)] * 2
    table = km.alleles(events)
    assert [(p, n, c) for p, n, w, c in table] == [(0, 1, 1), (0, 2, 2), (0, 2, 2), (2, 3, 3), (4, 70, 2)]
    assert km.bases_of(2, table[1][2]) == b"GA" and km.bases_of(2, table[2][2]) == b"GT"
    counts[0, pm.INS], counts[2, pm.INS], counts[4, pm.INS] = 5, 3, 2
    got = km.consensus(counts, table, block, 1, 1, 2, 0)
    # 0: A, then the first of the tied alleles GA; 1: T; 2: deleted, the insertion stays; 4: truncated, skipped; 5: G
    assert got["text"] == b"AGATCCC\x01TG" and got["records"] == [b"AGATCCC", b"TG"]
    assert got["starts"] == [0, 3, 4, 7, 8, 9, 10]
    assert [got[name] for name in km.STATS] == [5, 0, 2, 1, 2, 5, 1]
    low = km.consensus(counts, table, block, 3, 1, 2, 1)  # position 4 is below the depth: N, and no insertion is looked at
    assert low["text"] == b"AGATCCC\x01NG" and low["low_positions"] == 1 and low["truncated_skipped"] == 0
    keep = km.consensus(counts, table, block, 1, 1, 1, 0)  # 1 / 1: only the unanimous position is called
    assert keep["text"] == b"ACG\x01TT" and keep["called"] == 2 and keep["low_positions"] == 3
    recs = km.insertions(table, counts, [0, 4], 2, 1, 2)
    assert [r[:8] for r in recs] == [(0, 0, 0, 2, 2, 4, 5, 0), (0, 0, 0, 2, 2, 4, 5, 0), (2, 2, 0, 3, 3, 4, 3, 0), (4, 0, 1, 70, 2, 2, 2, 1)]


@pytest.mark.parametrize("seed", SAMPLE_SEEDS)
def test_the_normalised_consensus_of_the_planted_sample_is_the_sample(seed):
    """the condition of the end-to-end test on the all-CPU path: chain model, align model, walk, consensus"""
    ref, reads, sample, exp = sample_alignments(seed)
    recs = pm.records(exp)
    counts, events = km.walk(ref, recs, exp["ops"], exp["op_offsets"], reads, True, True)
    got = km.consensus(counts, km.alleles(events), ref, 1, 1, 2, 0)
    assert got["records"] == [sample] and got["deleted"] == 3 and got["inserted_bases"] == 2 and got["substitutions"] == 5
    # every read aligns to the consensus with edit distance 0
    params = dict(am.DEFAULTS)
    band, max_flank = params.pop("band"), params.pop("max_flank")
    again = am.expected([sample], reads, cm.expected([sample], reads, True, **params), band, max_flank)
    best = {}
    for c in range(len(again["target"])):
        if again["primary"][c]:
            best[int(again["target"][c])] = (int(again["edit_distance"][c]), int(again["t_end"][c] - again["t_start"][c]))
    assert best == {j: (0, 100) for j in range(len(reads))}


def test_without_normalisation_the_consensus_of_seed_3_is_not_the_sample():
    ref, reads, sample, exp = sample_alignments(3)
    counts, events = km.walk(ref, pm.records(exp), exp["ops"], exp["op_offsets"], reads, True, False)
    got = km.consensus(counts, km.alleles(events), ref, 1, 1, 2, 0)
    assert got["records"] != [sample]


def test_symbols_layouts_and_exports():
    header = open(_lib.__file__.replace("nolzss_amd/_lib.py", "include/nolzss_hip.h")).read()
    for name in ("nolzss_rlz_pileup_open_flags", "nolzss_rlz_pileup_log_info", "nolzss_rlz_pileup_insertions",
                 "nolzss_free_rlz_insertions_result", "nolzss_rlz_pileup_consensus", "nolzss_free_rlz_consensus_result",
                 "nolzss_debug_rlz_pileup_consensus"):
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(_lib.lib, name) and f"{name}(" in header
    for text in ("#define NOLZSS_RLZ_PILEUP_NORMALIZE 1u", "#define NOLZSS_RLZ_PILEUP_MAX_SHIFT 1024", "#define NOLZSS_RLZ_PILEUP_INS_BASES 64"):
        assert text in header
    assert INSERTION_DTYPE.itemsize == C.sizeof(_lib.RlzInsertion) == 56
    assert native.INSERTION_DTYPE.names == tuple(name for name, _ in _lib.RlzInsertion._fields_) == km.INSERTION_FIELDS
    assert C.sizeof(_lib.RlzConsensusParams) == 24 and C.sizeof(_lib.RlzInsertionsResult) == 16
    assert C.sizeof(_lib.RlzConsensusResult) == 5 * 8 + 7 * 8
    assert native.CONSENSUS_STATS == km.STATS and (native.PILEUP_NORMALIZE, native.PILEUP_INS_BASES) == (1, km.INS_BASES)
    assert C.sizeof(_lib.RlzPileupAddInfo) == 32 and C.sizeof(_lib.RlzPileupSummary) == 64 + C.sizeof(_lib.RlzAlignParams)  # kept
    import noLZSS.genomics.rlz as shim
    from nolzss_amd.genomics import rlz
    for name in ("INSERTION_DTYPE", "insertion_bases"):
        assert name in rlz.__all__ and name in shim.__all__ and getattr(shim, name) is getattr(rlz, name) is getattr(native, name)
    for method in ("insertions", "consensus"):
        assert hasattr(rlz.RlzPileup, method) and hasattr(native.RlzPileupHandle, method)
    assert hasattr(native, "debug_rlz_pileup_consensus")
    rec = np.zeros(1, dtype=native.INSERTION_DTYPE)[0]
    rec["length"], rec["bases"] = 33, km.words_of(b"ACGT" * 8 + b"G")
    assert insertion_bases(rec) == b"ACGT" * 8 + b"G"
    rec["length"] = 70
    assert len(native.insertion_bases(rec)) == 64


def test_bad_arguments_raise_before_the_native_layer_is_touched():
    from nolzss_amd.genomics import rlz
    ix = rlz.RlzIndex.__new__(rlz.RlzIndex)
    ix._handle = None
    with pytest.raises(ValueError, match="the index is closed"):
        ix.pileup(normalize_indels=True)
    pile = rlz.RlzPileup(None, ix, True)  # closed: anything that reached for the handle would say so
    for count, fraction in ((0, (1, 2)), (2, (3, 2)), (2, (1, 0)), (2, (-1, 2)), (2, 0.5), (1 << 32, (1, 2))):
        with pytest.raises(ValueError, match="min_count|min_fraction"):
            pile.insertions(count, fraction)
    for kwargs in (dict(min_depth=0), dict(min_depth=1 << 32), dict(min_fraction=(3, 2)), dict(min_fraction=(1, 0)),
                   dict(min_fraction=(1, 1 << 32)), dict(min_fraction=0.5), dict(low="n"), dict(low=1)):
        with pytest.raises(ValueError, match="min_depth|min_fraction|low is"):
            pile.consensus(**kwargs)
    for call in (lambda: pile.insertions(), lambda: pile.consensus()):
        with pytest.raises(ValueError, match="the pileup is closed"):
            call()
    pile.close()


def test_refusals_before_any_device_work():
    lib, bad = _lib.lib, _lib.ERR_INVALID_ARGUMENT
    params, out = _lib.RlzAlignParams(15, 64, 5000, 31, 40, 16, 256), C.c_void_p(5)
    stand_in = C.create_string_buffer(4096)  # zero bytes stand in for a handle where it is not read
    for flags in (2, 3, 1 << 31):
        assert lib.nolzss_rlz_pileup_open_flags(stand_in, C.byref(params), flags, C.byref(out)) == bad
        assert b"unknown flag bits" in lib.nolzss_last_error() and not out.value
    assert lib.nolzss_rlz_pileup_open_flags(stand_in, C.byref(params), 1, None) == bad
    assert lib.nolzss_rlz_pileup_open_flags(None, C.byref(params), 1, C.byref(out)) == bad
    assert b"handle is null" in lib.nolzss_last_error()
    assert lib.nolzss_rlz_pileup_open_flags(stand_in, None, 1, C.byref(out)) == bad
    wide = _lib.RlzAlignParams(15, 64, 5000, 31, 40, 17, 256)
    assert lib.nolzss_rlz_pileup_open_flags(stand_in, C.byref(wide), 1, C.byref(out)) == bad
    assert b"at most 64 diagonals" in lib.nolzss_last_error()
    flags, events, log_bytes = C.c_uint32(), C.c_uint64(), C.c_uint64()
    assert lib.nolzss_rlz_pileup_log_info(None, C.byref(flags), C.byref(events), C.byref(log_bytes)) == bad
    assert lib.nolzss_rlz_pileup_log_info(stand_in, None, C.byref(events), C.byref(log_bytes)) == bad
    res = _lib.RlzInsertionsResult(7, None)
    assert lib.nolzss_rlz_pileup_insertions(stand_in, 2, 1, 2, None) == bad
    assert lib.nolzss_rlz_pileup_insertions(None, 2, 1, 2, C.byref(res)) == bad
    assert b"handle is null" in lib.nolzss_last_error() and res.num_insertions == 0
    for min_count, num, den in ((2, 1, 0), (2, 3, 2), (0, 1, 2), (2, 1, 1 << 32)):
        assert lib.nolzss_rlz_pileup_insertions(stand_in, min_count, num, den, C.byref(res)) == bad, (min_count, num, den)
        assert b"rlz pileup: " in lib.nolzss_last_error() and not res.insertions
    cons = _lib.RlzConsensusResult()
    good = _lib.RlzConsensusParams(1, 0, 1, 2)
    assert lib.nolzss_rlz_pileup_consensus(stand_in, C.byref(good), 1, None) == bad
    assert lib.nolzss_rlz_pileup_consensus(None, C.byref(good), 1, C.byref(cons)) == bad
    assert lib.nolzss_rlz_pileup_consensus(stand_in, None, 1, C.byref(cons)) == bad
    for min_depth, low, num, den in ((0, 0, 1, 2), (1, 2, 1, 2), (1, 0, 1, 0), (1, 0, 3, 2), (1, 0, 1, 1 << 32)):
        refused = _lib.RlzConsensusParams(min_depth, low, num, den)
        assert lib.nolzss_rlz_pileup_consensus(stand_in, C.byref(refused), 0, C.byref(cons)) == bad, (min_depth, low, num, den)
        assert b"rlz pileup: " in lib.nolzss_last_error() and not cons.text and not cons.starts
    lib.nolzss_free_rlz_insertions_result(None)
    lib.nolzss_free_rlz_consensus_result(None)
    lib.nolzss_free_rlz_insertions_result(C.byref(res))
    lib.nolzss_free_rlz_consensus_result(C.byref(cons))
    assert cons.length == 0 and not cons.record_offsets


def test_the_debug_hook_refuses_what_the_pileup_hook_refuses():
    def hook(alignments, ops_per_alignment, targets=(b"GTTACAG",), block=b"ACGTTGCAAGGCTA", **kwargs):
        recs = np.zeros(len(alignments), dtype=native.ALIGN_DTYPE)
        ops, off = [], [0]
        for c, (a, mine) in enumerate(zip(alignments, ops_per_alignment)):
            for key, v in a.items():
                recs[key][c] = v
            ops += op_words(mine)
            off.append(len(ops))
        return native.debug_rlz_pileup_consensus(block, list(targets), recs, off, ops, **kwargs)

    OPS = [(3, EQ), (1, X), (2, D), (1, I), (2, EQ)]
    good = aln(0, 0, 7, 2, 10, 0)
    for a, mine, text in ((dict(good, target=1), OPS, "beyond the batch"), (dict(good, t_end=8), OPS, "leaves its target"),
                          (dict(good, r_start=7, r_end=15), OPS, "leaves the block"), (dict(good, r_end=11), OPS, "consume exactly"),
                          (good, OPS[:-1] + [(2, 3)], "unknown code"), (good, OPS[:-1] + [(0, EQ), (2, EQ)], "length 0"),
                          (good, [], "no ops")):
        with pytest.raises(ValueError, match=text):
            hook([a], [mine])
    with pytest.raises(ValueError, match="covers a separator"):
        hook([aln(0, 0, 6, 2, 8, 0)], [[(6, EQ)]], block=b"ACGT\x01TGCA")
    with pytest.raises(ValueError, match="invalid base"):
        hook([good], [OPS], targets=(b"GTTNCAG",))
    for kwargs in (dict(min_depth=0), dict(min_fraction=(2, 1)), dict(low="x")):
        with pytest.raises(ValueError, match="min_depth|min_fraction|low is"):
            hook([good], [OPS], **kwargs)
    bad_params = _lib.RlzConsensusParams(0, 0, 1, 2)
    ins, cons = _lib.RlzInsertionsResult(), _lib.RlzConsensusResult()
    assert _lib.lib.nolzss_debug_rlz_pileup_consensus(None, 0, None, None, 0, None, None, 0, None, 0, 0, 0, C.byref(bad_params), 0,
                                                      None, C.byref(ins), C.byref(cons)) == _lib.ERR_INVALID_ARGUMENT
    fine = _lib.RlzConsensusParams(1, 0, 1, 2)
    assert _lib.lib.nolzss_debug_rlz_pileup_consensus(None, 0, None, None, 0, None, None, 0, None, 0, 0, 2, C.byref(fine), 0,
                                                      None, C.byref(ins), C.byref(cons)) == _lib.ERR_INVALID_ARGUMENT
    assert b"unknown flag bits" in _lib.lib.nolzss_last_error()
