"""Maximal match seeds of the relative-LZ index without a GPU: the ms formulation the kernels run
(tests/rlz_seeds_model.ms_seeds) against the definition stated directly (brute_seeds), the interval of every seed
(rlz_locate_model.LocateModel) against the brute force of a locate, and what the library and the Python layers decide on
the host."""
import ctypes as C
import random

import numpy as np
import pytest

import rlz_locate_model as lm
import rlz_seeds_model as sm
from nolzss_amd import _lib
from nolzss_amd import _noLZSS as native

CASES = 320


@pytest.fixture(scope="module")
def cases():
    """[(refs, with_rc, target, ms, seeds)] -- computed once, shared and left unchanged"""
    rng = random.Random(20261020)
    out = []
    for n_case in range(CASES):
        with_rc = n_case % 2 == 0
        refs = lm.case(rng, hi=40 if n_case % 3 == 0 else 16)
        t = sm.target(rng, refs)
        out.append((refs, with_rc, t, sm.ms_array(refs, t, with_rc), sm.ms_seeds(refs, t, with_rc)))
    return out


def test_ms_seeds_are_the_seeds_of_the_definition(cases):
    for refs, with_rc, t, _, seeds in cases:
        assert seeds == sm.brute_seeds(refs, t, with_rc), (refs, t, with_rc)
    assert sum(with_rc for _, with_rc, *_ in cases) == CASES // 2


def test_the_interval_of_every_seed_is_its_locate(cases):
    total = repeated = positions = 0
    for refs, with_rc, t, ms, seeds in cases:
        ix = lm.LocateModel(refs, with_rc)
        up = t.upper()
        positions += len(up)
        for p, L in seeds:
            piece = up[p:p + L]
            exp = lm.brute_locate(refs, piece, with_rc)
            assert ix.interval(piece)[1] == len(exp) >= 1, (refs, piece, with_rc)
            assert ix.locate(piece) == exp, (refs, piece, with_rc)
            total += 1
            repeated += len(exp) > 1
    # the inputs are not vacuous
    assert total >= 2000 and positions >= 6000, (total, positions)
    assert repeated >= 0.10 * total, repeated / total


def test_ms_drops_by_at_most_one(cases):
    for refs, with_rc, t, ms, _ in cases:
        assert all(ms[p + 1] >= ms[p] - 1 for p in range(len(ms) - 1)), (refs, t, with_rc)
        # and each ms[p] is the longest match by the definition, not only by the incremental start
        up, rs = t.upper(), [r.upper() for r in refs]
        for p in range(0, len(up), 3):
            assert ms[p] == max([L for L in range(1, len(up) - p + 1) if sm.occurs(rs, up[p:p + L], with_rc)] + [0])


def test_min_length_never_creates_a_seed(cases):
    kept = 0
    for refs, with_rc, t, _, seeds in cases:
        for m in (0, 1, 2, 5, 9, 1000):
            got = sm.ms_seeds(refs, t, with_rc, min_length=m)
            assert got == [s for s in seeds if s[1] >= max(m, 1)], (refs, t, with_rc, m)
            kept += len(got)
    assert kept >= 4000


def test_hand_cases_of_the_model():
    refs = [b"ACGTTGCA", b"GGATCC"]
    assert sm.ms_seeds(refs, refs[0]) == [(0, 8)] == sm.brute_seeds(refs, refs[0])
    joined = refs[0] + refs[1]  # nothing crosses the record boundary
    assert sm.brute_seeds(refs, joined, False) == sm.ms_seeds(refs, joined, False) == [(0, 8), (8, 6)]
    assert sm.ms_seeds([b"AAAA"], b"CCGG") == [] and sm.ms_seeds([b"AAAA"], b"TT", True) == [(0, 2)]
    assert sm.ms_seeds([b"AAAA"], b"TT", False) == []
    exp = sm.expected([b"CCGAATTCCC"], [b"", b"tGAATTC", b"G"], True)
    assert exp["target"].tolist() == [1, 1, 2] and exp["start"].tolist() == [0, 1, 0] and exp["length"].tolist() == [1, 6, 1]
    lo = int(exp["offsets"][1])  # GAATTC is its own reverse complement: one position, forward first
    assert exp["position"][lo:lo + 2].tolist() == [2, 2] and exp["is_rc"][lo:lo + 2].tolist() == [False, True]
    capped = sm.expected([b"CCGAATTCCC"], [b"", b"tGAATTC", b"G"], True, max_hits=2)
    assert capped["counts"].tolist() == exp["counts"].tolist() and capped["offsets"].tolist() == [0, 0, 2, 2]


# ---- what needs no device ----------------------------------------------------------------------------------------
def test_symbols_and_layouts():
    for name in ("nolzss_rlz_index_seeds", "nolzss_free_rlz_seeds_result"):
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(_lib.lib, name)
    assert native.SEED_DTYPE.itemsize == 32 and native.SEED_DTYPE.names == ("target", "start", "length", "count")
    assert C.sizeof(_lib.RlzSeedsResult) == 5 * C.sizeof(C.c_void_p)


def test_both_packages_carry_the_query():
    import noLZSS.genomics.rlz as ref_path
    import nolzss_amd.genomics.rlz as amd_path
    for mod in (ref_path, amd_path):
        assert "SEED_DTYPE" in mod.__all__ and mod.SEED_DTYPE is native.SEED_DTYPE
        assert callable(mod.RlzIndex.seeds)
    assert callable(native.RlzIndexHandle.seeds)


def test_null_pointers_are_refused_with_the_argument_error():
    lib = _lib.lib
    pt, ln = (C.c_char_p * 1)(b"ACGT"), (C.c_size_t * 1)(4)
    res = _lib.RlzSeedsResult()
    res.num_seeds = 7
    assert lib.nolzss_rlz_index_seeds(None, pt, ln, 1, 1, 0, C.byref(res)) == _lib.ERR_INVALID_ARGUMENT
    assert b"handle is null" in lib.nolzss_last_error()
    assert res.num_seeds == 0 and not res.seeds and not res.hit_offsets and not res.hits
    assert lib.nolzss_rlz_index_seeds(None, None, None, 0, 1, 0, C.byref(res)) == _lib.ERR_INVALID_ARGUMENT
    assert lib.nolzss_rlz_index_seeds(None, pt, ln, 1, 1, 0, None) == _lib.ERR_INVALID_ARGUMENT
    assert b"output pointer is null" in lib.nolzss_last_error()
    lib.nolzss_free_rlz_seeds_result(C.byref(res))  # an empty result, and NULL: no-ops
    lib.nolzss_free_rlz_seeds_result(None)


def test_use_after_close_and_negative_arguments_raise_value_error():
    from nolzss_amd.genomics import rlz
    ix = rlz.RlzIndex(None, [b"ACGT"])  # (a closed index: no device is needed to make one)
    with pytest.raises(ValueError, match="closed"):
        ix.seeds([b"AC"])
    with pytest.raises(ValueError, match="closed"):
        ix.seeds([b"AC"], min_length=-1)


def test_the_expected_dict_has_the_dtypes_of_a_locate():
    exp = sm.expected([b"ACGT"], [b"ACG"], True)
    assert [exp[k].dtype for k in ("target", "start", "length", "counts", "offsets", "position", "record_offset")] == \
        [np.dtype(np.uint64)] * 7
    assert exp["record"].dtype == np.uint32 and exp["is_rc"].dtype == bool
