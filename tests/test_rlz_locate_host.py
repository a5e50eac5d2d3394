"""Pattern count and locate on the relative-LZ index without a GPU: the interval formulation the kernels run
(tests/rlz_locate_model.LocateModel) against the brute force of the definition, and what the library and the Python
layers decide on the host."""
import ctypes as C
import random

import numpy as np
import pytest

import rlz_locate_model as locate_model
import rlz_model as model
from nolzss_amd import _lib
from nolzss_amd import _noLZSS as native


def test_interval_model_matches_the_brute_force():
    rng = random.Random(20261019)
    pairs = with_hit = many = self_rc = at_end = 0
    per_record = {(rec, rc): 0 for rec in range(5) for rc in (0, 1)}
    for n_case in range(260):
        with_rc = n_case % 4 != 3
        refs = locate_model.case(rng, hi=40 if n_case % 3 == 0 else 16)
        ix = locate_model.LocateModel(refs, with_rc)
        ends = {start + len(r) for start, r in zip(locate_model.record_starts(refs), refs) if r}
        for p in locate_model.patterns(rng, refs, 20):
            exp = locate_model.brute_locate(refs, p, with_rc)
            assert ix.locate(p) == exp, (refs, p, with_rc)
            assert ix.count(p) == len(exp), (refs, p, with_rc)
            pairs += 1
            with_hit += bool(exp)
            many += len(exp) > 8
            up = p.upper()
            self_rc += bool(exp) and up == model.revcomp(up)
            at_end += any(not rc and pos + len(p) in ends for pos, _, rc in exp)
            for _, rec, rc in exp:
                per_record[rec, rc] += 1
    # the inputs are not vacuous
    assert pairs >= 5000
    assert with_hit >= 0.40 * pairs, with_hit / pairs
    assert many >= 0.10 * pairs, many / pairs
    assert self_rc >= 20 and at_end >= 50, (self_rc, at_end)
    assert min(per_record.values()) >= 50, per_record


def test_hand_cases_of_the_model():
    site = b"GAATTC"  # its own reverse complement: counted on both strands, forward first
    ix = locate_model.LocateModel([b"CC" + site + b"CC"], True)
    assert ix.locate(site) == [(2, 0, 0), (2, 0, 1)] == locate_model.brute_locate([b"CC" + site + b"CC"], site, True)
    assert locate_model.LocateModel([b"CC" + site + b"CC"], False).locate(site) == [(2, 0, 0)]
    refs = [b"ACGT", b"", b"GTAC"]
    ix = locate_model.LocateModel(refs, True)
    assert ix.locate(b"GTG") == [] and ix.locate(b"") == [] and ix.count(b"TGT") == 0  # nothing crosses R1 | R3
    # GT: forward in record 0 at 2 and record 2 at 6; AC is its reverse complement, at 0 and 8
    assert ix.locate(b"gt") == [(0, 0, 1), (2, 0, 0), (6, 2, 0), (8, 2, 1)]


# ---- what needs no device ----------------------------------------------------------------------------------------
def test_symbols_are_exported():
    for name in ("nolzss_rlz_index_count", "nolzss_rlz_index_locate"):
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(_lib.lib, name)
    assert C.sizeof(C.c_uint64) * 2 == native.HIT_DTYPE.itemsize == 16
    assert native.HIT_DTYPE.names == ("position", "record", "is_rc")


def test_both_packages_carry_the_queries():
    import noLZSS.genomics.rlz as ref_path
    import nolzss_amd.genomics.rlz as amd_path
    for mod in (ref_path, amd_path):
        assert "HIT_DTYPE" in mod.__all__ and mod.HIT_DTYPE is native.HIT_DTYPE
        assert callable(mod.RlzIndex.count) and callable(mod.RlzIndex.locate)
    assert ref_path.RlzIndex is amd_path.RlzIndex
    assert callable(native.RlzIndexHandle.count) and callable(native.RlzIndexHandle.locate)


def test_a_null_handle_is_refused_with_the_argument_error():
    lib = _lib.lib
    pt, ln = (C.c_char_p * 1)(b"ACGT"), (C.c_size_t * 1)(4)
    counts, offsets = np.zeros(1, dtype=np.uint64), np.zeros(2, dtype=np.uint64)
    hits, z = C.c_void_p(), C.c_size_t()
    assert lib.nolzss_rlz_index_count(None, pt, ln, 1, counts.ctypes.data) == _lib.ERR_INVALID_ARGUMENT
    assert b"handle is null" in lib.nolzss_last_error()
    assert lib.nolzss_rlz_index_locate(None, pt, ln, 1, 0, counts.ctypes.data, offsets.ctypes.data, C.byref(hits),
                                       C.byref(z)) == _lib.ERR_INVALID_ARGUMENT
    assert b"handle is null" in lib.nolzss_last_error() and not hits.value and z.value == 0
    # q == 0 on a null handle is still a null handle
    assert lib.nolzss_rlz_index_count(None, None, None, 0, None) == _lib.ERR_INVALID_ARGUMENT


def test_use_after_close_raises_value_error():
    from nolzss_amd.genomics import rlz
    ix = rlz.RlzIndex(None, [b"ACGT"])  # (a closed index: no device is needed to make one)
    with pytest.raises(ValueError, match="closed"):
        ix.count([b"AC"])
    with pytest.raises(ValueError, match="closed"):
        ix.locate([b"AC"], max_hits=3)


def test_the_sort_digits_never_straddle_the_key_halves():
    """key = (j << 33) | (position << 1) | is_rc: for every block length and batch size the library accepts, the digits
    are 8 bits wide, ascend, stay inside one 32-bit half of the key, and cover every bit that can be set"""
    lib = _lib.lib
    for B in (1, 2, 127, 128, 1 << 24, (1 << 31) - 1, 1 << 31, rlz_max_text()):
        for q in (1, 2, 129, 1 << 20, 1 << 24, (1 << 24) + 1, (1 << 25) + 1, (1 << 31) - 1):
            shifts, n = (C.c_int * 8)(), C.c_int()
            assert lib.nolzss_debug_rlz_locate_shifts(B, q, shifts, C.byref(n)) == _lib.OK
            got = list(shifts[:n.value])
            assert 1 <= len(got) <= 8 and got == sorted(set(got)), (B, q, got)
            assert all((s & 31) + 8 <= 32 for s in got), (B, q, got)
            covered = {b for s in got for b in range(s, s + 8)}
            largest = ((q - 1) << 33) | (B << 1) | 1  # every bit some key of this batch can set lies below its top bit
            used = set(range(1 + B.bit_length())) | {33 + b for b in range((q - 1).bit_length())}
            assert used <= covered and largest.bit_length() <= max(covered) + 1, (B, q, got)
    assert lib.nolzss_debug_rlz_locate_shifts(1, 1, None, None) == _lib.ERR_INVALID_ARGUMENT


def rlz_max_text():
    from nolzss_amd.genomics import rlz
    return rlz.MAX_TEXT
