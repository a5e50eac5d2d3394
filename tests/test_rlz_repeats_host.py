"""The two models of the maximal repeats of the reference (tests/rlz_repeats_model.py) against each other and against
hand cases with the expected records written out, and the host-side pieces of nolzss_rlz_index_repeats: the decision on
the totals, the sort digits, the names.  No GPU."""
import ctypes as C
import random
from pathlib import Path

import numpy as np
import pytest

import rlz_locate_model as lm
import rlz_model as model
import rlz_repeats_model as rm


def both(refs, with_rc, min_length=1, min_count=2):
    a = rm.brute_repeats(refs, with_rc, min_length, min_count)
    m = rm.RepeatsModel(refs, with_rc)
    b = m.records(min_length, min_count)
    assert a == b, (refs, with_rc, min_length, min_count)
    keys = [(r[0][0], r[0][1]) for r in a]
    assert len(set(keys)) == len(keys) and keys == sorted(keys), "the order key (position, length) is unique"
    d = m.repeats(min_length, min_count)  # the dict form agrees with the records, and asserts the unique key itself
    assert list(zip(d["position"].tolist(), d["length"].tolist(), d["count"].tolist(), d["record"].tolist(),
                    d["palindrome"].astype(int).tolist())) == [r[0] for r in a]
    assert m.repeat_count(min_length, min_count) == len(a)
    return a


# ---- 1. the two models on seeded cases ---------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(8))
def test_the_definition_equals_the_array_formulation(seed):
    rng = random.Random(9000 + seed)
    reported = palindromes = capped = 0
    for i in range(60):  # 480 cases in all: the alphabets of the locate model, 1 to 5 records, both kinds of index
        refs = lm.case(rng, hi=24 if i % 6 else 60)
        with_rc = bool((i + seed) & 1)
        got = both(refs, with_rc, rng.choice((1, 1, 2, 3, 5)), rng.choice((2, 2, 3, 4, 6)))
        reported += len(got)
        palindromes += sum(r[0][4] for r in got)
        capped += sum(1 for r in got if r[0][2] >= 8)
    assert reported >= 200 and palindromes >= 3 and capped >= 10  # nested, periodic and palindromic repeats are met


@pytest.mark.parametrize("seed", range(4))
def test_the_suffix_array_of_the_model_is_the_sorted_one(seed):
    rng = random.Random(9100 + seed)
    for i in range(40):
        m = rm.RepeatsModel(lm.case(rng, hi=40), bool(i & 1))
        sa, lcp = model.python_sa_lcp(m.X)
        assert np.array_equal(sa, m.sa) and np.array_equal(lcp, m.lcp)


def test_min_length_and_min_count_only_filter():
    rng = random.Random(9200)
    for i in range(40):
        refs, with_rc = lm.case(rng, hi=30), bool(i & 1)
        everything = both(refs, with_rc)
        for min_length, min_count in ((2, 2), (1, 3), (3, 4)):
            kept = [r for r in everything if r[0][1] >= min_length and r[0][2] >= min_count]
            assert both(refs, with_rc, min_length, min_count) == kept


# ---- 2. hand cases -----------------------------------------------------------------------------------------------------
def heads(records):
    return [r[0] for r in records]


@pytest.mark.parametrize("n", [2, 3, 6, 17])
def test_a_run_of_one_base(n):
    got = both([b"A" * n], False)
    assert heads(got) == [(0, k, n - k + 1, 0, 0) for k in range(1, n)]  # A^k, k = 1 .. n - 1, n - k + 1 times
    assert [h for _, h in got] == [[(a, 0, 0) for a in range(n - k + 1)] for k in range(1, n)]
    # with the reverse complement the mirrored block holds T^n: no occurrence of A^k is added, T^k has no forward one
    assert heads(both([b"A" * n], True)) == heads(got)


def test_a_lone_palindrome_is_no_repeat():
    assert both([b"ACGT"], True) == []
    assert both([b"ACGT"], False) == []
    # GAATTC at one locus is no repeat either; A is one: at 1 and 2, and as T at 3 and 4.  AA is none: both of its
    # occurrences -- forward at 1, reverse strand at 3 -- go on with T.
    assert both([b"GAATTC"], True) == [((1, 1, 4, 0, 0), [(1, 0, 0), (2, 0, 0), (3, 0, 1), (4, 0, 1)])]


def test_a_palindrome_at_two_loci():
    got = both([b"ACGT", b"ACGT"], True)
    assert got == [((0, 4, 4, 0, 1), [(0, 0, 0), (0, 0, 1), (5, 1, 0), (5, 1, 1)])]
    assert both([b"ACGT", b"ACGT"], True, min_count=5) == []  # min_count applies to the count as stated
    assert both([b"ACGT", b"ACGT"], False) == [((0, 4, 2, 0, 0), [(0, 0, 0), (5, 1, 0)])]


def test_an_inverted_pair():
    w = b"CAGGT"
    ref = w + b"T" + model.revcomp(w)
    assert ref == b"CAGGTTACCTG"
    # one record at the left copy: one forward and one reverse-strand hit
    assert both([ref], True, min_length=3) == [((0, 5, 2, 0, 0), [(0, 0, 0), (6, 0, 1)])]
    assert both([ref], False, min_length=3) == []


def test_a_repeat_that_touches_a_record_start_and_a_record_end():
    refs = [b"ACGTCC", b"GGACGT"]
    assert both(refs, False, min_length=3) == [((0, 4, 2, 0, 0), [(0, 0, 0), (9, 1, 0)])]
    # with the reverse complement ACGT is its own mirror image: two loci, every locus on both strands
    assert ((0, 4, 4, 0, 1), [(0, 0, 0), (0, 0, 1), (9, 1, 0), (9, 1, 1)]) in both(refs, True, min_length=3)


def test_a_separator_does_not_extend_a_repeat():
    refs = [b"GGACG", b"TTTCC", b"AACGTTTA"]  # ACG | TTT across the separator, ACGTTT inside the third record
    assert both(refs, False, min_length=3) == [((2, 3, 2, 0, 0), [(2, 0, 0), (13, 2, 0)]),
                                                ((6, 3, 2, 1, 0), [(6, 1, 0), (16, 2, 0)])]
    assert not any(r[0][1] > 3 for r in both(refs, True, min_length=3))
    assert not rm.is_maximal_repeat(refs, b"ACGTTT", True) and rm.is_maximal_repeat(refs, b"ACG", False)


def test_nested_and_periodic_repeats():
    got = both([b"ACACACAC"], False)
    # A always goes on with C, and everything that starts with C has A in front of it: (AC)^k, k = 1 .. 3, is what is left
    assert heads(got) == [(0, 2, 4, 0, 0), (0, 4, 3, 0, 0), (0, 6, 2, 0, 0)]


def test_empty_records_and_one_base():
    assert both([b"A"], True) == [] and both([b"", b"A", b""], True) == []
    assert both([b"A", b"A"], False) == [((0, 1, 2, 0, 0), [(0, 0, 0), (2, 1, 0)])]
    assert both([b"A", b"", b"T"], True) == [((0, 1, 2, 0, 0), [(0, 0, 0), (3, 2, 1)])]


# ---- 3. the host side of the library -----------------------------------------------------------------------------------
def test_the_decision_on_the_totals():
    from nolzss_amd import _lib
    from nolzss_amd.genomics import rlz
    f = _lib.lib.nolzss_debug_rlz_repeats_refusal

    def message():
        return _lib.lib.nolzss_last_error().decode()

    assert f(0, 0, 0, 1) == _lib.OK and f((1 << 31) - 1, rlz.MAX_TEXT, 64, 20) == _lib.OK
    assert f(5, rlz.MAX_TEXT + 1, 7, 20) == _lib.ERR_INVALID_ARGUMENT
    assert f"repeats would report {rlz.MAX_TEXT + 1} hits" in message() and "max_hits (it is 7" in message() and \
        "min_length (it is 20)" in message()
    for total in ((1 << 32) - 1, 1 << 32, (1 << 32) + 1, 1 << 40):
        assert f(5, total, 0, 12) == _lib.ERR_INVALID_ARGUMENT and str(total) in message()
    assert f(1 << 31, 0, 0, 3) == _lib.ERR_INVALID_ARGUMENT  # the sort key of a hit keeps its record in 31 bits
    assert f"2^31 - 1 records, this one has {1 << 31}" in message() and "min_length (it is 3)" in message()


def test_the_sort_digits_cover_the_key():
    from nolzss_amd import _lib
    for B in (1, 2, 255, 256, 257, 65535, 65536, (1 << 24) + 1, (1 << 31) - 1, 1 << 31, (1 << 32) - (1 << 19) - 1):
        shifts, npasses = (C.c_int * 8)(), C.c_int()
        assert _lib.lib.nolzss_debug_rlz_repeat_shifts(B, shifts, C.byref(npasses)) == _lib.OK
        got = list(shifts[:npasses.value])
        assert got == sorted(got) and len(got) <= 8 and all(s % 8 == 0 for s in got)
        covered = 0
        for s in got:
            covered |= 0xff << s
        assert covered & B == B and covered & (B << 32) == B << 32  # every bit of a length <= B and of a position <= B
        assert len(got) == 2 * -(-B.bit_length() // 8)  # and no digit that cannot differ


def test_names():
    from nolzss_amd import _lib, _noLZSS as native
    from nolzss_amd.genomics import rlz
    import noLZSS.genomics.rlz as shim
    header = (Path(__file__).resolve().parent.parent / "include" / "nolzss_hip.h").read_text()
    for name in ("nolzss_rlz_index_repeat_count", "nolzss_rlz_index_repeats", "nolzss_free_rlz_repeats_result",
                 "nolzss_debug_rlz_repeats_refusal", "nolzss_debug_rlz_repeat_shifts"):
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(_lib.lib, name) and f"{name}(" in header
    assert "REPEAT_DTYPE" in rlz.__all__ and "REPEAT_DTYPE" in shim.__all__ and shim.REPEAT_DTYPE is rlz.REPEAT_DTYPE
    assert rlz.REPEAT_DTYPE.names == ("position", "length", "count", "record", "palindrome") and rlz.REPEAT_DTYPE.itemsize == 32
    assert callable(rlz.RlzIndex.repeats) and callable(rlz.RlzIndex.repeat_count) and callable(native.RlzIndexHandle.repeats)
    # size_t, three pointers, size_t: no padding on a 64-bit host
    assert C.sizeof(_lib.RlzRepeatsResult) == 40 and [n for n, _ in _lib.RlzRepeatsResult._fields_] == \
        ["num_repeats", "repeats", "hit_offsets", "hits", "num_hits"]
