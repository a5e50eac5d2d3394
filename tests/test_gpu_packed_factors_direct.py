"""The compact container of factor records on the device against the sequential model
(tests/packed_factors_model.py), section by section and byte for byte: hand-made records are packed with
nolzss_factors_pack, the sections expanded with nolzss_factors_unpack and packed again (factor_pack.hip,
factor_pack_api.hip).  The records need no text: starts near the end of the 32-bit pipeline and steps of 2^31 cost
nothing here."""
import random

import numpy as np
import pytest

import packed_factors_model as model

pytestmark = pytest.mark.gpu

RC = model.RC_MASK
NEAR_END = model.MAX_TEXT - 3_000_000  # starts just below 2^32 - 2^19


@pytest.fixture(scope="module")
def native():
    from nolzss_amd import _noLZSS
    assert _noLZSS.device_count() >= 1, "no MI355X visible"
    return _noLZSS


def check(native, records, literals):
    """pack == the model; unpack gives the records back; packing again gives the same bytes; the same without literals"""
    literals = bytes(literals)
    want = model.pack(records, literals)
    back = model.unpack(want)
    assert np.array_equal(back[0], records) and back[1] == literals
    got = native.pack_factors(records, literals)
    for key in want:
        assert got[key] == want[key], key
    assert set(got) == set(want)
    r2, l2 = native.unpack_factors(got)
    assert r2.dtype == model.FACTOR_DTYPE and np.array_equal(r2, records) and l2 == literals
    assert native.pack_factors(r2, l2) == want
    bare = native.pack_factors(records)
    assert bare == model.pack(records) and bare["literal_mode"] == 2 and bare["literals"] == b""
    r3, l3 = native.unpack_factors(bare)
    assert np.array_equal(r3, records) and l3 is None
    return want


# ---- lengths and codes -----------------------------------------------------------------------------------------------
def test_length_class_edges(native):
    b = model.Builder(1 << 20)
    for L in (1, 255, 256, 65_535, 65_536):
        b.copy(3, L).copy(10, L, rc=True).copy_step(1)
    s = check(native, b.records(), b.literals)
    assert [n & 3 for n in model.nibbles(s)] == [1, 1, 1, 1, 1, 1, 2, 2, 1, 2, 2, 1, 3, 3, 1]


def test_code_class_edges(native):
    b = model.edge_builder()  # v = 0, 2^16 - 1 | 2^16, 2^32 - 1 | 2^32 | 2^32 + 1, 2^33 - 2 | 2^33 - 1
    s = check(native, b.records(), b.literals)
    assert [n >> 2 for n in model.nibbles(s)][1:] == [0, 1, 2, 3, 2, 3, 3, 3]


def test_both_signs_of_small_steps(native):
    b = model.Builder(100_000)
    b.copy(50_000, 10)
    for e in (0, 1, -1, 127, -128, 16_383, -16_384, 16_384, -16_385, 20_000, -20_000):
        b.copy_step(10, e=e)
    s = check(native, b.records(), b.literals)
    assert [n >> 2 for n in model.nibbles(s)][1:] == [0, 1, 1, 1, 1, 1, 1, 2, 2, 2, 2]


# ---- diagonals and strands -------------------------------------------------------------------------------------------
def test_chains_on_both_strands_behind_literals(native):
    b = model.Builder(0)
    for c in b"ACGTACGTTGCA":
        b.literal(bytes([c]))                  # the first record is a literal
    b.copy(0, 4)
    b.literal(b"N").literal(b"A")
    b.copy_step(3)                             # goes on behind two literals: v = 0
    b.copy(10, 5, rc=True)                     # strand toggled, off the diagonal
    b.literal(b"C")
    b.copy_step(4)                             # goes on colinearly on the other strand: v = 0, x falls
    b.copy(1, 9)                               # toggled back
    b.copy_step(4, e=-3)                       # kept, a deletion
    b.copy_step(2, e=5)                        # kept, an insertion
    assert b.codes[15] == 0 and b.codes[18] == 0 and b.rows[18] == (27, 4, RC | 5)
    s = check(native, b.records(), b.literals)
    assert s["literal_mode"] == 0 and s["first_start"] == 0


def test_strand_toggles_on_the_diagonal(native):
    b = model.Builder(3 << 30)                 # a toggle ON the diagonal needs 2^32 - p <= y <= p - L: p beyond 2^31
    b.copy((1 << 30) + 77, 40)
    b.copy_step(12, e=0, toggle=True)          # v = 1
    b.literal(b"G")
    b.copy_step(12, e=0, toggle=True)          # back, behind a literal: v = 1
    b.copy_step(12, e=0)                       # v = 0
    b.copy_step(30, e=-64, toggle=True)        # off the diagonal
    b.copy_step(30, e=64, toggle=True)
    assert [c for c in b.codes if c is not None][1:] == [1, 1, 0, 255, 257]
    check(native, b.records(), b.literals)


def test_first_record_a_reverse_complement_copy(native):
    b = model.Builder(50)
    b.copy(10, 40, rc=True).literal(b"T").copy_step(2).copy(0, 93)
    s = check(native, b.records(), b.literals)
    assert s["first_start"] == 50 and s["decoded"] == 136


def test_starts_near_the_end_of_the_pipeline(native):
    records, literals = model.random_records(random.Random(3), 3000, first_start=NEAR_END, max_length=1000)
    assert NEAR_END < int(records["start"][-1]) < model.MAX_TEXT
    s = check(native, records, literals)
    assert {n >> 2 for n in model.nibbles(s)} >= {0, 2, 3}
    b = model.Builder(model.MAX_TEXT - 10)
    b.copy(model.MAX_TEXT - 20, 10)            # ends on the last position the pipeline takes
    check(native, b.records(), b.literals)


# ---- record counts: odd and even pairs, the scan tile ----------------------------------------------------------------
@pytest.mark.parametrize("z", [1, 2, 3, 4095, 4096, 4097, 2 * 4096 + 1])
def test_record_counts(native, z):
    records, literals = model.random_records(random.Random(z), z, first_start=(z % 3) * 1000)
    check(native, records, literals)


def test_copies_only_and_literals_only(native):
    b = model.Builder(5000)
    for j in range(4097):
        b.copy_step(3, e=j % 5 - 2) if j else b.copy(100, 3)
    check(native, b.records(), b.literals)
    b = model.Builder(7)
    for j in range(4097):
        b.literal(bytes([b"ACGT"[j * 5 % 4]]))
    s = check(native, b.records(), b.literals)
    assert s["data"] == b"" and s["control"] == bytes(2049)


def test_no_records_launch_nothing(native):
    empty = np.zeros(0, dtype=model.FACTOR_DTYPE)
    native.profile_enable(True)
    try:
        native.profile_reset()
        s = check(native, empty, b"")
        assert s["control"] == s["data"] == s["literals"] == b"" and s["literal_mode"] == 1 and s["z"] == 0
        assert native.factorize_packed(b"") == s
        assert native.decode_packed_array(s)[0].size == 0
        report = native.profile_report()
    finally:
        native.profile_enable(False)
        native.profile_reset()
    # z == 0 launches no kernel: no stage was timed (every device path of these calls opens a profiler scope)
    assert not list(report), report


# ---- literals --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("count", [0, 1, 3, 4, 5, 300])
def test_literal_counts(native, count):
    b = model.Builder(100)
    b.copy(10, 30)
    for j in range(count):
        b.literal(bytes([b"ACGT"[(j * 7 + j // 4) % 4]]))
    b.copy_step(20)
    s = check(native, b.records(), b.literals)
    assert s["literal_mode"] == 1 and len(s["literals"]) == (count + 3) // 4 and model.nibbles(s)[-1] == 1


def test_one_n_among_the_literals(native):
    b = model.Builder(100)
    b.copy(10, 30).literal(b"A").literal(b"N").literal(b"T").copy_step(20).literal(b"C")
    s = check(native, b.records(), b.literals)
    assert s["literal_mode"] == 0 and s["literals"] == b"ANTC"


def test_tuples_are_taken_as_decode_takes_them(native):
    rows = [(0, 1, 0), (1, 1, 1), (2, 2, 0), (4, 3, RC | 1)]
    four = [(0, 1, 0, False), (1, 1, 1, False), (2, 2, 0, False), (4, 3, 1, True)]
    want = model.pack(np.array(rows, dtype=model.FACTOR_DTYPE), b"AC")
    assert native.pack_factors(rows, b"AC") == want == native.pack_factors(four, b"AC")
    assert native.decode_packed_array(want)[0].tobytes() == b"ACACGTG"
