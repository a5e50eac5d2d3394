"""The compact container on the device against the sequential model (tests/rlz_archive_pack_model.py), section by
section and byte for byte: archives opened with nolzss_rlz_archive_open_records from hand-made records are packed with
nolzss_rlz_archive_pack, the sections opened again with nolzss_rlz_archive_open_packed, and export, info, pack and
extract of that handle compared with the input and with the handle it came from (rlz_archive_pack.hip,
rlz_archive_pack_api.hip).

A step of the diagonal whose true value wraps mod 2^32 cannot be planted on a small block: |e| is below about 3 B.  The
cases below cover both signs and every edge of the byte classes of v instead (0, 255 | 256, 2^24 - 1 | 2^24, which need a
block of 2^22 bases and more), and the largest v the block admits; the codes beyond, up to v = 2^33 - 1, are decoded in
tests/test_gpu_rlz_archive_pack_refusals.py, where they must leave the block, and coded and decoded by the model alone
in tests/test_rlz_archive_pack_host.py."""
import random

import numpy as np
import pytest

import rlz_archive_pack_model as model

pytestmark = pytest.mark.gpu

RC = model.RC_MASK
INFO_KEYS = ("num_targets", "block_length", "z", "n_literals", "total_length", "device_bytes")


@pytest.fixture(scope="module")
def native():
    from nolzss_amd import _noLZSS
    assert _noLZSS.device_count() >= 1, "no MI355X visible"
    return _noLZSS


def _dna(n, seed, alphabet=b"ACGT"):
    rng = np.random.default_rng(seed)
    return np.frombuffer(alphabet, dtype=np.uint8)[rng.integers(0, len(alphabet), n)].tobytes()


BLOCK = _dna(70_001, 11)                     # odd, no multiple of 4: the last packed byte holds one base
BIG = _dna((1 << 22) + 300_001, 12)          # steps of 2^22 on one strand: the 5-byte class of v


def _ranges(rng, lengths, count, longest=3000):
    out = []
    live = [j for j, n in enumerate(lengths) if n]
    for _ in range(count if live else 0):
        j = rng.choice(live)
        lo = rng.randrange(0, lengths[j])
        out.append((j, lo, min(lengths[j], lo + rng.choice((0, 1, 15, 16, 17, 300, longest)))))
    return out + [(j, 0, min(n, 40_000)) for j, n in enumerate(lengths)]


def check(native, block, records, literals, lengths, seed=1, ranges=300):
    """pack == the model; open_packed gives back the archive: export, info, pack again, and the bytes of random ranges"""
    want = model.pack(block, records, literals, lengths)
    back = model.unpack(want, lengths)
    assert back[0] == bytes(block) and np.array_equal(back[1], records) and back[2] == bytes(literals)
    with native.RlzArchiveHandle.open_records(block, records, literals, lengths) as h:
        got = h.pack()
        for key in want:
            assert got[key] == want[key], key
        assert set(got) == set(want)
        with native.RlzArchiveHandle.open_packed(got, lengths) as h2:
            b2, r2, l2 = h2.export()
            assert b2 == bytes(block) and np.array_equal(r2, records) and l2 == bytes(literals)
            assert {k: h2.info[k] for k in INFO_KEYS} == {k: h.info[k] for k in INFO_KEYS}
            assert h2.target_lengths.tolist() == [int(x) for x in lengths]
            assert h2.pack() == want
            rows = _ranges(random.Random(seed), [int(x) for x in lengths], ranges)
            if rows:
                d1, o1 = h.extract_array(rows)
                d2, o2 = h2.extract_array(rows)
                assert np.array_equal(o1, o2) and np.array_equal(d1, d2)
    return want


def _nibbles(sections):
    c = sections["control"]
    return [(c[i >> 1] >> (4 * (i & 1))) & 15 for i in range(sections["z"])]


# ---- lengths ---------------------------------------------------------------------------------------------------------
def test_length_classes_and_a_copy_of_most_of_the_block(native):
    b = model.Builder(BLOCK)
    for L in (1, 255, 256, 65_535, 65_536):
        b.copy(3, L).copy(len(BLOCK) - L, L, rc=True).copy_step(1)
    b.copy(1, len(BLOCK) - 1)                  # most of the block
    b.copy(0, len(BLOCK), rc=True)             # all of it, the other way round
    s = check(native, BLOCK, b.records(), b.literals, [b.p])
    assert [n & 3 for n in _nibbles(s)] == [1, 1, 1, 1, 1, 1, 2, 2, 1, 2, 2, 1, 3, 3, 1, 3, 3]


# ---- the classes of v, both signs -----------------------------------------------------------------------------------
def test_code_classes_on_a_block_beyond_2_pow_22(native):
    B = len(BIG)
    b = model.Builder(BIG)
    b.copy(0, 9)                               # v = 0: the first copy lies on the diagonal 0
    b.copy_step(20, e=64)                      # v = 256
    b.copy_step(20, e=-64)                     # v = 254
    b.copy_step(20, e=1 << 22)                 # v = 2^24
    b.copy_step(20, e=-(1 << 22))              # v = 2^24 - 2 (three bytes, negative)
    b.copy_step(20, e=(1 << 22) - 1)           # v = 2^24 - 4 (three bytes)
    b.copy_step(20, e=-(1 << 22) - 1)          # v = 2^24 + 2 (five bytes, negative)
    b.copy(B - 10, 10, rc=True)                # reverse strand at its lowest y = B + 1
    b.copy_step(30, e=-64, toggle=True)        # back to forward, 64 below: v = 255
    b.copy(B - 10, 10, rc=True)
    b.literal(b"G")
    b.copy_step(5, e=300_000 - (1 << 22) - 11, toggle=True)  # reverse to forward behind a literal, three bytes
    b.copy(B - 10, 10, rc=True)
    b.copy_step(7, e=-(1 << 22), toggle=True)  # v = 2^24 - 1
    b.copy(0, 1)                               # the lowest forward y ...
    b.copy(0, 1, rc=True)                      # ... to the highest reverse one, y = 2 B: the largest v this block admits
    codes = [c for c in b.codes if c is not None]
    assert codes[:7] == [0, 256, 254, 1 << 24, (1 << 24) - 2, (1 << 24) - 4, (1 << 24) + 2]
    assert codes[8] == 255 and codes[12] == (1 << 24) - 1 and codes[-1] == ((2 * (2 * B - 1)) << 1) | 1
    s = check(native, BIG, b.records(), b.literals, [b.p], ranges=100)
    assert {n >> 2 for n in _nibbles(s)} == {0, 1, 2, 3}


def test_code_class_edges_small(native):
    b = model.Builder(BLOCK)
    b.copy(1000, 10)
    for e in (0, 1, -1, 63, -64, 64, -65, 127, -128, 128, 30_000, -30_000):  # v = 0, 4, 2, 252, 254, 256, 258, ...
        b.copy_step(10, e=e)
    s = check(native, BLOCK, b.records(), b.literals, [b.p])
    assert [n >> 2 for n in _nibbles(s)] == [2, 0, 1, 1, 1, 1, 2, 2, 2, 2, 2, 2, 2]


# ---- diagonals and strands ------------------------------------------------------------------------------------------
def test_chains_on_both_strands_behind_literals(native):
    b = model.Builder(BLOCK)
    b.copy(40_000, 100, rc=True)               # the first record is a reverse-complement copy
    b.literal(b"A").literal(b"C")
    b.copy_step(50)                            # the chain goes on behind two literals: v = 0, x falls
    b.literal(b"T")
    b.copy_step(256)
    b.copy(500, 80)                            # strand toggled
    b.literal(b"G")
    b.copy_step(300)                           # kept, colinear: v = 0
    b.copy_step(30, e=-7)                      # kept, a deletion
    b.copy_step(30, e=9)                       # kept, an insertion
    b.copy_step(30, e=0, toggle=False)
    b.copy(len(BLOCK) - 60, 60)                # forward, ends at the end of the block
    b.literal(b"A")
    b.copy_step(12, e=0, toggle=True)          # toggled ON the diagonal: y = B + 1, v = 1
    assert b.rows[3] == (len(BLOCK) + 102, 50, RC | (40_000 - 2 - 50)) and b.codes[3] == 0 and b.codes[5] == 0
    assert b.codes[8] == 0 and b.codes[11] == 0 and b.codes[-1] == 1 and b.codes[6] & 1
    lengths = [152, 0, b.p - 152]
    s = check(native, BLOCK, b.records(), b.literals, lengths)
    assert _nibbles(s)[3] == 1 and _nibbles(s)[5] == 2 and _nibbles(s)[8] == 2


def test_first_record_a_literal(native):
    b = model.Builder(BLOCK)
    b.literal(b"T").copy(5, 40).literal(b"G").copy_step(3)
    check(native, BLOCK, b.records(), b.literals, [1, b.p - 1])


# ---- record counts: the scan tile -----------------------------------------------------------------------------------
@pytest.mark.parametrize("z", [1, 2, 3, 4095, 4096, 4097, 2 * 4096 + 1])
def test_record_counts(native, z):
    records, literals, lengths = model.random_archive(random.Random(z), BLOCK, z)
    if z > 1000:  # empty targets at the front, in the middle and at the end
        m = len(lengths) // 2
        lengths = [0, 0] + lengths[:m] + [0] + lengths[m:] + [0, 0]
    check(native, BLOCK, records, literals, lengths, seed=z)


def test_a_target_boundary_on_every_10th_record(native):
    records, literals, lengths = model.random_archive(random.Random(77), BLOCK, 1234, boundary=10)
    assert len(lengths) == 124
    check(native, BLOCK, records, literals, lengths)


def test_no_records_and_no_targets(native):
    empty = np.zeros(0, dtype=model.FACTOR_DTYPE)
    native.profile_enable(True)
    try:
        native.profile_reset()
        for block in (b"", b"ACGT", b"AC\x01GT", b"ACgT"):
            for lengths in ([], [0, 0, 0]):
                s = check(native, block, empty, b"", lengths)
                assert s["control"] == s["data"] == s["literals"] == b"" and s["literal_mode"] == 1
        report = native.profile_report()
    finally:
        native.profile_enable(False)
        native.profile_reset()
    # z == 0 launches no kernel: no stage of the pack, the unpack or the extract was timed (the empty report is the only
    # observable of it; every device path of these calls opens a profiler scope)
    assert not [name for name in report if name.startswith(("rlz_", "packed_"))], report


# ---- literals -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("count", [0, 1, 3, 4, 5, 300])
def test_literal_counts(native, count):
    b = model.Builder(BLOCK)
    b.copy(10, 30)
    for j in range(count):
        b.literal(bytes([b"ACGT"[(j * 7 + j // 4) % 4]]))
    b.copy_step(20)
    s = check(native, BLOCK, b.records(), b.literals, [b.p])
    assert s["literal_mode"] == 1 and len(s["literals"]) == (count + 3) // 4 and _nibbles(s)[-1] == 1


def test_one_n_among_the_literals(native):
    b = model.Builder(BLOCK)
    b.copy(10, 30).literal(b"A").literal(b"N").literal(b"T").copy_step(20).literal(b"C")
    s = check(native, BLOCK, b.records(), b.literals, [b.p])
    assert s["literal_mode"] == 0 and s["literals"] == b"ANTC"


# ---- blocks ---------------------------------------------------------------------------------------------------------
def test_block_with_two_separators(native):
    block = bytearray(_dna(9_999, 21))
    block[3_000] = block[7_001] = 1
    records, literals, lengths = model.random_archive(random.Random(5), bytes(block), 400, with_rc=False)
    s = check(native, bytes(block), records, literals, lengths)
    assert s["block_mode"] == 1 and s["num_separators"] == 2
    assert s["block"][2_500:] == np.array([3_000, 7_001], dtype="<u4").tobytes()


def test_block_with_a_lower_case_byte(native):
    block = bytearray(_dna(9_999, 22))
    block[5_000] = ord("a")
    block[100] = 1
    records, literals, lengths = model.random_archive(random.Random(6), bytes(block), 400, with_rc=False)
    s = check(native, bytes(block), records, literals, lengths)
    assert s["block_mode"] == 0 and s["num_separators"] == 0 and s["block"] == bytes(block)
