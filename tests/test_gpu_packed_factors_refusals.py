"""What the compact container of factor records refuses on the device.  Each rule of nolzss_factors_unpack is planted
in sections the sequential model made (tests/packed_factors_model.py) and must be refused with the record and the rule
the model names; each refusal of nolzss_factors_pack likewise; nolzss_decode_packed refuses sections without literals
and a prefix of the wrong length."""
import re

import numpy as np
import pytest

import packed_factors_model as model

pytestmark = pytest.mark.gpu

RC = model.RC_MASK


@pytest.fixture(scope="module")
def native():
    from nolzss_amd import _noLZSS
    assert _noLZSS.device_count() >= 1, "no MI355X visible"
    return _noLZSS


def refused(native, s, index, rule):
    """the model and the device name the same record and rule; nothing comes back"""
    with pytest.raises(model.FormatError) as m:
        model.unpack(s)
    assert (m.value.index, m.value.rule) == (index, rule)
    pattern = rf"record {index}( \(behind the last\))? breaks {re.escape(rule)}"
    with pytest.raises(ValueError, match=pattern):
        native.unpack_factors(s)
    if s["literal_mode"] != 2 and s["first_start"] <= 100_000:  # decode_packed expands the same way
        with pytest.raises(ValueError, match=pattern):
            native.decode_packed_array(s, prefix=b"A" * s["first_start"])


def base(first_start=1000, z=120):
    """copy, literal, copy that goes on, ...: record 3 j a copy with L in 2 bytes, 3 j + 1 a literal, 3 j + 2 a copy"""
    b = model.Builder(first_start)
    for j in range(z // 3):
        b.copy(j, 300).literal(b"GN"[j % 2:j % 2 + 1]).copy_step(7)
    s = model.pack(b.records(), b.literals)
    assert s["literal_mode"] == 0
    return s


# ---- nolzss_factors_unpack -------------------------------------------------------------------------------------------
def test_spare_nibble(native):
    b = model.Builder(1000)
    b.copy(0, 300).literal(b"G").copy_step(7)
    s = model.pack(b.records(), b.literals)
    refused(native, model.with_bytes(s, "control", 1, bytes([s["control"][1] | 0x10])), 3, "spare nibble")


def test_literal_nibble(native):
    s = base()
    bad = model.with_bytes(s, "control", 9, bytes([s["control"][9] | 4 << 4]))          # record 19: b = 1
    bad = model.with_bytes(bad, "control", 30, bytes([bad["control"][30] | 12 << 4]))   # record 61: b = 3
    refused(native, bad, 19, "literal nibble")


@pytest.mark.parametrize("delta", [-1, 1])
def test_data_size(native, delta):
    s = base()
    data = s["data"][:-1] if delta < 0 else s["data"] + b"\0"
    refused(native, dict(s, data=data), s["z"], "data size")


def test_length_zero(native):
    s = base()
    off = model.data_offsets(s)
    refused(native, model.with_bytes(s, "data", off[63], b"\0\0"), 63, "length")        # two length bytes
    refused(native, model.with_bytes(s, "data", off[65], b"\0"), 65, "length")          # one


def test_the_smallest_of_two_offending_records_is_named(native):
    b = model.Builder(100_000)
    b.copy(5, 9)
    for j in range(5999):
        b.copy_step(3, e=(j % 3) - 1)
    s = model.pack(b.records(), b.literals)
    off = model.data_offsets(s)
    bad = model.with_bytes(model.with_bytes(s, "data", off[5000], b"\0"), "data", off[70], b"\0")
    refused(native, bad, 70, "length")


def test_diagonal_code_beyond_33_bits(native):
    b = model.edge_builder()
    s = model.pack(b.records(), b.literals)
    off, nib = model.data_offsets(s), model.nibbles(s)
    i = max(j for j in range(s["z"]) if nib[j] >> 2 == 3)
    at = off[i] + model.LENGTH_BYTES[nib[i] & 3] + 4
    assert s["data"][at] == 1                                                         # v = 2^33 - 2: bit 32
    refused(native, model.with_bytes(s, "data", at, b"\x02"), i, "diagonal code")        # bit 33
    refused(native, model.with_bytes(s, "data", at, b"\x81"), i, "diagonal code")        # bit 39


def test_source_range(native):
    # forward: a source that ends where its factor starts; one more symbol and it does not
    b = model.Builder(1000)
    b.copy(10, 20).copy(1020 - 50, 50).literal(b"A").copy(0, 9)
    s = model.pack(b.records(), b.literals)
    off = model.data_offsets(s)
    assert s["data"][off[1]] == 50
    refused(native, dict(model.with_bytes(s, "data", off[1], bytes([51])), decoded=s["decoded"] + 1), 1, "source range")
    # reverse complement: the mirrored coordinate is fixed by the stream, so a smaller first_start leaves the source behind
    b = model.Builder(50)
    b.copy(10, 40, rc=True).literal(b"T").copy_step(2)
    s = model.pack(b.records(), b.literals)
    refused(native, dict(s, first_start=49), 0, "source range")
    # a code that toggles the strand on a short text: the mirrored source lies far beyond p
    b = model.Builder(1000)
    b.copy(10, 20).copy_step(5, e=3)
    s = model.pack(b.records(), b.literals)
    off = model.data_offsets(s)
    assert model.nibbles(s)[1] == (1 | 1 << 2)
    bad = dict(model.with_bytes(s, "data", off[1] + 1, (0xFFFF).to_bytes(2, "little")))  # e = -2^14 and a toggle
    refused(native, bad, 1, "source range")


def test_literal_count_off_by_one(native):
    s = base()
    assert s["n_literals"] == 40
    refused(native, dict(s, n_literals=39, literals=s["literals"][:-1]), 118, "literal count")  # literal number 40
    refused(native, dict(s, n_literals=41, literals=s["literals"] + b"G"), 120, "literal count")  # behind the last
    with pytest.raises(ValueError, match=r"record 120 \(behind the last\) breaks literal count"):
        native.unpack_factors(dict(s, n_literals=41, literals=s["literals"] + b"G"))


def test_decoded_length(native):
    s = base()
    refused(native, dict(s, decoded=s["decoded"] + 1), 120, "decoded length")
    refused(native, dict(s, decoded=s["decoded"] - 1), 120, "decoded length")


def test_what_the_host_refuses_before_the_device(native):
    s = base()
    for changes, word in [({"literals": s["literals"] + b"\0"}, "literal section"),
                          ({"literals": s["literals"][:-1]}, "literal section"),
                          ({"control": s["control"][:-1]}, "control section"),
                          ({"first_start": model.MAX_TEXT - s["decoded"] + 1}, "text too long"),
                          ({"literal_mode": 3}, "literal_mode")]:
        bad = dict(s, **changes)
        with pytest.raises(ValueError):
            model.unpack(bad)
        with pytest.raises(ValueError, match=word):
            native.unpack_factors(bad)
    top = dict(s, first_start=model.MAX_TEXT - s["decoded"])  # the last position the pipeline takes: still valid
    records, literals = native.unpack_factors(top)
    assert np.array_equal(records, model.unpack(top)[0]) and int(records["start"][0]) == top["first_start"]


# ---- nolzss_factors_pack ---------------------------------------------------------------------------------------------
OK = [(0, 1, 0), (1, 1, 1), (2, 2, 0)]


@pytest.mark.parametrize("rows, lit, index, rule", [
    ([(0, 1, 0), (2, 1, 2)], b"AC", 1, "tiling"),                                    # a gap
    ([(0, 1, 0), (1, 1, 1), (1, 2, 0)], b"AC", 2, "tiling"),                         # an overlap
    ([(0, 1, 0), (1, 0, 0), (1, 1, 1)], b"AC", 1, "tiling"),                         # length 0
    ([(0, 2, 0)], b"A", 0, "literal length"),
    ([(5, 1, 5), (6, 3, 6)], b"AC", 1, "literal length"),
    (OK[:2] + [(2, 2, 1)], b"AC", 2, "source range"),                                # ends one behind its start
    (OK[:2] + [(2, 2, RC | 1)], b"AC", 2, "source range"),
    (OK[:2] + [(2, 2, 7)], b"AC", 2, "source range"),                                # starts behind it
    (OK, b"A", 1, "literal count"),
    (OK, b"ACG", 3, "literal count"),
    ([(model.MAX_TEXT - 2, 1, model.MAX_TEXT - 2), (model.MAX_TEXT - 1, 2, 0), (5, 1, 5)], b"AC", 1, "tiling"),  # beyond the pipeline
])
def test_pack_refusals(native, rows, lit, index, rule):
    records = np.array(rows, dtype=model.FACTOR_DTYPE)
    with pytest.raises(model.FormatError) as m:
        model.pack(records, lit)
    assert (m.value.index, m.value.rule) == (index, rule)
    with pytest.raises(ValueError) as e:
        native.pack_factors(records, lit)
    assert re.search(rf"record {index}( \(behind the last\))? breaks {rule}", str(e.value)), str(e.value)


def test_pack_names_the_first_of_many_bad_records(native):
    b = model.Builder(100_000)
    b.copy(5, 9)
    for j in range(8999):
        b.copy_step(3, e=(j % 3) - 1)
    records = b.records()
    for k in (7000, 4500, 8999):
        records["length"][k] += 1                                                    # the record behind it does not tile
    with pytest.raises(model.FormatError) as m:
        model.pack(records, b"")
    assert (m.value.index, m.value.rule) == (4501, "tiling")
    with pytest.raises(ValueError, match=r"record 4501 breaks tiling"):
        native.pack_factors(records, b"")


def test_pack_refuses_an_end_beyond_the_pipeline(native):
    with pytest.raises(ValueError, match="text too long"):
        native.pack_factors([(model.MAX_TEXT, 1, model.MAX_TEXT)], b"A")
    with pytest.raises(ValueError, match="text too long"):
        native.pack_factors([(0, 1, 0), (1, (1 << 64) - 1, 0)], b"A")


# ---- nolzss_decode_packed --------------------------------------------------------------------------------------------
def test_decode_packed_refusals(native):
    b = model.Builder(4)
    b.literal(b"G").copy(0, 5).copy(1, 3, rc=True)
    s = model.pack(b.records(), b.literals)
    assert native.decode_packed_array(s, prefix=b"ACGT")[0].tobytes() == b"ACGTGACGTGACG"
    with pytest.raises(ValueError, match="literal_mode 2"):
        native.decode_packed_array(model.pack(b.records()), prefix=b"ACGT")
    for prefix in (b"", b"ACG", b"ACGTA"):
        with pytest.raises(ValueError, match="first_start is 4"):
            native.decode_packed_array(s, prefix=prefix)
    with pytest.raises(ValueError, match="complement of a non-nucleotide"):
        native.decode_packed_array(s, prefix=b"ACNT")                                   # rc(CNT) has no complement
