"""nolzss_rlz_archive_open_packed on broken sections: a valid packed archive made by the sequential model
(tests/rlz_archive_pack_model.py), one thing corrupted at a time.  Every call returns the error status, names the
smallest offending record (or separator) and the rule -- the model's verdict on the same sections, and the index written
out here --, leaves no handle, and is followed in the same process by a successful open and extract of the valid archive.
The kernels bound every read by the sizes of the sections (rlz_archive_pack.hip), so none of these may fault."""
import ctypes as C
import re

import numpy as np
import pytest

import rlz_archive_pack_model as model

pytestmark = pytest.mark.gpu

RC = model.RC_MASK


@pytest.fixture(scope="module")
def native():
    from nolzss_amd import _noLZSS
    assert _noLZSS.device_count() >= 1, "no MI355X visible"
    return _noLZSS


def _dna(n, seed):
    rng = np.random.default_rng(seed)
    return np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, n)].tobytes()


def _valid():
    """11 records (odd), three targets, three literals, both strands, a block with three separators"""
    block = bytearray(_dna(1_003, 41))
    for p in (200, 201, 900):
        block[p] = 1
    b = model.Builder(bytes(block))
    b.copy(0, 100).literal(b"G").copy_step(50)            # records 0 .. 2: target 0 = 151 bytes
    b.copy(300, 64, rc=True).literal(b"T").copy_step(40)  # 3 .. 5
    b.copy(400, 300).copy_step(100)                       # 6, 7: target 1 ends behind record 7
    b.literal(b"A").copy(950, 53).copy(250, 20, rc=True)  # 8 .. 10: the forward copy ends at the end of the block
    lengths = [151, 505, 74]
    assert b.p == sum(lengths) and len(b.rows) == 11
    return bytes(block), b.records(), bytes(b.literals), lengths


BLOCK, RECORDS, LITERALS, LENGTHS = _valid()
VALID = model.pack(BLOCK, RECORDS, LITERALS, LENGTHS)
B, Z = len(BLOCK), len(RECORDS)


def _open_raw(native, sections, lengths):
    """the C call itself -> (status, handle value, message): a refusal must leave the handle NULL"""
    from nolzss_amd import _lib
    p = _lib.RlzArchivePacked()
    keep = []
    for name in native.PACKED_COUNTS:
        setattr(p, name, int(sections[name]))
    for name, size in native.PACKED_SECTIONS:
        raw = bytes(sections[name])
        buf = C.create_string_buffer(raw, len(raw)) if raw else None
        keep.append(buf)
        setattr(p, name, C.cast(buf, C.c_void_p) if buf is not None else None)
        setattr(p, size, len(raw))
    lens = np.ascontiguousarray(lengths, dtype=np.uint64)
    h = C.c_void_p(0xdead)
    rc = _lib.lib.nolzss_rlz_archive_open_packed(C.byref(p), lens.ctypes.data if lens.size else None, lens.size, 0, C.byref(h))
    return rc, h.value, _lib.lib.nolzss_last_error().decode()


def _still_works(native):
    with native.RlzArchiveHandle.open_packed(VALID, LENGTHS) as h:
        data, offsets = h.extract_array([(0, 0, LENGTHS[0]), (2, 0, LENGTHS[2]), (1, 100, 505)])
        with native.RlzArchiveHandle.open_records(BLOCK, RECORDS, LITERALS, LENGTHS) as ref:
            want, want_offsets = ref.extract_array([(0, 0, LENGTHS[0]), (2, 0, LENGTHS[2]), (1, 100, 505)])
        assert np.array_equal(data, want) and np.array_equal(offsets, want_offsets)
        assert np.array_equal(h.export()[1], RECORDS)


def _set_nibble(control, i, value):
    c = bytearray(control)
    c[i >> 1] = (c[i >> 1] & (0xF0 if i & 1 == 0 else 0x0F)) | (value << (4 * (i & 1)))
    return bytes(c)


def _data_offset(i):
    """where the data bytes of record i begin in the valid archive"""
    nib = [(VALID["control"][j >> 1] >> (4 * (j & 1))) & 15 for j in range(i)]
    return sum((0, 1, 2, 4)[n & 3] + (0, 1, 3, 5)[n >> 2] for n in nib)


def _repacked(records):
    """sections of records the model codes without judging them (the decoded length follows the records)"""
    control, data, _ = model.code_records(B, records)
    return {**VALID, "control": control, "data": data, "decoded": int(records[-1]["start"] + records[-1]["length"]) - B}


def _cases():
    out = {}
    out["data one byte short"] = ({"data": VALID["data"][:-1]}, LENGTHS, "record", Z, "data size")
    out["data one byte long"] = ({"data": VALID["data"] + b"\0"}, LENGTHS, "record", Z, "data size")
    out["literal nibble with b = 1"] = ({"control": _set_nibble(VALID["control"], 4, 1 << 2)}, LENGTHS, "record", 4,
                                        "literal nibble")
    out["literal nibble with b = 3, record 1"] = ({"control": _set_nibble(VALID["control"], 1, 3 << 2)}, LENGTHS, "record", 1,
                                                  "literal nibble")
    out["spare nibble"] = ({"control": VALID["control"][:-1] + bytes([VALID["control"][-1] | 0x50])}, LENGTHS, "record", Z,
                           "spare nibble")
    data = bytearray(VALID["data"])
    data[_data_offset(5)] = 0
    out["a copy with L = 0"] = ({"data": bytes(data)}, LENGTHS, "record", 5, "length")
    # x + L = B + 1: record 9 is the forward copy that ends at the end of the block, record 10 a reverse one
    fwd = RECORDS.copy()
    fwd[9]["ref"] += 1
    out["x + L = B + 1, forward"] = (_repacked(fwd), LENGTHS, "record", 9, "source inside the block")
    rev = RECORDS.copy()
    rev[10]["ref"] = RC | (B + 1 - 20)  # y = 2 B + 1 - x - L = B: one below the reverse strand's range
    out["x + L = B + 1, reverse"] = (_repacked(rev), LENGTHS, "record", 10, "source inside the block")
    out["a record straddles a target end"] = ({}, [150, 506, 74], "record", 2, "target boundary")
    out["a record behind the last target"] = ({"decoded": VALID["decoded"]}, [151, 505, 73], "record", 10, "target boundary")
    longer = RECORDS.copy()
    longer[10]["length"] += 1
    longer[10]["ref"] = RC | 249
    out["lengths sum to one more than the targets"] = (_repacked(longer), LENGTHS, "record", 10, "target boundary")
    out["targets sum to one more than the lengths"] = ({}, [151, 505, 75], "record", Z, "target boundary")
    out["literal section one symbol short"] = ({"n_literals": 2, "literals": model.pack_2bit(LITERALS[:2])}, LENGTHS,
                                               "record", 8, "literal count")
    out["literal count one too many"] = ({"n_literals": 4, "literals": model.pack_2bit(LITERALS + b"C")}, LENGTHS,
                                         "record", Z, "literal count")
    q = (B + 3) // 4
    seps = np.array([200, 201, 900], dtype="<u4")
    out["unsorted separator list"] = ({"block": VALID["block"][:q] + seps[[0, 2, 1]].tobytes()}, LENGTHS, "separator", 2,
                                      "separator list")
    out["a separator twice"] = ({"block": VALID["block"][:q] + np.array([200, 200, 900], dtype="<u4").tobytes()}, LENGTHS,
                                "separator", 1, "separator list")
    out["a separator at B"] = ({"block": VALID["block"][:q] + np.array([200, 201, B], dtype="<u4").tobytes()}, LENGTHS,
                               "separator", 2, "separator list")
    # the codes no small block can hold, decoded: the largest, v = 2^33 - 1 (e = -2^31, strand toggled), leaves the block;
    # a v of more than 33 bits is no code
    at = _data_offset(6)
    assert (VALID["control"][3] & 15) == (2 | 2 << 2)  # record 6: L in two bytes, v in three
    for name, code, rule in (("the largest v", (1 << 33) - 1, "source inside the block"),
                             ("a v of 34 bits", 1 << 33, "diagonal code")):
        data = VALID["data"][:at + 2] + code.to_bytes(5, "little") + VALID["data"][at + 5:]
        out[name] = ({"control": _set_nibble(VALID["control"], 6, 2 | 3 << 2), "data": data}, LENGTHS, "record", 6, rule)
    return out


CASES = _cases()


def test_the_valid_archive_opens(native):
    assert model.unpack(VALID, LENGTHS)[2] == LITERALS and VALID["num_separators"] == 3 and Z % 2 == 1
    _still_works(native)


@pytest.mark.parametrize("name", list(CASES))
def test_refusal(native, name):
    from nolzss_amd import _lib
    change, lengths, what, index, rule = CASES[name]
    sections = {**VALID, **change}
    with pytest.raises(model.FormatError) as verdict:  # the model's verdict on the same sections
        model.unpack(sections, lengths)
    assert (verdict.value.index, verdict.value.rule) == (index, rule)
    status, handle, message = _open_raw(native, sections, lengths)
    assert status == _lib.ERR_INVALID_ARGUMENT and handle is None, (status, handle, message)
    assert re.search(rf"rlz archive: {what} {index} (\(behind the last\) )?breaks {re.escape(rule)}", message), message
    with pytest.raises(ValueError):
        native.RlzArchiveHandle.open_packed(sections, lengths)
    _still_works(native)


def test_section_sizes_are_checked_on_the_host(native):
    for change in ({"control": VALID["control"][:-1]}, {"control": VALID["control"] + b"\0"},
                   {"literals": VALID["literals"] + b"\0"}, {"block": VALID["block"][:-1]}, {"num_separators": 4},
                   {"block_mode": 0}, {"block_mode": 2}, {"literal_mode": 0}, {"z": Z + 2}, {"block_length": B + 4},
                   {"block_length": 1 << 40}, {"decoded": 1 << 40}, {"z": 1 << 33}):
        with pytest.raises(ValueError):
            native.RlzArchiveHandle.open_packed({**VALID, **change}, LENGTHS)
    _still_works(native)
