"""CPU tests of the compact relative-LZ archive container (no GPU): the sequential model of the format
(tests/rlz_archive_pack_model.py) round-trips fuzzed and hand-made archives, the codes of the zigzag, strand-toggle and
wrap-around cases are what the format says, the host-only file writer and reader of nolzss_amd.genomics.rlz agree with
the model byte for byte and refuse every broken container, load() dispatches on the magic, and save() without compact=
writes what it wrote before."""
import random
import struct
import zipfile

import numpy as np
import pytest

import rlz_archive_pack_model as model
from nolzss_amd import _lib, _noLZSS as native
from nolzss_amd.genomics import rlz

RC = model.RC_MASK
M32 = model.M32


def _dna(n, seed, alphabet=b"ACGT"):
    rng = np.random.default_rng(seed)
    return np.frombuffer(alphabet, dtype=np.uint8)[rng.integers(0, len(alphabet), n)].tobytes()


def _nibbles(sections):
    c = sections["control"]
    return [(c[i >> 1] >> (4 * (i & 1))) & 15 for i in range(sections["z"])]


def _round_trip(block, records, literals, lengths):
    s = model.pack(block, records, literals, lengths)
    b2, r2, l2 = model.unpack(s, lengths)
    assert b2 == bytes(block) and l2 == bytes(literals) and np.array_equal(r2, records)
    return s


# ---- the model against itself ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(6))
def test_unpack_inverts_pack_on_fuzzed_archives(seed):
    rng = random.Random(seed)
    block = _dna(rng.choice((1, 7, 300, 5000)), seed, b"ACGT" if seed % 3 else b"ACGT\x01")
    for z in (0, 1, 2, 3, 64, 501):
        records, literals, lengths = model.random_archive(rng, block, z, alphabet=b"ACGT" if seed % 2 else b"ACGTN",
                                                           with_rc=seed != 4)
        s = _round_trip(block, records, literals, lengths)
        assert s["z"] == z and s["n_literals"] == len(literals) and s["decoded"] == sum(lengths)
        assert len(s["control"]) == (z + 1) // 2 and (z % 2 == 0 or s["control"][-1] >> 4 == 0)
        assert s["literal_mode"] == (0 if b"N" in literals else 1)


def test_every_nibble_class():
    # a block long enough for a 4-byte length and for a 5-byte code: same-strand steps of 2^22 need B > 2^22
    B = (1 << 22) + 300_000
    block = _dna(B, 3)
    b = model.Builder(block)
    b.literal(b"C")                                     # 0
    b.copy(10, 200)                                     # a = 1, b = 1: the first copy, v = zigzag(10 - 1) << 1
    b.copy_step(255)                                    # a = 1, b = 0
    b.copy_step(256, e=5)                               # a = 2, b = 1
    b.copy_step(65_535, e=-200)                         # a = 2, b = 2
    b.copy_step(65_536, e=(1 << 22))                    # a = 3, b = 3: v = 2^24
    b.copy_step(1)                                      # a = 1, b = 0
    b.copy_step(70_000, e=-(1 << 22) + 3)               # a = 3, b = 2: v = 2^24 - 14
    b.copy_step(66_000, e=30)                           # a = 3, b = 1
    b.copy_step(300, e=1 << 22)                         # a = 2, b = 3
    b.copy_step(9, e=-(1 << 22) - 1)                    # a = 1, b = 3: v = 2^24 + 2
    b.copy(1000, 50, rc=True)                           # the strand toggles, far away: b = 3
    b.copy_step(300)                                    # a = 2, b = 0 on the reverse strand (x falls by 300)
    b.copy(5000, 10)                                    # back
    b.copy_step(65_536)                                 # a = 3, b = 0
    b.copy_step(2, e=-40)                               # a = 1, b = 1
    b.copy_step(2, e=-400)                              # a = 1, b = 2
    assert b.rows[12][2] == RC | 700 and b.codes[12] == 0 and b.codes[11] & 1 and b.codes[13] & 1
    s = _round_trip(block, b.records(), b.literals, [b.p])
    seen = set(_nibbles(s))
    assert seen == {0} | {a | bb << 2 for a in (1, 2, 3) for bb in (0, 1, 2, 3)}, sorted(seen)
    assert b.codes[5] == 1 << 24 and b.codes[7] == (1 << 24) - 14 and b.codes[10] == (1 << 24) + 2


def test_zigzag_toggle_and_wrap_around_codes():
    assert [model.zigzag32(d & M32) for d in (0, -1, 1, -2, 2, -(1 << 31), (1 << 31) - 1)] == \
        [0, 1, 2, 3, 4, M32, M32 - 1]
    for zz in (0, 1, 2, 3, 255, 256, (1 << 23) - 1, 1 << 23, M32 - 1, M32):
        assert model.zigzag32(model.unzigzag32(zz)) == zz
    # a block that is not laid out: 2 B + 1 is beyond 32 bits, every coordinate wraps
    B = (1 << 32) - (1 << 20)
    b = model.Builder(b"", B=B)
    b.copy(0, 5)                          # forward at 0: g = 0, v = 0
    b.literal().literal()
    b.copy(7, 3)                          # colinear behind two literals: v = 0
    b.copy(B - 4, 4, rc=True)             # y = 2 B + 1 - B = B + 1: wraps; strand toggled
    b.literal()
    b.copy(B - 4 - 1 - 6, 6, rc=True)     # the RC chain goes on behind a literal (x falls as p rises): v = 0
    b.copy(B - 9, 9)                      # back to forward, far away
    b.copy(0, 1)                          # a step of nearly -2^32, which IS a small positive one mod 2^32 ...
    records = b.records()
    assert b.codes[0] == 0 and b.codes[3] == 0 and b.codes[4] & 1 == 1 and b.codes[6] == 0 and b.codes[7] & 1 == 1
    control, data, lits = model.code_records(B, records)
    s = {"block_length": B, "z": len(records), "n_literals": lits, "decoded": b.p, "control": control, "data": data,
         "literals": model.pack_2bit(b.literals), "literal_mode": 1}
    got, symbols = model.decode_records(s, [b.p])
    assert np.array_equal(got, records) and symbols == bytes(b.literals)
    # ... and the largest code, e = -2^31 with the strand toggled: v = 2^33 - 1, five bytes of 0xff but the top seven bits
    b2 = model.Builder(b"", B=B)
    b2.copy((1 << 31) + 17, 2)
    b2.copy_step(3, e=-(1 << 31), toggle=True)
    assert b2.codes[1] == (1 << 33) - 1
    control, data, _ = model.code_records(B, b2.records())
    assert data[-5:] == b"\xff\xff\xff\xff\x01" and control[0] >> 4 == 1 | 3 << 2
    s = {"block_length": B, "z": 2, "n_literals": 0, "decoded": b2.p, "control": control, "data": data, "literals": b"",
         "literal_mode": 1}
    assert np.array_equal(model.decode_records(s, [2, 3])[0], b2.records())


def test_model_refusals_name_the_smallest_record():
    block = _dna(400, 9)
    b = model.Builder(block)
    b.copy(0, 10).literal(b"G").copy_step(20).copy(100, 7, rc=True).literal(b"T").copy_step(5)
    lengths = [31, 13]
    s = model.pack(block, b.records(), b.literals, lengths)
    assert _nibbles(s)[1] == 0 and _nibbles(s)[2] == 1

    def refusal(**change):
        with pytest.raises(model.FormatError) as e:
            model.unpack({**s, **change}, change.pop("lengths", lengths))
        return e.value.index, e.value.rule

    ctl = bytearray(s["control"])
    ctl[0] |= 1 << 6                                    # record 1, a literal, gets b = 1
    assert refusal(control=bytes(ctl)) == (1, "literal nibble")
    assert refusal(data=s["data"][:-1]) == (6, "data size") and refusal(data=s["data"] + b"\0") == (6, "data size")
    data = bytearray(s["data"])
    data[0] = 0
    assert refusal(data=bytes(data)) == (0, "length")
    assert refusal(lengths=[30, 14]) == (2, "target boundary")
    assert refusal(lengths=[31, 12]) == (5, "target boundary")
    assert refusal(n_literals=1, literals=model.pack_2bit(b"G")) == (4, "literal count")
    assert refusal(n_literals=3, literals=model.pack_2bit(b"GTA")) == (6, "literal count")
    odd = model.pack(block, b.records()[:5], b.literals, [31, 8])
    with pytest.raises(model.FormatError) as e:
        model.unpack({**odd, "control": odd["control"][:-1] + bytes([odd["control"][-1] | 0x10])}, [31, 8])
    assert (e.value.index, e.value.rule) == (5, "spare nibble")


# ---- the file ------------------------------------------------------------------------------------------------------------
def _sample(seed=5, z=40, alphabet=b"ACGT"):
    rng = random.Random(seed)
    block = _dna(900, seed, b"ACGT\x01")
    records, literals, lengths = model.random_archive(rng, block, z, alphabet=alphabet)
    return block, records, literals, lengths, model.pack(block, records, literals, lengths)


@pytest.mark.parametrize("ids", [None, "names"])
def test_container_round_trip(tmp_path, ids):
    block, records, literals, lengths, s = _sample()
    names = None if ids is None else [f"sample é {j}" for j in range(len(lengths))]
    path = tmp_path / "a.rlz"
    rlz.write_packed_archive(path, s, lengths, names)
    raw = path.read_bytes()
    assert raw == model.container_bytes(s, lengths, names) and raw[:8] == b"noLZRLZ1" == rlz.PACKED_MAGIC
    assert len(raw) % 8 == 0 and model.HEADER.size % 8 == 0
    got, got_lengths, got_ids = rlz.read_packed_archive(path)
    assert got == s and got_lengths.dtype == np.uint64 and got_lengths.tolist() == lengths and got_ids == names
    assert model.parse_container(raw) == (s, lengths, names)
    # an empty archive, no target
    empty = model.pack(b"ACGT", np.zeros(0, dtype=model.FACTOR_DTYPE), b"", [])
    rlz.write_packed_archive(path, empty, [], None if ids is None else [])
    got, got_lengths, got_ids = rlz.read_packed_archive(path)
    assert got == empty and len(got_lengths) == 0 and got_ids == (None if ids is None else [])


def test_id_rules_are_those_of_archive_arrays(tmp_path):
    block, records, literals, lengths, s = _sample()
    k = len(lengths)
    for names in ([f"x{j}" for j in range(k - 1)], ["same"] * k, [f"x{j}" for j in range(k - 1)] + ["nul\0"]):
        with pytest.raises(ValueError):
            rlz.write_packed_archive(tmp_path / "bad.rlz", s, lengths, names)


def test_every_broken_container_is_a_value_error(tmp_path):
    block, records, literals, lengths, s = _sample()
    names = [f"t{j}" for j in range(len(lengths))]
    raw = model.container_bytes(s, lengths, names)
    path = tmp_path / "a.rlz"
    head = model.HEADER

    def refused(data, why):
        path.write_bytes(bytes(data))
        with pytest.raises(ValueError, match=why):
            rlz.read_packed_archive(path)
        with pytest.raises(ValueError):
            model.parse_container(bytes(data))

    def with_field(index, value):
        f = list(head.unpack_from(raw))
        f[index] = value
        return head.pack(*f) + raw[head.size:]

    path.write_bytes(raw)
    rlz.read_packed_archive(path)
    refused(b"noLZRLZ2" + raw[8:], "bad magic")
    refused(raw[:40], "bad magic")
    refused(with_field(1, 2), "version")
    refused(with_field(2, head.unpack_from(raw)[2] | 8), "flags")
    sizes = head.unpack_from(raw)[9:]
    for j in range(6):  # every section pushed past the end of the file
        refused(with_field(9 + j, sizes[j] + len(raw)), "ends behind the end of the file")
    refused(raw + b"\0" * 8, "behind the last section")
    refused(raw[:-8], "ends behind the end of the file|behind the last")
    # non-zero padding: the data section of this archive does not end on 8 bytes
    assert len(s["data"]) % 8
    at = head.size + sum(n + (-n % 8) for n in sizes[:5]) - 1
    refused(raw[:at] + b"\x01" + raw[at + 1:], "padding")
    # sizes that the counts rule out
    refused(with_field(5, head.unpack_from(raw)[5] + 2), "size")       # z: the control section is too short for it
    refused(with_field(6, head.unpack_from(raw)[6] + 8), "size")       # n_literals
    refused(with_field(3, head.unpack_from(raw)[3] + 4), "size")       # B
    refused(with_field(7, head.unpack_from(raw)[7] + 1), "sum")        # decoded
    refused(with_field(4, head.unpack_from(raw)[4] + 1), "target lengths")  # k


# ---- load dispatches on the magic; save without compact= is what it was -----------------------------------------------
def test_load_dispatches_on_the_magic_and_save_is_unchanged(tmp_path, monkeypatch):
    block, records, literals, lengths, s = _sample()
    names = [f"t{j}" for j in range(len(lengths))]
    arrays = rlz.archive_arrays(block, records, literals, lengths, names)
    calls = []

    class FakeHandle:
        target_lengths = np.asarray(lengths, dtype=np.uint64)

        def __init__(self, how, *args):
            calls.append((how, args))

        @classmethod
        def open_records(cls, *args):
            return cls("records", *args)

        @classmethod
        def open_packed(cls, *args):
            return cls("packed", *args)

        def close(self):
            pass

    monkeypatch.setattr(rlz._native, "RlzArchiveHandle", FakeHandle)
    monkeypatch.setattr(rlz._native, "get_device", lambda: 0)
    monkeypatch.setattr(rlz._native, "set_device", lambda d: None)
    npz, packed = tmp_path / "a.npz", tmp_path / "a.rlz"
    # save(path) of a host-built archive: byte for byte save_archive_arrays of the same arrays
    arc = rlz.RlzArchive(block, records, literals, lengths, ids=names)
    arc.save(npz)
    rlz.save_archive_arrays(tmp_path / "b.npz", arrays)
    with zipfile.ZipFile(npz) as z1, zipfile.ZipFile(tmp_path / "b.npz") as z2:  # (the zip directory carries the time)
        assert [(n, z1.read(n)) for n in z1.namelist()] == [(n, z2.read(n)) for n in z2.namelist()]
        assert z1.namelist() == [f"{k}.npy" for k in rlz.ARCHIVE_ARRAYS]
    calls.clear()
    loaded = rlz.RlzArchive.load(npz)
    assert [c[0] for c in calls] == ["records"] and loaded.ids == names
    rlz.write_packed_archive(packed, s, lengths, names)
    calls.clear()
    loaded = rlz.RlzArchive.load(packed)
    assert [c[0] for c in calls] == ["packed"] and calls[0][1][0] == s and list(calls[0][1][1]) == lengths
    assert loaded.ids == names and loaded.target_lengths == lengths and len(loaded) == len(lengths)
    for call in (lambda: loaded.append([b"ACGT"], ids=["new"]), loaded.finder):
        with pytest.raises(ValueError, match="needs an archive made by RlzArchive.from_index"):
            call()
    # a broken container is refused before a handle is opened
    packed.write_bytes(packed.read_bytes() + b"\0")
    calls.clear()
    with pytest.raises(ValueError, match="compact relative-LZ archive"):
        rlz.RlzArchive.load(packed)
    with pytest.raises(ValueError, match="not a relative-LZ archive"):
        rlz.RlzArchive.load(tmp_path / "missing.npz")
    assert calls == []


def test_entry_points_are_declared_and_exported():
    from pathlib import Path

    import noLZSS.genomics.rlz as shim
    header = (Path(__file__).resolve().parent.parent / "include" / "nolzss_hip.h").read_text()
    for name in ("nolzss_rlz_archive_pack", "nolzss_free_rlz_archive_packed", "nolzss_rlz_archive_open_packed"):
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(_lib.lib, name) and f"{name}(" in header
    for name in ("write_packed_archive", "read_packed_archive"):
        assert name in rlz.__all__ and name in shim.__all__ and getattr(shim, name) is getattr(rlz, name)
    assert callable(native.RlzArchiveHandle.pack) and callable(native.RlzArchiveHandle.open_packed)
    fields = dict(_lib.RlzArchivePacked._fields_)
    # two uint32, five uint64, four pointers, four uint64: no padding on a 64-bit host
    assert list(fields)[:7] == list(native.PACKED_COUNTS) and struct.calcsize("=II5Q4Q4Q") == \
        __import__("ctypes").sizeof(_lib.RlzArchivePacked)
