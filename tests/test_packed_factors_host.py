"""The compact container of factor records without a GPU: the sequential model (tests/packed_factors_model.py)
round-trips random record lists, every class edge of L and v, both colinear v = 0 cases and the oracle's factorizations
in every mode (decoded again by tests/decode_model.py); the host-only file writer and reader; the names are exported."""
import json
import random
import struct
from pathlib import Path

import numpy as np
import pytest

import decode_model
import genomes
import oracle_lib as oracle
import packed_factors_model as model
from nolzss_amd import _lib, utils
from nolzss_amd import _noLZSS as native

RC = model.RC_MASK
NEAR_END = model.MAX_TEXT - 3_000_000  # starts just below 2^32 - 2^19
KATS = json.loads((Path(__file__).resolve().parent / "golden" / "kats.json").read_text())


def _round_trip(records, literals):
    s = model.pack(records, literals)
    back, lit = model.unpack(s)
    assert np.array_equal(back, records) and lit == bytes(literals)
    assert model.pack(back, lit) == s
    bare = model.pack(records)
    assert bare["literal_mode"] == 2 and bare["literals"] == b"" and bare["n_literals"] == s["n_literals"]
    assert bare["control"] == s["control"] and bare["data"] == s["data"]
    back, lit = model.unpack(bare)
    assert np.array_equal(back, records) and lit is None
    return s


def _nibbles(s):
    c = s["control"]
    return [(c[i >> 1] >> (4 * (i & 1))) & 15 for i in range(s["z"])]


# ---- random record lists -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(40))
def test_unpack_inverts_pack_on_random_records(seed):
    rng = random.Random(seed)
    first = rng.choice((0, 0, 1, 77, 100_000, NEAR_END, 3 << 30))
    records, literals = model.random_records(rng, rng.choice((1, 2, 3, 50, 501)), first_start=first,
                                             alphabet=rng.choice((b"ACGT", b"ACGTN", bytes(range(256)))))
    s = _round_trip(records, literals)
    assert s["first_start"] == first and s["decoded"] == int(records["length"].sum())
    assert all(c is None or c < 1 << 33 for c in model.code_records(records)[3])


def test_no_records():
    empty = np.zeros(0, dtype=model.FACTOR_DTYPE)
    s = _round_trip(empty, b"")
    assert s == {"literal_mode": 1, "first_start": 0, "z": 0, "n_literals": 0, "decoded": 0, "control": b"", "data": b"",
                 "literals": b""}


# ---- class edges ---------------------------------------------------------------------------------------------------
def test_length_classes():
    b = model.Builder(1 << 20)
    for L in (1, 255, 256, 65_535, 65_536):
        b.copy(3, L).copy(10, L, rc=True)
    s = _round_trip(b.records(), b.literals)
    assert [n & 3 for n in _nibbles(s)] == [1, 1, 1, 1, 2, 2, 2, 2, 3, 3]
    assert s["data"][:1] == b"\x01"


def test_code_class_edges():
    b = model.edge_builder()
    codes = [c for c in b.codes if c is not None]
    assert codes[1:] == [0, (1 << 16) - 1, 1 << 16, (1 << 32) + 1, (1 << 32) - 1, 1 << 32, (1 << 33) - 1, (1 << 33) - 2]
    s = _round_trip(b.records(), b.literals)
    assert [n >> 2 for n in _nibbles(s)][1:] == [0, 1, 2, 3, 2, 3, 3, 3]
    assert model.code_records(b.records())[3] == b.codes


def test_both_signs_of_the_step():
    b = model.Builder(100_000)
    b.copy(50_000, 10)
    for e in (1, -1, 127, -128, 20_000, -20_000, 16_383, -16_384, 16_384, -16_385):
        b.copy_step(10, e=e)
    s = _round_trip(b.records(), b.literals)
    assert [c for c in b.codes[1:]] == [4, 2, 508, 510, 80_000, 79_998, 65_532, 65_534, 65_536, 65_538]
    assert [n >> 2 for n in _nibbles(s)][1:] == [1, 1, 1, 1, 2, 2, 1, 1, 2, 2]


def test_colinear_copies_on_both_strands_have_v_0():
    b = model.Builder(0)
    for c in b"ACGTACGTTGCA":
        b.literal(bytes([c]))
    b.copy(0, 4)                      # forward
    b.literal(b"N").literal(b"A")
    b.copy_step(3)                    # goes on behind two literals: x = 0 + 4 + 2
    assert b.rows[-1] == (18, 3, 6) and b.codes[-1] == 0
    b.copy(10, 5, rc=True)            # the other strand
    b.literal(b"C")
    b.copy_step(4)                    # goes on colinearly: the source moves DOWN by the literal and its own length
    assert b.rows[-1] == (27, 4, RC | 5) and b.codes[-1] == 0
    s = _round_trip(b.records(), b.literals)
    assert s["literal_mode"] == 0 and _nibbles(s)[-1] == 1 and _nibbles(s)[-4] == 1


def test_first_record_a_copy_needs_first_start():
    b = model.Builder(50)
    b.copy(10, 40, rc=True).literal(b"T").copy_step(2)
    s = _round_trip(b.records(), b.literals)
    assert s["first_start"] == 50 and s["decoded"] == 43 and s["literals"] == b"\x03"


def test_literal_modes():
    b = model.Builder(0)
    for c in b"ACGTA":
        b.literal(bytes([c]))
    s = model.pack(b.records(), b.literals)
    assert s["literal_mode"] == 1 and s["literals"] == bytes([0 | 1 << 2 | 2 << 4 | 3 << 6, 0])
    b.literal(b"a")
    s = model.pack(b.records(), b.literals)
    assert s["literal_mode"] == 0 and s["literals"] == b"ACGTAa"


# ---- refusals of the model -----------------------------------------------------------------------------------------
def test_pack_refusals_name_the_first_record():
    ok = [(0, 1, 0), (1, 1, 1), (2, 2, 0)]
    rows = lambda r: np.array(r, dtype=model.FACTOR_DTYPE)  # noqa: E731
    model.pack(rows(ok), b"AC")
    for bad, lit, rule, rec in [
        ([(0, 1, 0), (2, 1, 2)], b"AC", "tiling", 1),
        ([(0, 1, 0), (1, 0, 0), (1, 1, 1)], b"AC", "tiling", 1),
        ([(0, 2, 0)], b"A", "literal length", 0),
        ([(0, 1, 0), (1, 1, 1), (2, 2, 1)], b"AC", "source range", 2),
        ([(0, 1, 0), (1, 1, 1), (2, 2, RC | 1)], b"AC", "source range", 2),
        (ok, b"A", "literal count", 1),
        (ok, b"ACG", "literal count", 3),
        ([(model.MAX_TEXT - 1, 1, model.MAX_TEXT - 1), (model.MAX_TEXT, 1, model.MAX_TEXT)], b"AC", "tiling", 1),
    ]:
        with pytest.raises(model.FormatError) as e:
            model.pack(rows(bad), lit)
        assert (e.value.rule, e.value.index) == (rule, rec), bad


def planted(s, **changes):
    out = dict(s)
    out.update(changes)
    return out


def test_unpack_refusals_name_the_smallest_record():
    b = model.Builder(1000)
    for j in range(40):
        b.copy(j, 300).literal(b"G").copy_step(7)
    s = model.pack(b.records(), b.literals)
    assert s["z"] == 120
    control = bytearray(s["control"])
    control[9] |= 4 << 4                            # record 19 is a literal: b = 1
    control[30] |= 8 << 0                           # and record 60
    with pytest.raises(model.FormatError) as e:
        model.unpack(planted(s, control=bytes(control)))
    assert (e.value.index, e.value.rule) == (19, "literal nibble")
    for data, rule in ((s["data"][:-1], "data size"), (s["data"] + b"\0", "data size")):
        with pytest.raises(model.FormatError) as e:
            model.unpack(planted(s, data=data))
        assert (e.value.index, e.value.rule) == (120, rule)
    odd = model.pack(b.records()[:119], b.literals)  # (record 118 is the last literal)
    control = bytearray(odd["control"])
    control[-1] |= 1 << 4
    with pytest.raises(model.FormatError) as e:
        model.unpack(planted(odd, control=bytes(control)))
    assert (e.value.index, e.value.rule) == (119, "spare nibble")
    for nlit, index in ((39, 118), (41, 120)):      # one too few: literal number 40 is record 118; one too many: behind
        lit = s["literals"] if (nlit + 3) // 4 == len(s["literals"]) else s["literals"] + b"\0"
        with pytest.raises(model.FormatError) as e:
            model.unpack(planted(s, n_literals=nlit, literals=lit))
        assert (e.value.index, e.value.rule) == (index, "literal count")
    with pytest.raises(model.FormatError) as e:
        model.unpack(planted(s, decoded=s["decoded"] + 1))
    assert (e.value.index, e.value.rule) == (120, "decoded length")
    with pytest.raises(ValueError):
        model.unpack(planted(s, literals=s["literals"] + b"\0"))
    with pytest.raises(ValueError):
        model.unpack(planted(s, first_start=model.MAX_TEXT - 100))


# ---- the oracle's factorizations -----------------------------------------------------------------------------------
def _seq(name):
    return b"".join(s for _, s in genomes.records(name))


def _kat_inputs(groups):
    out = []
    for g in groups:
        for v in KATS[g]:
            if "input" in v:
                out.append(v["input"].encode())
            else:
                word, times = v["input_repeat"]
                out.append(word.encode() * times)
    return out


@pytest.mark.parametrize("text", _kat_inputs(["plain", "derived_plain"]) + [_seq("short_dna1")], ids=lambda t: f"n{len(t)}")
def test_oracle_plain_packs_and_decodes(text):
    f = oracle.factors_array(text)
    s = _round_trip(f, decode_model.literal_symbols(text, f))
    back, lit = model.unpack(s)
    assert decode_model.decode(back, lit)[0] == text
    assert s["first_start"] == 0 and s["decoded"] == len(text)


@pytest.mark.parametrize("text", _kat_inputs(["dna_w_rc", "derived_dna_w_rc"]) + [b"ATGCAT", _seq("short_dna2")],
                         ids=lambda t: f"n{len(t)}")
def test_oracle_rc_packs_and_decodes(text):
    S, orig, _ = oracle.prepare_multiple_dna_w_rc([text])
    f = oracle.factors_array_multiple_dna_w_rc(S)
    s = _round_trip(f, decode_model.literal_symbols(S, f))
    back, lit = model.unpack(s)
    assert decode_model.decode(back, lit)[0] == text.upper()


def test_oracle_t7_after_t3_packs_and_decodes():
    t3, t7 = _seq("T3"), _seq("T7")
    prefix = t3 + b"\x01"
    f = oracle.factors_array(prefix + t7, start_pos=len(prefix))
    s = _round_trip(f, decode_model.literal_symbols(prefix + t7, f))
    assert s["first_start"] == len(prefix) and s["decoded"] == len(t7)
    back, lit = model.unpack(s)
    assert decode_model.decode(back, lit, prefix)[0] == prefix + t7
    # a factor file, not a compressor: well below the 24-byte records, near the text at 2 bits per base
    size = len(s["control"]) + len(s["data"]) + len(s["literals"])
    assert size * 4 < 24 * s["z"]


# ---- the file ------------------------------------------------------------------------------------------------------
def _sections(seed=5, z=301, **kw):
    records, literals = model.random_records(random.Random(seed), z, **kw)
    return model.pack(records, literals)


@pytest.mark.parametrize("kw", [{}, {"alphabet": b"ACGTN"}, {"first_start": NEAR_END}, {"z": 0}, {"z": 1}])
def test_file_round_trip(tmp_path, kw):
    s = _sections(**kw)
    path = tmp_path / "factors.nolzfac"
    size = utils.write_packed_factors(path, s)
    raw = path.read_bytes()
    assert size == len(raw) == 72 + sum(len(s[k]) + (-len(s[k]) % 8) for k in ("control", "data", "literals"))
    assert raw[:8] == b"noLZFAC1" and struct.unpack_from("<II7Q", raw, 8) == (
        1, s["literal_mode"], s["first_start"], s["z"], s["n_literals"], s["decoded"], len(s["control"]), len(s["data"]),
        len(s["literals"]))
    assert utils.read_packed_factors(path) == s
    bare = dict(s, literal_mode=2, literals=b"")
    utils.write_packed_factors(path, bare)
    assert utils.read_packed_factors(path) == bare


def test_the_reader_names_what_is_wrong(tmp_path):
    s = _sections()
    path = tmp_path / "f.bin"
    utils.write_packed_factors(path, s)
    raw = path.read_bytes()

    def refused(data, word):
        path.write_bytes(bytes(data))
        with pytest.raises(utils.NoLZSSError, match=word):
            utils.read_packed_factors(path)

    def with_field(index, value, fmt="Q"):
        out = bytearray(raw)
        struct.pack_into("<" + fmt, out, index, value)
        return out

    refused(b"noLZRLZ1" + raw[8:], "wrong magic")
    refused(with_field(8, 2, "I"), "unknown version")
    refused(with_field(12, s["literal_mode"] | 4, "I"), "unknown flag bits")
    refused(with_field(12, 3, "I"), "unknown flag bits")
    refused(with_field(24, s["z"] + 2), "section sizes disagree with the counts: the control")
    refused(with_field(32, s["n_literals"] + 4), "section sizes disagree with the counts: the literals")
    refused(with_field(48, len(s["control"]) + 8), "section sizes disagree")
    refused(raw[:40], "truncated")
    refused(raw[:-8], "truncated")
    refused(with_field(56, len(s["data"]) + 800), "truncated")
    refused(raw + b"\0" * 8, "trailing bytes")
    if len(s["data"]) % 8:
        out = bytearray(raw)
        out[72 + len(s["control"]) + (-len(s["control"]) % 8) + len(s["data"])] = 1
        refused(out, "padding")
    with pytest.raises(utils.NoLZSSError, match="File not found"):
        utils.read_packed_factors(tmp_path / "none")
    with pytest.raises(ValueError):
        utils.write_packed_factors(path, dict(s, z=s["z"] + 2))


# ---- names ---------------------------------------------------------------------------------------------------------
def test_entry_points_are_declared_and_exported():
    import noLZSS
    import nolzss_amd
    header = (Path(__file__).resolve().parent.parent / "include" / "nolzss_hip.h").read_text()
    for name in ("nolzss_factors_pack", "nolzss_factorize_packed", "nolzss_factorize_packed_device",
                 "nolzss_free_packed_factors", "nolzss_factors_unpack", "nolzss_decode_packed"):
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(_lib.lib, name) and f"{name}(" in header
    for name in ("factorize_packed", "pack_factors", "unpack_factors", "decode_packed", "write_packed_factors",
                 "read_packed_factors"):
        assert name in nolzss_amd.__all__ and name in noLZSS.__all__ and callable(getattr(noLZSS, name))
    for name in ("factorize_packed", "factorize_packed_device", "pack_factors", "unpack_factors", "decode_packed_array"):
        assert callable(getattr(native, name)) and getattr(noLZSS._noLZSS, name) is getattr(native, name)
    # two uint32, four uint64, three pointers, three uint64: no padding on a 64-bit host
    import ctypes as C
    assert C.sizeof(_lib.PackedFactors) == struct.calcsize("=II4Q3Q3Q") == 88
    assert [f[0] for f in _lib.PackedFactors._fields_ if f[0] != "reserved"][:5] == list(native.PACKED_FACTOR_COUNTS)


def test_what_needs_no_device():
    """z == 0 and every host-side refusal return before a device is touched"""
    empty = np.zeros(0, dtype=model.FACTOR_DTYPE)
    want = model.pack(empty, b"")
    assert native.pack_factors(empty, b"") == want
    assert native.pack_factors(empty) == dict(want, literal_mode=2)
    assert native.factorize_packed(b"") == want and native.factorize_packed(b"", with_rc=True, literals=False)["literal_mode"] == 2
    records, literals = native.unpack_factors(want)
    assert len(records) == 0 and literals == b""
    assert native.unpack_factors(dict(want, literal_mode=2))[1] is None
    assert native.decode_packed_array(want)[0].tobytes() == b""
    with pytest.raises(ValueError, match="literal count"):
        native.pack_factors(empty, b"A")
    s = _sections()
    for changes, word in [({"literal_mode": 3}, "literal_mode"), ({"control": s["control"] + b"\0"}, "control section"),
                          ({"literals": s["literals"] + b"\0"}, "literal section"),
                          ({"first_start": model.MAX_TEXT - 100}, "text too long"),
                          ({"decoded": model.MAX_TEXT + 1}, "text too long")]:
        with pytest.raises(ValueError, match=word):
            native.unpack_factors(dict(s, **changes))
    with pytest.raises(ValueError, match="literal_mode 2"):
        native.decode_packed_array(dict(s, literal_mode=2, literals=b""))
    with pytest.raises(ValueError, match="first_start"):
        native.decode_packed_array(s, prefix=b"A")
    for changes, word in [({"data": b"\0"}, "data size"), ({"n_literals": 1, "literals": b"\0"}, "literal count"),
                          ({"decoded": 1}, "decoded length")]:
        with pytest.raises(ValueError, match=word):
            native.unpack_factors(dict(want, **changes))
