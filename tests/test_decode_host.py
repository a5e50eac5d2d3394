"""The decoder without a GPU: the sequential model (tests/decode_model.py) round-trips the oracle's factorizations in
every mode, the host-only entry points (literal extractor, the z == 0 path, argument checks) behave as the header
says, rlz_decode refuses a bad factor before any native call, and the new names are exported everywhere."""
import ctypes as C
import json
from pathlib import Path

import numpy as np
import pytest

import decode_model as model
import genomes
import oracle_lib as oracle
from nolzss_amd import _lib
from nolzss_amd import _noLZSS as native

KATS = json.loads((Path(__file__).resolve().parent / "golden" / "kats.json").read_text())
RC_MASK = 1 << 63


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


PLAIN_KATS = _kat_inputs(["plain", "derived_plain"])
RC_KATS = _kat_inputs(["dna_w_rc", "dna_w_rc_partial", "derived_dna_w_rc",
                       "reference_doc_example_contradicted_by_the_code"]) + [b"ATGCAT"]


def _seq(name):
    return b"".join(s for _, s in genomes.records(name))


# ---- the model round-trips the oracle ----------------------------------------------------------------------------
@pytest.mark.parametrize("text", PLAIN_KATS + [_seq("short_dna1"), _seq("short_dna2")], ids=lambda t: f"n{len(t)}")
def test_model_roundtrips_plain(text):
    f = oracle.factors_array(text)
    lit = model.literal_symbols(text, f)
    got, depth = model.decode(f, lit)
    assert got == text
    assert model.decode_slices(f, lit) == text
    assert all(int(r & ~np.uint64(RC_MASK)) + int(l) <= int(s) for s, l, r in zip(f["start"], f["length"], f["ref"])
               if r != s), "source range"


def test_model_depth_of_abracadabra():
    f = oracle.factors_array(b"abracadabra")
    assert model.decode(f, model.literal_symbols(b"abracadabra", f)) == (b"abracadabra", 2)


@pytest.mark.parametrize("text", RC_KATS, ids=lambda t: t.decode())
def test_model_roundtrips_rc(text):
    S, orig, sent = oracle.prepare_multiple_dna_w_rc([text])
    f = oracle.factors_array_multiple_dna_w_rc(S)
    got, _ = model.decode(f, model.literal_symbols(S, f))
    assert got == S[:orig - 1] == text
    assert model.decode_slices(f, model.literal_symbols(S, f)) == text


def test_model_atgcat_uses_the_other_strand():
    S, orig, _ = oracle.prepare_multiple_dna_w_rc([b"ATGCAT"])
    f = oracle.factors_array_multiple_dna_w_rc(S)
    assert (f["ref"] >> np.uint64(63)).any()


def test_model_roundtrips_t7_after_t3():
    t3, t7 = _seq("T3"), _seq("T7")
    prefix = t3 + b"\x01"
    f = oracle.factors_array(prefix + t7, start_pos=len(prefix))
    lit = model.literal_symbols(prefix + t7, f)
    got, depth = model.decode(f, lit, prefix)
    assert got == prefix + t7
    assert model.decode_slices(f, lit, prefix) == prefix + t7


def test_model_roundtrips_bacterial_records_with_rc():
    seqs = [s for _, s in genomes.records("test_bacterial_dna")]
    assert len(seqs) == 2
    S, orig, sent = oracle.prepare_multiple_dna_w_rc(seqs)
    f = oracle.factors_array_multiple_dna_w_rc(S)
    lit = model.literal_symbols(S, f)
    got, depth = model.decode(f, lit)
    assert got == S[:orig - 1]
    assert (f["ref"] >> np.uint64(63)).any()
    assert sum(1 for c in lit if c not in b"ACGT") == 1, "the sentinel between the records is a literal"
    assert all(int(r & ~np.uint64(RC_MASK)) + int(l) <= int(s) for s, l, r in zip(f["start"], f["length"], f["ref"])
               if r != s)


def test_deep_chain_in_the_model():
    rows, lit = model.deep_chain(20_000)
    text, depth = model.decode(rows, lit)
    assert depth == 9_999 and len(text) == 20_000
    assert text == (b"ACGTGTAC" * 2500)
    plain, d2 = model.decode(*model.deep_chain(20_000, alternate=False))
    assert plain == b"AC" * 10_000 and d2 == 9_999
    every, d3 = model.decode(*model.deep_chain(20_000, all_rc=True))
    assert every == b"ACGT" * 5_000 and d3 == 9_999


def test_model_refusals():
    ok = [(0, 1, 0), (1, 1, 1), (2, 2, 0)]
    assert model.decode(ok, b"AC")[0] == b"ACAC"
    for rows, lit, rule, rec in [
        ([(0, 1, 0), (2, 1, 2)], b"AC", "tiling", 1),
        ([(0, 1, 0), (1, 1, 1), (2, 2, 1)], b"AC", "source range", 2),
        ([(0, 2, 0)], b"A", "literal length", 0),
        (ok, b"A", "literal count", 1),
        (ok, b"ACG", "literal count", 3),
        ([(0, 1, 0), (1, 1, RC_MASK)], b"\x02", "complement", 1),
    ]:
        with pytest.raises(model.DecodeError) as e:
            model.decode(rows, lit)
        assert (e.value.rule, e.value.record) == (rule, rec)
    with pytest.raises(model.DecodeError):
        model.decode(ok, b"AC", prefix=b"T")  # the first start differs from prefix_len


# ---- nolzss_literal_symbols ----------------------------------------------------------------------------------------
def test_literal_symbols_equal_the_model():
    for text in PLAIN_KATS + [_seq("short_dna1")]:
        f = oracle.factors_array(text)
        assert native.literal_symbols(text, f) == model.literal_symbols(text, f)
        rows = list(zip(f["start"].tolist(), f["length"].tolist(), f["ref"].tolist()))
        assert native.literal_symbols(text, rows) == model.literal_symbols(text, f)
    S, orig, _ = oracle.prepare_multiple_dna_w_rc([b"ATGCAT"])
    f = oracle.factorize_multiple_dna_w_rc(S)  # 4-tuples
    assert native.literal_symbols(S, f) == model.literal_symbols(S, f) == b"ATG"
    assert native.literal_symbols(b"", []) == b""


def test_literal_symbols_refuses_a_start_beyond_the_text():
    with pytest.raises(ValueError, match="record 1"):
        native.literal_symbols(b"ab", [(0, 1, 0), (2, 1, 2)])
    assert native.literal_symbols(b"ab", [(0, 1, 0), (1, 5, 0)]) == b"a"  # (a copy is not read)


# ---- nolzss_decode without a device ----------------------------------------------------------------------------------
def test_no_records_return_the_prefix_without_a_device():
    text, info = native.decode_array([], b"", prefix=b"ACGT\x01")
    assert text.tobytes() == b"ACGT\x01"
    assert info == {"n": 5, "z": 0, "n_literals": 0, "resolved_at_expand": 0, "rounds": 0, "max_active": 0}
    text, info = native.decode_array(np.zeros(0, dtype=native.FACTOR_DTYPE), b"")
    assert len(text) == 0 and info["n"] == 0
    with pytest.raises(ValueError, match="literal count"):
        native.decode_array([], b"A")


def test_null_pointers_and_counts_are_argument_errors():
    lib = _lib.lib
    out, n, info = C.c_void_p(), C.c_size_t(), _lib.DecodeInfo()
    rec = np.array([(0, 1, 0)], dtype=native.FACTOR_DTYPE)
    lit = np.frombuffer(b"A", dtype=np.uint8)
    cases = [
        (None, 1, lit.ctypes.data, 1, None, 0, b"factors pointer is null"),
        (rec.ctypes.data, 1, None, 1, None, 0, b"literals pointer is null"),
        (rec.ctypes.data, 1, lit.ctypes.data, 1, None, 3, b"prefix pointer is null"),
    ]
    for f, z, lp, ln, pp, pn, msg in cases:
        assert lib.nolzss_decode(f, z, lp, ln, pp, pn, 0, C.byref(out), C.byref(n), C.byref(info)) == _lib.ERR_INVALID_ARGUMENT
        assert msg in lib.nolzss_last_error()
        assert not out.value and n.value == 0
    assert lib.nolzss_decode(None, 0, None, 0, None, 0, 0, None, C.byref(n), None) == _lib.ERR_INVALID_ARGUMENT
    assert lib.nolzss_decode(None, 0, None, 0, None, 0, 0, C.byref(out), None, None) == _lib.ERR_INVALID_ARGUMENT
    # a text beyond the 32-bit pipeline is refused up front, from the last record alone
    far = np.array([(0, 1 << 33, 0)], dtype=native.FACTOR_DTYPE)
    assert lib.nolzss_decode(far.ctypes.data, 1, None, 0, None, 0, 0, C.byref(out), C.byref(n), None) == _lib.ERR_INVALID_ARGUMENT
    assert b"text too long" in lib.nolzss_last_error()
    cnt, first = C.c_void_p(), C.c_size_t()
    assert lib.nolzss_literal_symbols(None, 4, None, 0, C.byref(cnt), C.byref(first)) == _lib.ERR_INVALID_ARGUMENT
    assert lib.nolzss_literal_symbols(None, 0, None, 1, C.byref(cnt), C.byref(first)) == _lib.ERR_INVALID_ARGUMENT
    assert lib.nolzss_literal_symbols(None, 0, None, 0, None, None) == _lib.ERR_INVALID_ARGUMENT
    z, m, fm = C.c_size_t(), C.c_uint64(), C.c_uint64()
    assert lib.nolzss_roundtrip(None, 5, 0, 0, C.byref(z), C.byref(m), C.byref(fm), None) == _lib.ERR_INVALID_ARGUMENT
    assert lib.nolzss_roundtrip(b"ACGTA", 5, 0, 0, None, C.byref(m), C.byref(fm), None) == _lib.ERR_INVALID_ARGUMENT
    assert lib.nolzss_roundtrip(None, 0, 1, 0, C.byref(z), C.byref(m), C.byref(fm), None) == _lib.OK
    assert (z.value, m.value, fm.value) == (0, 0, (1 << 64) - 1)
    assert lib.nolzss_debug_count_mismatches(None, None, 3, 0, C.byref(m), C.byref(fm)) == _lib.ERR_INVALID_ARGUMENT


def test_factor_forms_are_accepted():
    with pytest.raises(ValueError, match="3 or 4 fields"):
        native.literal_symbols(b"ab", [(0, 1)])
    four = native._decode_records([(3, 3, 0, True), (6, 2, 2, False)])
    assert four["ref"].tolist() == [RC_MASK, 2]
    arr = np.array([(3, 3, RC_MASK)], dtype=native.FACTOR_DTYPE)
    assert native._decode_records(arr)["ref"].tolist() == [RC_MASK]


# ---- rlz_decode: the block, the rebasing, the refusal ----------------------------------------------------------------
def _rlz(rows):
    from nolzss_amd.genomics import rlz
    return np.array(rows, dtype=rlz.RLZ_DTYPE)


def test_rlz_absolute_records_and_literals():
    from nolzss_amd.genomics import rlz
    refs = [b"ACGT", b"ggA"]
    factors = [_rlz([(0, 3, 1, False, False), (3, 1, 0, False, True), (4, 2, 5, True, False)]), _rlz([]),
               _rlz([(0, 1, 0, False, True)])]
    block, recs, lengths = rlz.absolute_records(refs, factors)
    assert block == b"ACGT" + rlz.SEPARATOR + b"GGA" and rlz.SEPARATOR not in (b"A", b"C", b"G", b"T")
    assert lengths == [6, 0, 1]
    assert recs["start"].tolist() == [8, 11, 12, 14] and recs["length"].tolist() == [3, 1, 2, 1]
    assert recs["ref"].tolist() == [1, 11, RC_MASK | 5, 14]
    assert rlz.rlz_literals([b"CGTnCC", b"", b"t"], factors) == [b"N", b"", b"T"]


def test_rlz_decode_refuses_a_factor_across_a_separator_before_any_native_call(monkeypatch):
    from nolzss_amd.genomics import rlz

    def never(*a, **k):
        raise AssertionError("the native decoder must not be called")
    monkeypatch.setattr(native, "decode_array", never)
    refs = [b"ACGT", b"GGA"]  # separator at block position 4
    with pytest.raises(ValueError, match="target 1, factor 0"):
        rlz.rlz_decode(refs, [_rlz([]), _rlz([(0, 3, 2, False, False)])], [b"", b""])
    with pytest.raises(ValueError, match="target 0, factor 0"):
        rlz.rlz_decode(refs, [_rlz([(0, 1, 4, True, False)])], [b""])  # on the separator
    with pytest.raises(ValueError, match="leaves the reference block"):
        rlz.rlz_decode(refs, [_rlz([(0, 4, 5, False, False)])], [b""])  # past the end
    with pytest.raises(AssertionError):
        rlz.rlz_decode(refs, [_rlz([(0, 3, 5, False, False)])], [b""])  # [5, 8) is fine: the decoder is reached


# ---- names -------------------------------------------------------------------------------------------------------------
def test_new_names_are_exported():
    for name in ["nolzss_literal_symbols", "nolzss_decode", "nolzss_roundtrip", "nolzss_roundtrip_device",
                 "nolzss_debug_count_mismatches"]:
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(_lib.lib, name)
    import nolzss_amd
    import nolzss_amd.genomics.rlz as amd_rlz
    import noLZSS
    import noLZSS.genomics.rlz as ref_rlz
    for pkg in (nolzss_amd, noLZSS):
        assert "decode" in pkg.__all__ and "literal_symbols" in pkg.__all__
        assert callable(pkg.decode) and callable(pkg.literal_symbols)
    for mod in (amd_rlz, ref_rlz):
        assert "rlz_decode" in mod.__all__ and "rlz_literals" in mod.__all__
        assert callable(mod.rlz_decode) and callable(mod.rlz_literals)
    for name in ["literal_symbols", "decode_array", "roundtrip_check", "roundtrip_device", "debug_count_mismatches"]:
        assert callable(getattr(native, name))
    assert noLZSS.literal_symbols(b"abcabcabc", [(0, 1, 0), (1, 1, 1), (2, 1, 2), (3, 3, 0), (6, 3, 0)]) == b"abc"
