"""The decoder on the device (decode.hip, decode_api.hip): factors and literals back to text by pointer jumping.  Every
comparison is byte equality with the sequential model (tests/decode_model.py) or with the input text; the number of
jump rounds is held against the chain depth the model measures."""
import functools
import json
import math
from pathlib import Path

import numpy as np
import pytest

import decode_model as model
import gen
import genomes

pytestmark = pytest.mark.gpu

RC_MASK = 1 << 63
KATS = json.loads((Path(__file__).resolve().parent / "golden" / "kats.json").read_text())
RC_KATS = sorted({v["input"].encode() for g in ("dna_w_rc", "dna_w_rc_partial", "derived_dna_w_rc",
                                                  "reference_doc_example_contradicted_by_the_code") for v in KATS[g]}
                 | {b"ATGCAT"})


@pytest.fixture(scope="module")
def native():
    from nolzss_amd import _noLZSS
    assert _noLZSS.device_count() >= 1, "no MI355X visible"
    return _noLZSS


def round_bound(depth):
    return math.ceil(math.log2(max(depth, 1))) + 2


def decode_and_check(native, records, literals, expect, prefix=b""):
    """device against model against the expected text; the round bound from the model's depth -> info"""
    got, info = native.decode_array(records, literals, prefix)
    exp, depth = model.decode(records, literals, prefix)
    assert exp == expect
    assert got.dtype == np.uint8 and got.tobytes() == expect
    assert info["n"] == len(expect) and info["z"] == len(records) and info["n_literals"] == len(literals)
    assert info["rounds"] <= round_bound(depth), (info, depth)
    assert info["resolved_at_expand"] + info["max_active"] == len(expect) - len(prefix)
    assert (info["rounds"] == 0) == (info["max_active"] == 0)
    return info


def roundtrip(native, text, with_rc=False):
    f = native.factorize_dna_w_rc_array(text) if with_rc else native.factorize_array(text)
    lit = native.literal_symbols(text, f)
    info = decode_and_check(native, f, lit, text)
    return f, lit, info


# ---- KATs and the smallest inputs ------------------------------------------------------------------------------------
def test_abracadabra(native):
    f, lit, info = roundtrip(native, b"abracadabra")
    assert lit == b"abrcd" and info["rounds"] <= 2
    assert native.decode_array([(0, 1, 0), (1, 1, 1), (2, 1, 2), (3, 1, 0), (4, 1, 4), (5, 1, 0), (6, 1, 6), (7, 4, 0)],
                               b"abrcd")[0].tobytes() == b"abracadabra"


def test_atgcat_with_rc(native):
    f, lit, info = roundtrip(native, b"ATGCAT", with_rc=True)
    assert (f["ref"] >> np.uint64(63)).any() and lit == b"ATG"
    four = [(0, 1, 0, False), (1, 1, 1, False), (2, 1, 2, False), (3, 3, 0, True)]
    assert native.decode_array(four, b"ATG")[0].tobytes() == b"ATGCAT"


def test_one_symbol_and_one_copy(native):
    info = decode_and_check(native, [(0, 1, 0)], b"x", b"x")
    assert info["rounds"] == 0 and info["max_active"] == 0
    info = decode_and_check(native, [(0, 1, 0), (1, 1, 0)], b"\xff", b"\xff\xff")
    assert info["rounds"] == 1 and info["max_active"] == 1
    decode_and_check(native, [(0, 1, 0), (1, 1, RC_MASK)], b"G", b"GC")


# ---- round trip of the device's own factorizations -----------------------------------------------------------------
def _fibonacci_word(n):
    a, b = b"b", b"a"
    while len(b) < n:
        a, b = b, b + a
    assert len(b) == n
    return b


@functools.lru_cache(maxsize=None)
def _repeat_text():
    return gen.repeat_dna(200_000, seed=7, lo=16, hi=2048).tobytes()


def _plain_inputs():
    rng = np.random.default_rng(30)
    x = gen.random_dna(10_000, seed=31).tobytes()
    cases = {f"random{n}": gen.random_dna(n, seed=n).tobytes() for n in (4095, 4096, 4097, 3 * 4096 + 5)}
    cases.update({"repeat200k": _repeat_text(), "a5000": b"A" * 5000, "fibonacci": _fibonacci_word(75_025),
                  "bytes256": rng.integers(0, 256, 30_000, dtype=np.uint8).tobytes(), "x_plus_x": x + x})
    return cases


@pytest.mark.parametrize("name", ["random4095", "random4096", "random4097", "random12293", "repeat200k", "a5000",
                                  "fibonacci", "bytes256", "x_plus_x"])
def test_roundtrip_plain(native, name):
    text = _plain_inputs()[name]
    f, lit, info = roundtrip(native, text)
    if name == "x_plus_x":
        k = int(f["length"].argmax())
        first, last = int(f["start"][k]), int(f["start"][k] + f["length"][k]) - 1
        assert last // 4096 - first // 4096 >= 2, "one factor spans three tiles"
    if name == "bytes256":
        assert len(set(text)) == 256


def _rc_inputs():
    v = gen.random_dna(9_000, seed=41).tobytes()
    cases = {"repeat60k": gen.repeat_dna(60_000, seed=9, lo=16, hi=512).tobytes(), "v_plus_rc": v + genomes.revcomp(v)}
    cases.update({"kat_" + t.decode(): t for t in RC_KATS})
    return cases


@pytest.mark.parametrize("name", ["repeat60k", "v_plus_rc"] + ["kat_" + t.decode() for t in RC_KATS])
def test_roundtrip_rc(native, name):
    text = _rc_inputs()[name]
    f, lit, info = roundtrip(native, text, with_rc=True)
    masked = (f["ref"] >> np.uint64(63)).astype(bool)
    if name == "v_plus_rc":
        k = int(np.where(masked, f["length"], 0).argmax())
        first, last = int(f["start"][k]), int(f["start"][k] + f["length"][k]) - 1
        assert last // 4096 - first // 4096 >= 2, "one reverse-complement factor spans tiles"
    if not name.startswith("kat_") or name == "kat_ATGCAT":
        assert masked.any(), "the input must exercise the other strand"


# ---- the deep hand-built chain -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["alternate", "none", "all"])
def test_deep_chain(native, kind):
    rows, lit = model.deep_chain(20_000, alternate=kind == "alternate", all_rc=kind == "all")
    expect = {"alternate": b"ACGTGTAC" * 2500, "none": b"AC" * 10_000, "all": b"ACGT" * 5_000}[kind]
    info = decode_and_check(native, rows, lit, expect)
    assert model.decode(rows, lit)[1] == 9_999
    assert info["rounds"] <= 16, "a decoder that hops one factor per round needs 9 999"
    assert info["max_active"] == 19_998 and info["resolved_at_expand"] == 2


# ---- prefix forms ------------------------------------------------------------------------------------------------------
def _seq(name):
    return b"".join(s for _, s in genomes.records(name))


def test_reference_and_target(native):
    t3, t7 = _seq("T3"), _seq("T7")
    f = native.factorize_w_reference(t3, t7)
    prefix = t3 + b"\x01"
    assert f[0][0] == len(prefix)
    lit = native.literal_symbols(prefix + t7, f)
    decode_and_check(native, f, lit, prefix + t7, prefix)


def test_dna_reference_and_target_with_rc(native):
    ref, tgt = _seq("short_dna2"), _seq("short_dna1")
    f = native.factorize_dna_w_reference_seq(ref, tgt)  # 4-tuples
    S, orig, sent = native.prepare_multiple_dna_sequences_w_rc_bytes([ref, tgt])
    start = len(ref) + 1
    assert f[0][0] == start
    n = f[-1][0] + f[-1][1]
    assert n == orig - 1
    lit = native.literal_symbols(S, f)
    decode_and_check(native, f, lit, S[:n], S[:start])


@pytest.mark.parametrize("with_rc", [True, False])
def test_concatenated_fasta_forms(native, tmp_path, with_rc):
    path = genomes.materialize("test_bacterial_dna", tmp_path)
    seqs = [s for _, s in native.debug_parse_fasta(path)]
    assert len(seqs) == 2
    if with_rc:
        f, sentinel_factors, ids = native.factorize_fasta_multiple_dna_w_rc(path)
        S = native.prepare_multiple_dna_sequences_w_rc_bytes(seqs)[0]
    else:
        f, sentinel_factors, ids = native.factorize_fasta_multiple_dna_no_rc(path)
        S = native.prepare_multiple_dna_sequences_no_rc_bytes(seqs)[0]
    n = f[-1][0] + f[-1][1]
    lit = native.literal_symbols(S, f)
    assert any(c not in b"ACGT" for c in lit), "the sentinel between the records comes from the literal stream"
    assert len(sentinel_factors) >= 1 and all(f[k][2] == f[k][0] and not f[k][3] for k in sentinel_factors)
    decode_and_check(native, f, lit, S[:n])
    if with_rc:
        assert any(r[3] for r in f)


# ---- refusals ------------------------------------------------------------------------------------------------------------
OK_ROWS = [(0, 1, 0), (1, 1, 1), (2, 2, 0), (4, 3, RC_MASK | 1)]  # AC AC + rc(CAC) = GTG


@pytest.mark.parametrize("rows, lit, prefix, pattern", [
    ([(0, 1, 0), (1, 1, 1), (3, 2, 0)], b"AC", b"", r"record 2 .*tiling"),                 # a gap
    ([(0, 1, 0), (1, 1, 1), (2, 2, 1)], b"AC", b"", r"record 2 .*source range"),           # ref + length == start + 1
    ([(0, 1, 0), (1, 2, 1), (3, 1, 0)], b"AC", b"", r"record 1 .*literal length"),
    (OK_ROWS, b"A", b"", r"record 1 .*literal count"),                                       # one byte too few
    (OK_ROWS, b"ACG", b"", r"record 4 .*literal count"),                                     # one too many
    ([(0, 1, 0), (1, 1, 1), (2, 2, RC_MASK)], b"A\x02", b"", r"record 2 .*complement"),      # chain ends in a sentinel
    ([(1, 1, RC_MASK)], b"", b"\x02", r"record 0 .*complement"),                             # ... that lies in the prefix
    (OK_ROWS, b"AC", b"T", r"record 0 .*tiling"),                                            # first start != prefix_len
], ids=["gap", "overlap", "literal2", "too_few", "too_many", "sentinel_chain", "sentinel_prefix", "first_start"])
def test_refusals_name_the_record_and_leave_the_context_clean(native, rows, lit, prefix, pattern):
    with pytest.raises(model.DecodeError):
        model.decode(rows, lit, prefix)
    with pytest.raises(ValueError, match=pattern):
        native.decode_array(rows, lit, prefix)
    assert native.decode_array(OK_ROWS, b"AC")[0].tobytes() == b"ACACGTG"


def test_refusal_records_match_the_model(native):
    for rows, lit, prefix in [([(0, 1, 0), (1, 1, 1), (3, 2, 0)], b"AC", b""), (OK_ROWS, b"A", b""),
                              ([(0, 1, 0), (1, 1, 1), (2, 2, RC_MASK)], b"A\x02", b"")]:
        with pytest.raises(model.DecodeError) as e:
            model.decode(rows, lit, prefix)
        with pytest.raises(ValueError, match=f"record {e.value.record} "):
            native.decode_array(rows, lit, prefix)


# ---- wrong data decodes deterministically --------------------------------------------------------------------------------
def test_a_flipped_literal_decodes_as_the_model_says(native):
    text = _repeat_text()
    f = native.factorize_array(text)
    lit = bytearray(native.literal_symbols(text, f))
    lit[0] = ord("C") if lit[0] != ord("C") else ord("G")
    got, info = native.decode_array(f, bytes(lit))
    exp, _ = model.decode(f, bytes(lit))
    assert got.tobytes() == exp and exp != text
    a, b = np.frombuffer(text, dtype=np.uint8), np.frombuffer(exp, dtype=np.uint8)
    where = np.flatnonzero(a != b)
    assert len(where) >= 1 and where[0] == 0
    assert native.debug_count_mismatches(got, text) == (len(where), int(where[0]))


# ---- the comparison kernel -------------------------------------------------------------------------------------------------
def test_count_mismatches(native):
    rng = np.random.default_rng(50)
    a = rng.integers(0, 256, 10_000, dtype=np.uint8)
    assert native.debug_count_mismatches(a, a.copy()) == (0, None)
    for where in ([0], [9_999], sorted(rng.choice(10_000, 37, replace=False).tolist())):
        b = a.copy()
        b[where] ^= 0x55
        assert native.debug_count_mismatches(a, b) == (len(where), where[0])
    assert native.debug_count_mismatches(a[:5], a[:5] ^ 1) == (5, 0)  # shorter than one wide load
    assert native.debug_count_mismatches(b"", b"") == (0, None)


# ---- the device-resident round trip ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_rc", [False, True])
def test_roundtrip_check(native, with_rc):
    if with_rc:
        text = gen.repeat_dna(1 << 18, seed=12, lo=16, hi=1024).tobytes()
        z = native.count_factors_dna_w_rc(text)
    else:
        text = gen.repeat_dna(1 << 20, seed=11, lo=16, hi=4096).tobytes()
        z = native.count_factors(text)
    res = native.roundtrip_check(text, with_rc=with_rc)
    assert res["mismatches"] == 0 and res["first_mismatch"] is None
    assert res["z"] == z and res["n"] == len(text)
    assert 0 < res["n_literals"] <= 4 and 1 <= res["rounds"] <= 34
    assert res["resolved_at_expand"] + res["max_active"] == len(text)


def test_roundtrip_check_small(native):
    assert native.roundtrip_check(b"")["z"] == 0
    res = native.roundtrip_check(b"abracadabra")
    assert (res["z"], res["mismatches"], res["n_literals"]) == (8, 0, 5)
    res = native.roundtrip_check(b"atgcat", with_rc=True)  # (compared with the upper-cased strand)
    assert (res["z"], res["mismatches"], res["n"]) == (4, 0, 6)


# ---- relative LZ -------------------------------------------------------------------------------------------------------------
R1 = b"ACGGTCATTGCAAGCTTAGGCATCGA"
R2 = b"TTGACCGGTAAGGCCTTTAGACCA"


def _dna(n, seed, alphabet=b"ACGT"):
    rng = np.random.default_rng(seed)
    return np.frombuffer(alphabet, dtype=np.uint8)[rng.integers(0, len(alphabet), n)].tobytes()


def _cut_targets(ref, seed, lengths):
    rng = np.random.default_rng(seed)
    targets = []
    for n in lengths:
        t = b""
        while len(t) < n:
            kind = rng.random()
            a = int(rng.integers(0, len(ref) - 1))
            piece = ref[a:a + int(rng.integers(1, 400))]
            if kind < 0.45:
                t += piece
            elif kind < 0.8:
                t += genomes.revcomp(piece)
            else:
                t += _dna(int(rng.integers(1, 30)), int(rng.integers(1 << 30)))
        targets.append(t[:n])
    return targets


def _rlz_cases():
    ref = _dna(6000, 60)
    return {
        "equal": ([R1], [R1]),
        "revcomp": ([R1], [genomes.revcomp(R1)]),
        "literals": ([b"ATTATAATTTA"], [b"ATGAT", b"GCG"]),
        "boundary": ([R1, R2], [R1[-9:] + R2[:9]]),
        "empty_between": ([R1, R2], [R2[3:17], b"", genomes.revcomp(R1[2:20]) + b"A"]),
        "tiles": ([ref[:2500], ref[2500:]], _cut_targets(ref, 61, [5000, 0, 3777, 4096, 4999])),
    }


@pytest.mark.parametrize("with_rc", [True, False])
@pytest.mark.parametrize("name", ["equal", "revcomp", "literals", "boundary", "empty_between", "tiles"])
def test_rlz_decode(native, name, with_rc):
    from nolzss_amd.genomics import rlz
    refs, targets = _rlz_cases()[name]
    factors = rlz.rlz_factorize(refs, targets, with_rc=with_rc)
    literals = rlz.rlz_literals(targets, factors)
    got, info = rlz.rlz_decode(refs, factors, literals, return_info=True)
    assert got == targets
    assert info["rounds"] <= 1 and info["max_active"] == 0, "every pointer lands in the reference block"
    assert info["n_literals"] == sum(len(x) for x in literals)
    assert rlz.rlz_decode(refs, factors, literals) == targets
    if with_rc and name in ("revcomp", "tiles"):
        assert any(f["is_rc"].any() for f in factors)
    block, records, lengths = rlz.absolute_records(refs, factors)
    assert model.decode(records, b"".join(literals), block)[0][len(block):] == b"".join(targets)


def test_rlz_decode_of_nothing(native):
    from nolzss_amd.genomics import rlz
    assert rlz.rlz_decode([R1], [], []) == []
    factors = rlz.rlz_factorize([R1], [b"", b""])
    assert rlz.rlz_decode([R1], factors, rlz.rlz_literals([b"", b""], factors)) == [b"", b""]


# ---- the reference's import path ----------------------------------------------------------------------------------------------
def test_reference_import_path(native):
    from noLZSS import decode, factorize, literal_symbols
    f = factorize(b"abcabcabc")
    assert decode(f, literal_symbols(b"abcabcabc", f)) == b"abcabcabc"
    import nolzss_amd
    f = nolzss_amd.factorize_w_reference(b"GATTACA", b"TACAGATT")
    prefix = b"GATTACA\x01"
    assert nolzss_amd.decode(f, nolzss_amd.literal_symbols(prefix + b"TACAGATT", f), prefix) == prefix + b"TACAGATT"
