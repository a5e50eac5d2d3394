"""The compact container of factor records end to end on the device (factor_pack.hip, factor_pack_api.hip): for every
input factorize_packed gives the bytes pack_factors gives for the factorizer's own records, which are the bytes of the
sequential model (tests/packed_factors_model.py); unpack_factors gives the factorizer's records back by integer
equality and decode_packed the text, without the 24-byte records crossing PCIe."""
import functools

import numpy as np
import pytest

import gen
import genomes
import packed_factors_model as model

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def native():
    from nolzss_amd import _noLZSS
    assert _noLZSS.device_count() >= 1, "no MI355X visible"
    return _noLZSS


def _fibonacci_word(n):
    a, b = b"b", b"a"
    while len(b) < n:
        a, b = b, b + a
    assert len(b) == n
    return b


@functools.lru_cache(maxsize=None)
def _inputs():
    rng = np.random.default_rng(30)
    return {"abracadabra": b"abracadabra", "bytes256": rng.integers(0, 256, 30_000, dtype=np.uint8).tobytes(),
            "repeat200k": gen.repeat_dna(200_000, seed=7, lo=16, hi=2048).tobytes(), "a5000": b"A" * 5000,
            "fibonacci": _fibonacci_word(75_025), "repeat60k": gen.repeat_dna(60_000, seed=9, lo=16, hi=512).tobytes()}


def same_sections(got, want):
    for key in want:
        assert got[key] == want[key], key
    assert set(got) == set(want)


def check_records(native, records, literals, text, prefix=b""):
    """pack_factors == the model; unpack_factors and decode_packed give the records and the text back"""
    want = model.pack(records, literals)
    got = native.pack_factors(records, literals)
    same_sections(got, want)
    back, lit = native.unpack_factors(got)
    assert np.array_equal(back["start"], records["start"]) and np.array_equal(back["length"], records["length"])
    assert np.array_equal(back["ref"], records["ref"]) and lit == literals
    out, info = native.decode_packed_array(got, prefix)
    assert out.tobytes() == text
    assert info["n"] == len(text) and info["z"] == len(records) and info["n_literals"] == len(literals)
    return got


@pytest.mark.parametrize("name, with_rc", [("abracadabra", False), ("bytes256", False), ("repeat200k", False),
                                           ("a5000", False), ("fibonacci", False), ("repeat60k", True), ("repeat60k", False)])
def test_factorize_packed(native, name, with_rc):
    text = _inputs()[name]
    f = native.factorize_dna_w_rc_array(text) if with_rc else native.factorize_array(text)
    lit = native.literal_symbols(text, f)
    s = check_records(native, f, lit, text)
    same_sections(native.factorize_packed(text, with_rc=with_rc), s)
    assert s["first_start"] == 0 and s["decoded"] == len(text) and s["z"] == len(f)
    bare = native.factorize_packed(text, with_rc=with_rc, literals=False)
    same_sections(bare, dict(s, literal_mode=2, literals=b""))
    if with_rc:
        assert (f["ref"] >> np.uint64(63)).any(), "the input must exercise the other strand"
    if name == "bytes256":
        assert s["literal_mode"] == 0 and len(set(lit)) == 256
    if name in ("repeat200k", "repeat60k", "a5000"):
        assert s["literal_mode"] == 1


def test_factorize_packed_device(native):
    import torch
    text = _inputs()["repeat60k"]
    d = torch.frombuffer(bytearray(text), dtype=torch.uint8).cuda()
    torch.cuda.synchronize()
    for with_rc in (False, True):
        same_sections(native.factorize_packed_device(d.data_ptr(), len(text), with_rc=with_rc),
                      native.factorize_packed(text, with_rc=with_rc))


def test_lower_case_text_with_rc_packs_the_upper_cased_strand(native):
    text = _inputs()["repeat60k"][:5000]
    s = native.factorize_packed(text.lower(), with_rc=True)
    same_sections(s, native.factorize_packed(text, with_rc=True))
    assert native.decode_packed_array(s)[0].tobytes() == text
    with pytest.raises(RuntimeError, match="Invalid nucleotide"):
        native.factorize_packed(b"ACGTNACGT", with_rc=True)


def _seq(name):
    return b"".join(s for _, s in genomes.records(name))


def test_two_record_bacterial_fixture_with_rc(native):
    seqs = [s for _, s in genomes.records("test_bacterial_dna")]
    assert len(seqs) == 2
    S, orig, sent = native.prepare_multiple_dna_sequences_w_rc_bytes(seqs)
    f = native.factorize_multiple_dna_w_rc_array(S)
    n = int(f["start"][-1] + f["length"][-1])
    lit = native.literal_symbols(S, f)
    s = check_records(native, f, lit, S[:n])
    assert s["literal_mode"] == 0, "the sentinel between the records is a literal"
    assert (f["ref"] >> np.uint64(63)).any()


def test_multi_sequence_rc_string(native):
    rng = np.random.default_rng(5)
    a = gen.random_dna(3000, seed=51).tobytes()
    seqs = [a, genomes.revcomp(a[500:2500]) + gen.random_dna(700, seed=52).tobytes(), a[1000:1800] * 2,
            bytes(rng.choice(list(b"ACGT"), 33).astype(np.uint8))]
    S, orig, sent = native.prepare_multiple_dna_sequences_w_rc_bytes(seqs)
    f = native.factorize_multiple_dna_w_rc_array(S)
    n = int(f["start"][-1] + f["length"][-1])
    assert n == orig - 1
    check_records(native, f, native.literal_symbols(S, f), S[:n])


def test_t7_against_t3_needs_the_prefix(native):
    t3, t7 = _seq("T3"), _seq("T7")
    rows = native.factorize_w_reference(t3, t7)
    prefix = t3 + b"\x01"
    f = np.array(rows, dtype=model.FACTOR_DTYPE)
    s = check_records(native, f, native.literal_symbols(prefix + t7, f), prefix + t7, prefix)
    assert s["first_start"] == len(prefix) and s["decoded"] == len(t7)
    with pytest.raises(ValueError, match="first_start"):
        native.decode_packed_array(s)


def test_empty_text(native):
    for with_rc in (False, True):
        s = native.factorize_packed(b"", with_rc=with_rc)
        same_sections(s, model.pack(np.zeros(0, dtype=model.FACTOR_DTYPE), b""))
        records, literals = native.unpack_factors(s)
        assert len(records) == 0 and literals == b"" and native.decode_packed_array(s)[0].size == 0


def test_round_trip_through_a_file(native, tmp_path):
    import noLZSS
    import nolzss_amd
    text = _inputs()["repeat200k"]
    s = nolzss_amd.factorize_packed(text)
    path = tmp_path / "repeat.nolzfac"
    size = nolzss_amd.write_packed_factors(path, s)
    assert size == path.stat().st_size < 24 * s["z"] / 3
    back = noLZSS.read_packed_factors(path)
    assert back == s
    assert noLZSS.decode_packed(back) == text
    records, literals = nolzss_amd.unpack_factors(back)
    assert [tuple(int(v) for v in r) for r in records[:50]] == nolzss_amd.factorize(text)[:50]
    assert nolzss_amd.decode(records, literals) == text
    assert noLZSS.pack_factors(noLZSS.factorize(text), noLZSS.literal_symbols(text, noLZSS.factorize(text))) == s
    bare = noLZSS.factorize_packed(text, literals=False)
    nolzss_amd.write_packed_factors(path, bare)
    assert nolzss_amd.read_packed_factors(path) == bare and nolzss_amd.unpack_factors(bare)[1] is None
