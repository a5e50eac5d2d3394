"""GPU: every output form of the chain stage (chain.hip: mark_chain, then factor starts / records / lengths taken from
the mark) at the edges of the cursor's 4096-position tiles and from a non-zero start_pos -- the count-only,
device-only and starts-only forms, which leave nothing but a number to look at, next to the forms that deliver
records.  The yardstick is the CPU oracle (tests/oracle_lib.py), for relative LZ the brute-force parse
(tests/rlz_model.py); never the GPU alone."""
import numpy as np
import pytest

import gen
import oracle_lib as oracle
import rlz_model

TILE = 4096
SIZES = (1, 2, 4095, 4096, 4097, 8193, 12289)
FIELDS = ("start", "length", "ref")
RC_MASK = np.uint64(1 << 63)


def tile_jump_text() -> np.ndarray:
    """5 tiles + 1 of random bases; the 9000 bases from 3000 positions into the second tile are a copy of the start of
    the text (base by base: where source and destination overlap the copy repeats itself)"""
    t = gen.random_dna(5 * TILE + 1, seed=0xC4A1)
    dst = TILE + 3000
    for at in range(0, 9000, dst):
        ln = min(dst, 9000 - at)
        t[dst + at:dst + at + ln] = t[at:at + ln]
    return t


def jumps_a_tile(f) -> bool:
    """some factor begins in front of a tile and ends behind it: the chain never enters that tile"""
    first = f["start"].astype(np.int64) // TILE + 1  # the first tile that begins behind the factor's start
    return bool(np.any((first + 1) * TILE <= (f["start"] + f["length"]).astype(np.int64)))


def make_texts():
    texts = {f"n{n}": gen.repeat_dna(n, lo=8, hi=512) for n in SIZES}
    texts["jump"] = tile_jump_text()
    return {k: np.ascontiguousarray(v).tobytes() for k, v in texts.items()}


TEXTS = make_texts()
RC_NAMES = [k for k, t in TEXTS.items() if len(t) >= 2]


def start_positions(n):
    return sorted({sp for sp in (0, 1, TILE - 1, TILE, n - 1) if 0 <= sp < n})


@pytest.fixture(scope="module")
def plain_oracle():
    """name -> {start_pos: the oracle's records}, computed once"""
    return {k: {sp: oracle.factors_array(t, sp) for sp in start_positions(len(t))} for k, t in TEXTS.items()}


@pytest.fixture(scope="module")
def rc_oracle():
    return {k: oracle.factors_array_multiple_dna_w_rc(oracle.prepare_multiple_dna_w_rc([TEXTS[k]])[0]) for k in RC_NAMES}


def same(got, exp) -> bool:
    return len(got) == len(exp) and all(np.array_equal(got[f], exp[f]) for f in FIELDS)


def test_oracle_side_of_the_cases(plain_oracle):
    """No GPU: the texts are what the tests below take them for."""
    assert [len(TEXTS[f"n{n}"]) for n in SIZES] == list(SIZES)
    assert len(TEXTS["jump"]) == 5 * TILE + 1
    assert jumps_a_tile(plain_oracle["jump"][0])
    assert not jumps_a_tile(plain_oracle["n4096"][0])  # (one tile: nothing to jump)
    for k, by_sp in plain_oracle.items():
        for sp, f in by_sp.items():
            assert f["start"][0] == sp and int(f["length"].sum()) == len(TEXTS[k]) - sp, (k, sp)


@pytest.fixture(scope="module")
def native():
    from nolzss_amd import _noLZSS
    assert _noLZSS.device_count() >= 1, "no MI355X visible"
    return _noLZSS


@pytest.fixture(scope="module")
def device_texts(native):
    import torch
    d = {k: torch.from_numpy(np.frombuffer(t, dtype=np.uint8).copy()).cuda() for k, t in TEXTS.items()}
    torch.cuda.synchronize()
    return d


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(TEXTS))
def test_plain_forms(native, device_texts, plain_oracle, name):
    t, d = TEXTS[name], device_texts[name]
    n = len(t)
    assert name != "jump" or jumps_a_tile(plain_oracle[name][0])
    for sp, exp in plain_oracle[name].items():
        assert same(native.factorize_array(t, sp), exp), (name, sp)
        for emit in (0, 1, 2):
            z, got = native.factorize_device(d.data_ptr(), n, emit=emit, start_pos=sp)
            assert z == len(exp), (name, sp, emit, z, len(exp))
            assert (got is None) if emit < 2 else same(got, exp), (name, sp, emit)
    exp = plain_oracle[name][0]
    assert native.count_factors(t) == len(exp), name
    assert np.array_equal(native.factor_lengths(t).astype(np.uint64), exp["length"]), name
    h = native.factor_length_histogram(t)
    assert h["z"] == len(exp) and int(h["fwd"].sum() + h["rc"].sum()) + len(h["tail_lengths"]) == len(exp), name
    every = native.debug_position_factors(t)
    assert same(every[exp["start"].astype(np.int64)], exp), name


@pytest.mark.gpu
@pytest.mark.parametrize("name", RC_NAMES)
def test_reverse_complement_forms(native, device_texts, plain_oracle, rc_oracle, name):
    t, d, exp = TEXTS[name], device_texts[name], rc_oracle[name]
    n = len(t)
    assert same(native.factorize_dna_w_rc_array(t), exp), name
    assert native.count_factors_dna_w_rc(t) == len(exp), name
    for emit in (0, 1, 2):
        z, got = native.factorize_dna_w_rc_device(d.data_ptr(), n, emit=emit)
        assert z == len(exp), (name, emit, z, len(exp))
        assert (got is None) if emit < 2 else same(got, exp), (name, emit)
    assert np.array_equal(native.factor_lengths(t, with_rc=True).astype(np.uint64), exp["length"]), name
    assert native.count_factors_batch_both([t]) == ([len(exp)], [len(plain_oracle[name][0])]), name


@pytest.mark.gpu
@pytest.mark.parametrize("with_rc", [False, True])
def test_merged_batch(native, plain_oracle, rc_oracle, with_rc):
    names = ["n4097", "jump"]
    texts = [TEXTS[k] for k in names]
    exp = [rc_oracle[k] if with_rc else plain_oracle[k][0] for k in names]
    counts, arrays = native.factorize_batch(texts, want_factors=True, with_rc=with_rc)
    only_counts, none = native.factorize_batch(texts, want_factors=False, with_rc=with_rc)
    assert none is None and counts == only_counts == [len(e) for e in exp]
    one = native.factorize_dna_w_rc_array if with_rc else native.factorize_array
    for k, got, e, t in zip(names, arrays, exp, texts):
        assert same(got, one(t)) and same(got, e), k


@pytest.mark.gpu
@pytest.mark.parametrize("with_rc", [False, True])
def test_relative_lz(native, with_rc):
    ref, tgt = TEXTS["n8193"], TEXTS["jump"]
    exp = rlz_model.brute_absolute([ref], [tgt], with_rc)[0]
    full = native.rlz_factorize_arrays([ref], [tgt], with_rc=with_rc, want_factors=True)
    count = native.rlz_factorize_arrays([ref], [tgt], with_rc=with_rc, want_factors=False)
    assert count["factors"] is None and full["counts"] == count["counts"] == [len(exp)]
    with native.RlzIndexHandle.open([ref], with_rc=with_rc) as index:
        ifull = index.factorize_arrays([tgt], want_factors=True)
        icount = index.factorize_arrays([tgt], want_factors=False)
    assert icount["factors"] is None and ifull["counts"] == icount["counts"] == [len(exp)]
    assert same(full["factors"][0], ifull["factors"][0]) and same(full["factors"][0], exp)
