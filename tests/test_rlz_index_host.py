"""The relative-LZ index without a GPU: the search formulation (tests/rlz_index_model) against the brute force of the
definition, the batch plan of RlzIndex, and every refusal of nolzss_rlz_index_open that is decided on the host."""
import ctypes as C
import random

import pytest

import rlz_index_model as index_model
import rlz_model as model
from nolzss_amd import _lib
from nolzss_amd import _noLZSS as native
from nolzss_amd.genomics import rlz


def _dna(rng, n, alphabet=b"ACGT"):
    return bytes(rng.choice(alphabet) for _ in range(n))


def _case(rng):
    """1 to 3 reference records (empty ones among them, never all), targets assembled from reference pieces,
    reverse-complemented pieces and random bases, empty targets among them"""
    alphabet = rng.choice([b"AC", b"ACG", b"ACGT"])
    m = rng.randint(1, 3)
    refs = [_dna(rng, rng.choice([0, 1, 3, 8, 14]), alphabet) for _ in range(m)]
    if not any(refs):
        refs[rng.randrange(m)] = _dna(rng, rng.randint(1, 14), alphabet)
    block = b"".join(refs)
    targets = []
    for _ in range(rng.randint(1, 3)):
        t = b""
        for _ in range(rng.randint(0, 4)):
            kind = rng.random()
            a = rng.randrange(len(block))
            piece = block[a:a + rng.randint(1, 9)]
            if kind < 0.4:
                t += piece
            elif kind < 0.7:
                t += model.revcomp(piece)
            else:
                t += _dna(rng, rng.randint(1, 4))
        targets.append(t)
    return refs, targets


@pytest.mark.parametrize("with_rc", [True, False])
def test_index_model_matches_the_brute_force(with_rc):
    rng = random.Random(31337 + with_rc)
    for _ in range(300):  # (two modes: 600 cases)
        refs, targets = _case(rng)
        ix = index_model.IndexModel(refs, with_rc)
        for t in targets:
            assert ix.codes(t) == model.brute_codes(refs, t, with_rc).tolist(), (refs, t)
            assert ix.parse(t) == model.brute_parse(refs, t, with_rc), (refs, t)


# ---- the batch plan ----------------------------------------------------------------------------------------------
def test_plan_closes_a_batch_exactly_at_the_limit():
    # block of 10: a batch of k targets with s bases takes 10 + 1 + s + k positions
    assert rlz.plan_index_batches([5, 5], 10, limit=23) == [(0, 2)]       # 11 + 10 + 2 = 23: still one batch
    assert rlz.plan_index_batches([5, 5], 10, limit=22) == [(0, 1), (1, 2)]
    assert rlz.plan_index_batches([5, 5, 5], 10, limit=23) == [(0, 2), (2, 3)]
    assert rlz.plan_index_batches([], 10, limit=23) == []


def test_plan_keeps_empty_targets_and_the_order():
    lengths = [0, 3, 0, 0, 4, 1, 0]
    plan = rlz.plan_index_batches(lengths, 10, limit=18)  # 11 + bases + k <= 18
    assert plan[0][0] == 0 and plan[-1][1] == len(lengths)
    assert all(a[1] == b[0] for a, b in zip(plan, plan[1:])) and all(lo < hi for lo, hi in plan)
    for lo, hi in plan:
        assert 11 + sum(lengths[lo:hi]) + (hi - lo) <= 18
    for (lo, hi), nxt in zip(plan, plan[1:]):  # greedy: the next target would not have fitted
        assert 11 + sum(lengths[lo:hi + 1]) + (hi + 1 - lo) > 18
    assert plan == [(0, 4), (4, 6), (6, 7)]


def test_plan_gives_an_overlong_target_a_batch_of_its_own():
    assert rlz.plan_index_batches([2, 100, 2], 10, limit=30) == [(0, 1), (1, 2), (2, 3)]
    assert rlz.plan_index_batches([100], 10, limit=30) == [(0, 1)]


def test_plan_batch_bases():
    assert rlz.plan_index_batches([4, 4, 4, 9, 1], 10, batch_bases=8) == [(0, 2), (2, 3), (3, 4), (4, 5)]
    assert rlz.plan_index_batches([4, 4, 4], 10, batch_bases=None) == [(0, 3)]
    assert rlz.plan_index_batches([1] * 5, 10) == [(0, 5)]
    assert rlz.MAX_TEXT == 0xffffffff - (1 << 19)


# ---- refusals that need no device --------------------------------------------------------------------------------
def test_symbols_are_exported():
    for name in ("nolzss_rlz_index_open", "nolzss_rlz_index_open_fasta", "nolzss_rlz_index_info",
                 "nolzss_rlz_index_factorize", "nolzss_rlz_index_codes", "nolzss_rlz_index_close"):
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(_lib.lib, name)


def test_open_without_a_reference_is_refused():
    with pytest.raises(ValueError, match="at least one reference"):
        native.RlzIndexHandle.open([])
    for refs in ([b""], [b"", b""]):
        with pytest.raises(ValueError, match="reference block is empty"):
            native.RlzIndexHandle.open(refs)
    with pytest.raises(ValueError, match="at least one reference"):
        rlz.RlzIndex.build([])


@pytest.mark.parametrize("with_rc, m_over", [(True, 125), (False, 251)])
def test_open_with_too_many_references_is_refused(with_rc, m_over):
    assert (2 * m_over + 1 if with_rc else m_over) > 250 >= (2 * (m_over - 1) + 1 if with_rc else m_over - 1)
    with pytest.raises(ValueError, match="Too many sequences"):
        native.RlzIndexHandle.open([b"ACGT"] * m_over, with_rc=with_rc)


def test_open_refuses_an_invalid_base_before_any_device_is_touched():
    with pytest.raises(RuntimeError, match="Invalid nucleotide 'N' found in sequence 1"):
        native.RlzIndexHandle.open([b"ACGT", b"ACNT"])
    with pytest.raises(RuntimeError, match="Invalid nucleotide 'x' found in sequence 0"):
        native.RlzIndexHandle.open(b"ACxT", with_rc=False)


def test_open_refuses_a_prefix_beyond_twelve_and_a_too_long_block():
    with pytest.raises(ValueError, match="prefix_syms"):
        native.RlzIndexHandle.open(b"ACGT", prefix_syms=13)
    # the lengths alone decide; the 4 bytes behind the pointer are never read
    refs, lens, h = (C.c_char_p * 1)(b"ACGT"), (C.c_size_t * 1)(1 << 31), C.c_void_p()
    assert _lib.lib.nolzss_rlz_index_open(refs, lens, 1, 1, 0, 0, C.byref(h)) == _lib.ERR_INVALID_ARGUMENT
    assert b"text too long" in _lib.lib.nolzss_last_error() and not h.value


def test_null_handles_are_refused_and_close_of_null_is_a_no_op():
    lib = _lib.lib
    assert lib.nolzss_rlz_index_close(None) == _lib.OK
    info, res = _lib.RlzIndexSummary(), _lib.RlzResult()
    assert lib.nolzss_rlz_index_info(None, C.byref(info)) == _lib.ERR_INVALID_ARGUMENT
    tg, ln = (C.c_char_p * 1)(b"ACGT"), (C.c_size_t * 1)(4)
    assert lib.nolzss_rlz_index_factorize(None, tg, ln, 1, 1, C.byref(res)) == _lib.ERR_INVALID_ARGUMENT


def test_open_on_valid_input_needs_a_device():
    if native.device_count() == 0:
        with pytest.raises(RuntimeError, match="no HIP device"):
            native.RlzIndexHandle.open([b"ACGT", b"GGA"])
        with pytest.raises(RuntimeError, match="no HIP device"):
            rlz.RlzIndex.build(b"ACGTACGT", with_rc=False)
    else:
        with native.RlzIndexHandle.open([b"ACGT", b"GGA"]) as h:
            assert h.info["block_length"] == 8 and h.info["num_references"] == 2
