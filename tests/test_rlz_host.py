"""Relative LZ without a GPU: the layout of the prepared string against a Python restatement, every refusal of the
entry points, the split / rebasing / summary functions on hand-made records, and the array formulation (tests/rlz_model)
against the brute force of the definition."""
import ctypes as C
import random

import numpy as np
import pytest

import rlz_model as model
from nolzss_amd import _lib
from nolzss_amd import _noLZSS as native
from nolzss_amd.genomics import rlz

RC_MASK = 1 << 63


def _dna(rng, n, alphabet=b"ACGT"):
    return bytes(rng.choice(alphabet) for _ in range(n))


# ---- the layout --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_rc", [True, False])
@pytest.mark.parametrize("m", [1, 3])
@pytest.mark.parametrize("k", [0, 1, 5])
def test_prepare_matches_the_python_layout(m, k, with_rc):
    rng = random.Random(100 * m + 10 * k + with_rc)
    for trial in range(6):  # both parities of B - 1 + E come up
        refs = [_dna(rng, rng.randint(1, 9)) for _ in range(m)]
        targets = [_dna(rng, rng.choice([0, 0, 1, 4, 7])) for _ in range(k)]
        if trial % 2:
            refs[0] = refs[0].lower()
            targets = [t.lower() if j % 2 else t for j, t in enumerate(targets)]
        got = native.rlz_prepare(refs, targets, with_rc=with_rc)
        exp = model.layout(refs, targets, with_rc)
        assert got["S"] == exp["S"]
        assert got["target_offsets"] == exp["target_offsets"]
        assert got["block_length"] == exp["block_length"] == sum(map(len, refs)) + m - 1
        assert got["rc_block_start"] == exp["rc_block_start"]
        assert got["rcN"] == exp["rcN"]
        S, B, E = got["S"], got["block_length"], got["rc_block_start"]
        sentinels = [c for c in S if c not in b"ACGT"]
        assert len(sentinels) == len(set(sentinels)), "sentinels must be unique"
        assert S[:B] == model.layout(refs, [], False)["S"][:B]
        if with_rc:
            assert (B - 1 + E) % 2 == 0 and got["rcN"] == (B - 1 + E) // 2
            after_targets = B + 1 + sum(map(len, targets)) + k
            assert E - after_targets == (B - 1 + after_targets) % 2, "a pad exactly when the parity needs it"
            assert len(S) == E + B + 1
            # the exact mirror: position E + j holds the complement of Rblk[B - 1 - j], separators on separators
            for j in range(B):
                a, b = S[B - 1 - j], S[E + j]
                if a in b"ACGT":
                    assert bytes([b]) == model.revcomp(bytes([a]))
                else:
                    assert b not in b"ACGT"
        else:
            assert E == len(S) == B + 1 + sum(map(len, targets)) + k and got["rcN"] == 0
        for t, off in zip(targets, got["target_offsets"]):
            assert S[off:off + len(t)] == t.upper()
            assert S[off + len(t)] not in b"ACGT"


def test_sentinels_follow_the_library_sequence():
    got = native.rlz_prepare([b"AC", b"GT"], [b"A", b"", b"C"], with_rc=True)["S"]
    sent = [c for c in got if c not in b"ACGT"]
    assert sent == model.SENTINELS[:len(sent)]


# ---- refusals ----------------------------------------------------------------------------------------------------
def test_no_reference_is_refused():
    with pytest.raises(ValueError, match="at least one reference"):
        native.rlz_prepare([], [b"ACGT"])
    with pytest.raises(ValueError, match="at least one reference"):
        native.rlz_factorize_arrays([], [b"ACGT"])
    for refs in ([b""], [b"", b""]):
        with pytest.raises(ValueError, match="reference block is empty"):
            native.rlz_prepare(refs, [b"ACGT"])
        with pytest.raises(ValueError, match="reference block is empty"):
            native.rlz_factorize_arrays(refs, [b"ACGT"])


@pytest.mark.parametrize("with_rc, m, k_ok", [(True, 1, 247), (True, 3, 243), (False, 1, 249), (False, 3, 247)])
def test_sentinel_limit_at_the_boundary_and_one_over(with_rc, m, k_ok):
    refs = [b"ACGT"] * m
    assert (2 * m + k_ok + 1 if with_rc else m + k_ok) == 250
    got = native.rlz_prepare(refs, [b"A"] * k_ok, with_rc=with_rc)
    sent = [c for c in got["S"] if c not in b"ACGT"]
    assert len(sent) == len(set(sent)) and len(sent) in (250, 249)  # (249: no pad was needed)
    with pytest.raises(ValueError, match="Too many sequences"):
        native.rlz_prepare(refs, [b"A"] * (k_ok + 1), with_rc=with_rc)
    with pytest.raises(ValueError, match="Too many sequences"):
        native.rlz_factorize_arrays(refs, [b"A"] * (k_ok + 1), with_rc=with_rc)


@pytest.mark.parametrize("with_rc", [True, False])
def test_too_long_is_refused_before_any_byte_is_read(with_rc):
    # the lengths alone decide: 2^31 reference bases mirror to more than the 32-bit pipeline takes, and without the
    # mirror 2^32 do; the buffers behind the pointers are 4 bytes long and are never read
    lib = _lib.lib
    refs = (C.c_char_p * 1)(b"ACGT")
    tgts = (C.c_char_p * 1)(b"ACGT")
    ref_lens = (C.c_size_t * 1)(1 << (31 if with_rc else 32))
    tgt_lens = (C.c_size_t * 1)(4)
    S, off = C.c_void_p(), C.c_void_p()
    n, B, E, rcN = C.c_size_t(), C.c_size_t(), C.c_size_t(), C.c_size_t()
    rc = lib.nolzss_rlz_prepare(refs, ref_lens, 1, tgts, tgt_lens, 1, int(with_rc), C.byref(S), C.byref(n), C.byref(off),
                                C.byref(B), C.byref(E), C.byref(rcN))
    assert rc == _lib.ERR_INVALID_ARGUMENT
    assert b"text too long" in lib.nolzss_last_error()
    res = _lib.RlzResult()
    rc = lib.nolzss_rlz_factorize(refs, ref_lens, 1, tgts, tgt_lens, 1, int(with_rc), 1, 0, C.byref(res))
    assert rc == _lib.ERR_INVALID_ARGUMENT
    assert b"text too long" in lib.nolzss_last_error()


def test_invalid_nucleotide_counts_references_first():
    with pytest.raises(RuntimeError, match="Invalid nucleotide 'N' found in sequence 1"):
        native.rlz_prepare([b"ACGT", b"ACNT"], [b"ACGT"])
    with pytest.raises(RuntimeError, match="Invalid nucleotide 'x' found in sequence 4"):
        native.rlz_prepare([b"ACGT", b"ACGT"], [b"ACGT", b"", b"ACxT"], with_rc=False)
    with pytest.raises(RuntimeError, match="Invalid nucleotide 'N' found in sequence 2"):
        native.rlz_factorize_arrays([b"ACGT", b"ACGT"], [b"NACGT"])
    with pytest.raises(RuntimeError, match="Invalid nucleotide 'N' found in sequence 2"):
        native.debug_rlz_codes([b"ACGT", b"ACGT"], [b"NACGT"])


def test_no_targets_is_an_empty_result_without_a_device():
    for want in (True, False):
        res = native.rlz_factorize_arrays([b"ACGT", b"GGA"], [], want_factors=want)
        assert res["counts"] == [] and res["target_offsets"] == [] and res["block_length"] == 8
        assert res["factors"] == ([] if want else None)
    assert rlz.rlz_factorize(b"ACGT", []) == []
    assert rlz.rlz_count_factors(b"ACGT", []) == []
    assert len(native.debug_rlz_codes(b"ACGT", [])) == 0


# ---- split, rebasing, summary --------------------------------------------------------------------------------------
def _records(rows):
    return np.array(rows, dtype=native.FACTOR_DTYPE)


def test_split_and_rebase_on_hand_made_records():
    # block of 10 (positions 0..9), sentinel at 10, target 0 at 11..16, sentinel 17, an empty target at 18, sentinel
    # 18, target 2 at 19..22, sentinel 23
    offsets, lengths = [11, 18, 19], [6, 0, 4]
    recs = _records([
        (11, 3, 2),                # forward match
        (14, 1, 14),               # literal: ref == start
        (15, 1, 7),                # a match of length 1: ref < block
        (16, 1, RC_MASK | 4),      # a reverse-complement match of length 1
        (17, 1, 17), (18, 1, 18),  # the sentinels between the targets
        (19, 4, RC_MASK | 0),      # reverse-complement match at reference position 0
    ])
    per = rlz.split_and_rebase(recs, offsets, lengths)
    assert [len(p) for p in per] == [4, 0, 1]
    a = per[0]
    assert a["start"].tolist() == [0, 3, 4, 5] and a["length"].tolist() == [3, 1, 1, 1]
    assert a["ref"].tolist() == [2, 0, 7, 4]
    assert a["is_literal"].tolist() == [False, True, False, False]
    assert a["is_rc"].tolist() == [False, False, False, True]
    c = per[2]
    assert c["start"].tolist() == [0] and c["length"].tolist() == [4] and c["ref"].tolist() == [0]
    assert c["is_rc"].tolist() == [True] and c["is_literal"].tolist() == [False]
    assert per[1].dtype == rlz.RLZ_DTYPE and len(per[1]) == 0

    summary = rlz.rlz_summary(per)
    assert summary[0] == {"factors": 4, "forward_bases": 4, "rc_bases": 1, "literal_bases": 1}
    assert summary[1] == {"factors": 0, "forward_bases": 0, "rc_bases": 0, "literal_bases": 0}
    assert summary[2] == {"factors": 1, "forward_bases": 0, "rc_bases": 4, "literal_bases": 0}


def test_rebase_of_one_target_equals_the_split():
    recs = _records([(21, 2, 0), (23, 1, 23), (24, 5, RC_MASK | 3)])
    one = rlz.rebase(recs, 21)
    assert np.array_equal(one, rlz.split_and_rebase(recs, [21], [8])[0])
    assert one["start"].tolist() == [0, 2, 3]


# ---- the array formulation against the definition --------------------------------------------------------------------
def _case(rng):
    m, k = rng.randint(1, 3), rng.randint(1, 4)
    alphabet = rng.choice([b"ACGT", b"ACGT", b"AC", b"AT"])  # A/T: reverse complements everywhere
    refs = [_dna(rng, rng.randint(1, 14), alphabet) for _ in range(m)]
    block = b"".join(refs)
    targets = []
    for _ in range(k):
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
def test_array_model_matches_the_brute_force(with_rc):
    rng = random.Random(20260 + with_rc)
    for _ in range(100):  # (two modes: 200 cases)
        refs, targets = _case(rng)
        lay = native.rlz_prepare(refs, targets, with_rc=with_rc)
        S, B, E = lay["S"], lay["block_length"], lay["rc_block_start"]
        chain_end = lay["target_offsets"][-1] + len(targets[-1])
        sa, lcp = model.python_sa_lcp(S)
        code = model.array_codes(sa, lcp, B, E, with_rc)
        recs = model.array_records(sa, lcp, code, B, chain_end, lay["rcN"])
        exp = model.brute_absolute(refs, targets, with_rc)
        for j, (t, off) in enumerate(zip(targets, lay["target_offsets"])):
            got = model.records_of_target(recs, off, len(t))
            assert np.array_equal(got, exp[j]), (refs, targets, j)
        # everything outside the targets is a sentinel literal
        inside = sum(len(e) for e in exp)
        assert len(recs) - inside == len(targets) - 1
