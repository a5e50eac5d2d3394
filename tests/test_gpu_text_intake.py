"""The front of the pipeline (text_pack.hip) on the edges of its decisions and at every alignment of the text.

Alphabet and classification: the texts of text_intake_cases.py, one child process with NOLZSS_TRACE=1 for all of them.  The
trace names the plan and the key width of every text -- "segmented" or "general" on 17, 15 or 7 symbols, that is 2, 4 or
8 bits --, which proves the decision; suffix array, inverse, LCP, L* and factors are compared with the oracle by integer
equality (a segmented text whose once-only bytes are not in the device's order: the ordering rule of rc_positions.py in place
of suffix-array equality).

Alignment: presence_kernel, find_terminators_kernel and pack_kernel have a 16-byte-aligned vector branch and a byte branch,
with head and tail pieces; the *_device entry points take any device address.  The text is placed at the offsets 0 .. 16 of
a buffer filled with a poison byte that is not in its alphabet: one poison byte read changes sigma, or the segmented
decision, and with it the result.  Expected: the oracle, at every offset."""
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

import key_layout_cases as K
import oracle_lib as oracle
import text_intake_cases as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALIGN_LENGTHS = (1, 15, 16, 17, 31, 4097, 65537)
OFFSETS = range(17)


def test_cases_get_the_decision_they_are_named_for():
    """(no GPU) text_pack.hip's rules restated in numpy (key_layout_cases.classify) agree with the case table"""
    names = set()
    for name, t, bits, segmented in T.cases():
        sigma, got_bits, got_seg = K.classify(t)
        assert (got_bits, got_seg) == (bits, segmented), (name, sigma, got_bits, got_seg)
        names.add(name)
        assert len(t) <= 300_000
    a = np.frombuffer(dict((c[0], c[1]) for c in T.cases())["one_other_value_70000_times"], dtype=np.uint8)
    assert int((a == ord("N")).sum()) == 70_000
    assert {f"sigma_{s}" for s in (1, 2, 3, 4, 5, 15, 16, 17, 255, 256)} <= names
    for n in T.LENGTHS:
        assert f"two_bit_{n}" in names and (n < 15 or f"four_bit_{n}" in names) and (n < 17 or f"eight_bit_{n}" in names)


@pytest.mark.gpu
def test_alphabet_and_classification_edges(tmp_path):
    cases = T.as_layout_cases()
    path = tmp_path / "expected.pickle"
    with open(path, "wb") as f:
        pickle.dump([K.expected_of(c) for c in cases], f)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "text_intake_cases.py"), str(path)], cwd=ROOT,
                       env=dict(os.environ, NOLZSS_TRACE="1"), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and f"ok {len(cases)}" in r.stdout, r.stdout[-2000:] + r.stderr[-6000:]
    trace = K.split_trace(r.stderr)
    for i, case in enumerate(cases):
        keys = K.TRACE_KEY.findall(trace[i])
        want = {(len(case.data), case.lay.k_syms, case.plan)}
        assert keys and {(int(n), int(ks), plan) for n, _, ks, plan in keys} == want, (case.name, keys, want)
        # the terminator table of a segmented text: the tied count is the model's only if every once-only byte cut the text
        codes, lim = K.text_view(case.data)
        model = K.tied_after_key_sort(codes, lim, case.lay.bits, case.lay.k_syms)
        assert all(int(m) == model for _, m, _, _ in keys), (case.name, keys, model)


# ---- alignment -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def native():
    from nolzss_amd import _noLZSS
    assert _noLZSS.device_count() >= 1, "no MI355X visible"
    return _noLZSS


def _texts(n):
    """kind -> (text, poison byte): a 2-bit, a 4-bit, an 8-bit and a segmented text of n bytes (as far as n allows)"""
    out = {"two_bit": (T.over(b"ACGT", n, 60 + n), ord("N")), "four_bit": (T.over(b"ACGNT", n, 61 + n), ord("#")),
           "eight_bit": (T.over(bytes(range(97, 114)), n, 62 + n), ord("#"))}
    if n >= 15:
        out["segmented"] = (T.dna_with(n, 63 + n, b"#\x01", at=[n // 2, n - 1]), ord("N"))
    return out


def _placed(torch, t, poison, offset):
    """the text at `offset` of a buffer of len(t) + 64 poison bytes -> (tensor, address of the text)"""
    buf = np.full(len(t) + 64, poison, dtype=np.uint8)
    buf[offset:offset + len(t)] = np.frombuffer(t, dtype=np.uint8)
    d = torch.from_numpy(buf).cuda()
    torch.cuda.synchronize()
    assert d.data_ptr() % 16 == 0
    return d, d[offset:].data_ptr()


def _same(got, exp):
    return len(got) == len(exp) and all(np.array_equal(np.asarray(got[k]), np.asarray(exp[k])) for k in ("start", "length", "ref"))


@pytest.mark.gpu
@pytest.mark.parametrize("n", ALIGN_LENGTHS)
def test_every_alignment_single_text(native, n):
    """factorize_device (records built on the device, and downloaded), factorize_dna_w_rc_device and roundtrip_device"""
    import torch
    for kind, (t, poison) in _texts(n).items():
        assert poison not in t
        exp = oracle.factors_array(t)
        rc = kind == "two_bit"
        if rc:
            exp_rc = oracle.factors_array_multiple_dna_w_rc(oracle.prepare_multiple_dna_w_rc([t])[0])
        for o in OFFSETS:
            d, p = _placed(torch, t, poison, o)
            assert p % 16 == o % 16
            z, none = native.factorize_device(p, n, emit=1)
            assert (z, none) == (len(exp), None), (kind, o, z, len(exp))
            z, got = native.factorize_device(p, n, emit=2)
            assert z == len(exp) and _same(got, exp), (kind, o)
            res = native.roundtrip_device(p, n, with_rc=False)
            assert (res["z"], res["mismatches"], res["first_mismatch"]) == (len(exp), 0, None), (kind, o, res)
            if rc:
                z, got = native.factorize_dna_w_rc_device(p, n, emit=2)
                assert z == len(exp_rc) and _same(got, exp_rc), (kind, o, "reverse complement")
                res = native.roundtrip_device(p, n, with_rc=True)
                assert (res["z"], res["mismatches"], res["first_mismatch"]) == (len(exp_rc), 0, None), (kind, o, res)
            del d


@pytest.mark.gpu
def test_every_alignment_batch(native):
    """factorize_batch_device with every record at another residue modulo 16: once merged into runs of independent
    sequences, once with a record over another alphabet, which sends the whole batch through one run per record"""
    import torch
    recs = [T.over(b"ACGT", n, 70 + j) for j, n in enumerate(ALIGN_LENGTHS + (2, 3, 14, 18, 33, 64, 255, 1000, 4096, 5000))]
    assert len(recs) == 17
    for extra in ([], [T.over(b"ACGNT", 777, 90)]):
        batch = recs + extra
        buf, at, pos = [], [], 0
        for j, r in enumerate(batch):
            pad = (j - pos) % 16 + 16  # record j starts at residue j modulo 16, poison in front of it
            buf.append(b"N" * pad if not extra else b"#" * pad)
            pos += pad
            at.append(pos)
            buf.append(r)
            pos += len(r)
        buf.append((b"N" if not extra else b"#") * 64)
        d = torch.from_numpy(np.frombuffer(b"".join(buf), dtype=np.uint8).copy()).cuda()
        torch.cuda.synchronize()
        assert d.data_ptr() % 16 == 0 and [a % 16 for a in at[:17]] == list(range(16)) + [0]
        want = [oracle.count_factors(r) for r in batch]
        for emit in (0, 1):
            m0, s0 = native.debug_batch_counters()
            got = native.factorize_batch_device([d.data_ptr() + a for a in at], [len(r) for r in batch], emit=emit)
            m1, s1 = native.debug_batch_counters()
            assert got == want, (emit, bool(extra))
            assert (m1 - m0, s1 - s0) == ((0, len(batch)) if extra else (len(batch), 0)), (m1 - m0, s1 - s0)
