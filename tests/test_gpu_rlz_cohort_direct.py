"""The pack-from-bytes, pair, site and column kernels of a cohort (rlz_cohort.hip) driven through add_calls on samples
made here, against tests/rlz_cohort_model.py by integer and byte equality: every block length around a word and a
staging turn, every cohort size around a tile of 64 samples, one slice and many, and the shapes of input that single out
one term of the counting."""
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import rlz_cohort_model as hm

pytestmark = pytest.mark.gpu

@pytest.fixture(scope="module")
def rlz():
    from nolzss_amd import _noLZSS
    assert _noLZSS.device_count() >= 1, "no MI355X visible"
    from nolzss_amd.genomics import rlz
    return rlz


def dna(rng, n, alphabet=b"ACGT"):
    return bytes(rng.choice(alphabet) for _ in range(n))


def sample_of(rng, block, alphabet=b"ACGT", missing=0.3, lower=False):
    """one byte per block position: a letter of the alphabet, or with probability `missing` a byte that is no call"""
    out = bytearray(rng.choice(b"N-.*\x00n") if rng.random() < missing else rng.choice(alphabet) for _ in range(len(block)))
    return bytes(out).lower() if lower else bytes(out)


def site_rows(found):
    return [(int(r["position"]), int(r["record_offset"]), int(r["record"]), int(r["present"]), tuple(int(v) for v in r["counts"]),
             int(r["reference"])) for r in found]


def same_everything(co, refs, samples, rlz, site_rules=None):
    """infos, calls, both matrices, sites under the rules and an alignment against the model -> the model's calls"""
    block = b"\x01".join(bytes(r).upper() for r in refs)
    raw = [hm.raw_calls_from_bytes(s, block) for s in samples]
    calls = [hm.letters(r) for r in raw]
    n = len(samples)
    assert co.info["samples"] == n == len(co) and co.info["block_length"] == len(block)
    assert co.samples() == [dict(hm.infos(r, block), sample=s, id=None) for s, r in enumerate(raw)]
    for s in range(n):
        assert co.calls(s) == calls[s], s
    diff, comp = hm.distances(calls)
    got = co.distances()
    assert got["differences"].dtype == got["compared"].dtype == np.uint32 and got["differences"].shape == (n, n)
    assert got["differences"].tolist() == diff, np.argwhere(got["differences"] != np.array(diff))[:5].tolist()
    assert got["compared"].tolist() == comp, np.argwhere(got["compared"] != np.array(comp))[:5].tolist()
    assert got["called"].tolist() == [comp[s][s] for s in range(n)]
    assert got["to_reference"].tolist() == [hm.infos(r, block)["differs"] for r in raw]
    starts = hm.record_starts(block)
    for min_present, with_reference in site_rules or ((0, True), (n, True), (n + 1, True), (max(n // 2, 1), False)):
        found = co.sites(min_present, with_reference)
        assert found.dtype == rlz.COHORT_SITE_DTYPE
        assert site_rows(found) == hm.sites(calls, block, starts, min_present, with_reference), (min_present, with_reference)
    positions, letters = co.alignment()
    core = [r[0] for r in hm.sites(calls, block, starts, n, True)]
    assert positions.tolist() == core and letters.shape == (n, len(core)) and letters.dtype == np.uint8
    assert [bytes(row) for row in letters] == hm.columns(calls, core)
    return calls


@pytest.mark.parametrize("B", (1, 63, 64, 65, 127, 128, 129, 4095, 4096, 4097))
def test_block_lengths_around_a_word_and_a_staging_turn(rlz, B):
    """W = 1, 2, 3 words and 64, 65 words: the last word partly filled, one slice of 64 words and a second one of one"""
    rng = random.Random(B)
    ref = dna(rng, B)
    samples = [sample_of(rng, ref), sample_of(rng, ref, b"AC"), sample_of(rng, ref, lower=True)]
    spots = sorted({63, 64, B - 1})
    if B >= 65:  # two samples that differ exactly at 63 and 64, and at B - 1
        base, twin = bytearray(samples[0]), bytearray(samples[0])
        for p in spots:
            base[p], twin[p] = ord("A"), ord("C")
        samples[0] = bytes(base)
        samples.append(bytes(twin))
    with rlz.RlzIndex.build([ref]) as ix, ix.cohort() as co:
        for s in samples:
            co.add_calls(s)
        same_everything(co, [ref], samples, rlz)
        if B >= 65:
            got = co.distances()
            assert got["differences"][0, 3] == len(spots) == got["differences"][3, 0]
            assert got["compared"][0, 3] == got["called"][0] == got["called"][3]
            assert co.alignment(spots)[1][[0, 3]].tolist() == [[65] * len(spots), [67] * len(spots)]


@pytest.mark.parametrize("N", (1, 2, 3, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 130))
def test_cohort_sizes_around_a_tile(rlz, N):
    """one tile partly filled, exactly filled, two and three tiles per side; the thread map's 16-sample steps"""
    rng = random.Random(N)
    B = 130 if N <= 65 else 70  # (three words, the last holding two bits; two words for the large cohorts)
    ref = dna(rng, B)
    samples = [sample_of(rng, ref, (b"ACGT", b"AG", b"T")[s % 3]) for s in range(N)]
    with rlz.RlzIndex.build([ref]) as ix, ix.cohort() as co:
        for s in samples:
            co.add_calls(s)
        assert co.info["capacity"] >= N and co.info["device_bytes"] == co.info["capacity"] * 24 * ((B + 63) // 64)
        same_everything(co, [ref], samples, rlz, site_rules=((0, True), (N, False)))


def test_slices_of_one_three_and_seven_words_against_the_default(rlz, monkeypatch):
    B = (1 << 17) + 1
    rng = random.Random(17)
    ref = dna(rng, B)
    arr = np.frombuffer(ref, dtype=np.uint8)
    samples = []
    for s in range(5):  # the reference mutated at 1 % and 10 % no-calls, drawn with numpy: the model runs once
        draw = np.random.default_rng(s)
        mine = arr.copy()
        hit = draw.random(B) < 0.01
        mine[hit] = np.frombuffer(b"ACGT", dtype=np.uint8)[draw.integers(0, 4, int(hit.sum()))]
        mine[draw.random(B) < 0.1] = ord("N")
        samples.append(mine.tobytes())
    with rlz.RlzIndex.build([ref]) as ix, ix.cohort() as co:
        for s in samples:
            co.add_calls(s)
        whole = co.distances()  # the default: 33 slices of 64 words (atomic adds)
        diff, comp = hm.distances([hm.calls_from_bytes(s, ref) for s in samples])
        assert whole["differences"].tolist() == diff and whole["compared"].tolist() == comp
        for words in ("1", "3", "7", "100000"):  # (the last: one slice over all words, plain stores)
            monkeypatch.setenv("NOLZSS_RLZ_COHORT_SLICE", words)  # the knob is read on every call
            got = co.distances()
            assert np.array_equal(got["differences"], whole["differences"]) and np.array_equal(got["compared"], whole["compared"]), words
        monkeypatch.delenv("NOLZSS_RLZ_COHORT_SLICE")


def test_shapes_that_single_out_one_term(rlz):
    rng = random.Random(5)
    B = 200
    ref = dna(rng, B)
    one = sample_of(rng, ref, missing=0.0)
    evens = bytes(c if p % 2 == 0 else ord("N") for p, c in enumerate(one))
    odds = bytes(c if p % 2 else ord("N") for p, c in enumerate(one))
    samples = [one, one, one.lower(), b"N" * B, evens, odds, b"\x00" * B]
    with rlz.RlzIndex.build([ref]) as ix, ix.cohort() as co:
        for s in samples:
            co.add_calls(s)
        same_everything(co, [ref], samples, rlz)
        got = co.distances()
        assert not got["differences"][:3, :3].any() and (got["compared"][:3, :3] == B).all()  # identical samples, either case
        assert not got["compared"][3].any() and not got["compared"][:, 6].any()                # not a single call
        assert got["compared"][4, 5] == 0 == got["differences"][4, 5]                         # disjoint ok masks
        assert got["compared"][4, 0] == B // 2 and got["called"].tolist() == [B, B, B, 0, B // 2, B // 2, 0]
    # identical samples alone: a zero matrix, and no site without the reference
    with rlz.RlzIndex.build([ref]) as ix, ix.cohort() as co:
        for _ in range(3):
            co.add_calls(one)
        assert not co.distances()["differences"].any()
        assert len(co.sites(0, False)) == 0 and len(co.alignment(with_reference=False)[0]) == 0
        assert co.alignment(with_reference=False)[1].shape == (3, 0)


def test_separators_of_a_three_record_block_are_never_counted(rlz):
    rng = random.Random(9)
    refs = [dna(rng, 70), dna(rng, 1), dna(rng, 60)]
    block = b"\x01".join(refs)
    samples = [sample_of(rng, block, missing=0.0) for _ in range(4)]  # letters at the separators 70 and 72 too
    assert all(s[70] in b"ACGT" and s[72] in b"ACGT" for s in samples)
    with rlz.RlzIndex.build(refs) as ix, ix.cohort() as co:
        for s in samples:
            co.add_calls(s)
        calls = same_everything(co, refs, samples, rlz)
        assert all(c[70] == c[72] == ord("N") for c in calls)
        got = co.distances()
        assert (got["compared"] == len(block) - 2).all()
        found = co.sites(0, True)
        assert 70 not in found["position"] and 72 not in found["position"] and set(found["record"].tolist()) == {0, 1, 2}
        assert co.alignment([72, 71, 70])[1][:, [0, 2]].tolist() == [[78, 78]] * 4


def test_sites_none_all_and_agreement_against_the_reference(rlz, monkeypatch):
    rng = random.Random(21)
    B = 150
    ref = dna(rng, B)
    other = bytes({65: 67, 67: 71, 71: 84, 84: 65}[c] for c in ref)   # every base another one
    third = bytes({65: 71, 67: 84, 71: 65, 84: 67}[c] for c in ref)   # and a third
    with rlz.RlzIndex.build([ref]) as ix:
        with ix.cohort() as co:  # none variable
            for s in (ref, ref.lower(), ref):
                co.add_calls(s)
            same_everything(co, [ref], [ref, ref.lower(), ref], rlz)
            assert len(co.sites(0, True)) == 0 and len(co.sites(0, False)) == 0
        with ix.cohort() as co:  # every position variable, with and without the reference
            for s in (ref, other, third):
                co.add_calls(s)
            same_everything(co, [ref], [ref, other, third], rlz)
            assert co.sites(3, False)["position"].tolist() == list(range(B))
            whole = co.sites(0, True)
            for chunk in ("1", "3", "7"):
                monkeypatch.setenv("NOLZSS_RLZ_LOCATE_CHUNK", chunk)  # the knob is read on every call
                assert np.array_equal(co.sites(0, True), whole), chunk
                assert np.array_equal(co.distances()["compared"], np.full((3, 3), B, dtype=np.uint32))
            monkeypatch.delenv("NOLZSS_RLZ_LOCATE_CHUNK")
        with ix.cohort() as co:  # all samples agree on a base that is not the reference's
            for s in (other, other.lower()):
                co.add_calls(s)
            same_everything(co, [ref], [other, other.lower()], rlz)
            assert co.sites(2, True)["position"].tolist() == list(range(B)) and len(co.sites(0, False)) == 0
            assert len(co.sites(3, True)) == 0  # min_present above N


def test_columns_and_calls(rlz, monkeypatch):
    rng = random.Random(33)
    refs = [dna(rng, 100), dna(rng, 99)]
    block = b"\x01".join(refs)
    B = len(block)
    samples = [sample_of(rng, block) for _ in range(5)]
    with rlz.RlzIndex.build(refs) as ix, ix.cohort() as co:
        for s in samples:
            co.add_calls(s)
        calls = [hm.calls_from_bytes(s, block) for s in samples]
        positions = [199, 0, 100, 63, 64, 63, 63, 128, 100, 5]  # unsorted, repeated, the separator
        whole = co.alignment(positions)
        assert whole[0].tolist() == positions and [bytes(r) for r in whole[1]] == hm.columns(calls, positions)
        empty = co.alignment([])
        assert empty[0].shape == (0,) and empty[1].shape == (5, 0)
        for bad in ([B], [0, B + 5], [1 << 40]):
            with pytest.raises(ValueError, match="lies at or beyond the block's length 200"):
                co.alignment(bad)
        for bad in ([-1], [0.5]):
            with pytest.raises(ValueError, match="non-negative integers"):
                co.alignment(bad)
        ranges = [(0, B), (60, 70), (63, 64), (64, 64), (1, 129), (127, 200), (199, 200)]
        for chunk in (None, "1", "3", "7"):
            if chunk:
                monkeypatch.setenv("NOLZSS_RLZ_LOCATE_CHUNK", chunk)  # the knob is read on every call
            assert np.array_equal(co.alignment(positions)[1], whole[1]), chunk
            for s in (0, 4):
                for lo, hi in ranges:
                    assert co.calls(s, lo, hi) == calls[s][lo:hi], (chunk, s, lo, hi)
        monkeypatch.delenv("NOLZSS_RLZ_LOCATE_CHUNK")
        for args in ((5,), (0, 3, 2), (0, 0, B + 1), (-1,), (0, -1)):
            with pytest.raises(ValueError, match="sample|start <= end|negative"):
                co.calls(*args)


def test_refused_adds_leave_the_cohort_as_it_was(rlz):
    rng = random.Random(41)
    ref, elsewhere = dna(rng, 90), dna(rng, 90)
    samples = [sample_of(rng, ref) for _ in range(3)]
    with rlz.RlzIndex.build([ref]) as ix, rlz.RlzIndex.build([elsewhere]) as other, ix.cohort() as co:
        for s, name in zip(samples, ("a", None, b"c")):
            co.add_calls(s, id=name)
        before, info, infos = co.distances(), co.info, co.samples()
        assert co.ids == ["a", None, "c"] and co.calls("c") == co.calls(2) == hm.calls_from_bytes(samples[2], ref)
        for wrong in (ref[:-1], ref + b"A", b""):
            with pytest.raises(ValueError, match="one byte per block position \\(90\\)"):
                co.add_calls(wrong, id="d")
        with pytest.raises(ValueError, match="distinct"):
            co.add_calls(samples[0], id="a")
        with pytest.raises(KeyError):
            co.calls("d")
        with other.pileup() as foreign, pytest.raises(ValueError, match="not open over the index of this cohort"):
            co.add(foreign)
        with ix.pileup() as pile:
            with pytest.raises(ValueError, match="min_fraction"):
                co.add(pile, min_fraction=(2, 1))
        assert co.info == info and co.samples() == infos and co.ids == ["a", None, "c"]
        after = co.distances()
        assert all(np.array_equal(after[k], before[k]) for k in before)
        assert co.add_calls(samples[1], id="d")["sample"] == 3 and co.calls("d") == co.calls(1)
    with pytest.raises(ValueError, match="the cohort is closed"):
        co.distances()


CHILD = r'''
import random, sys
sys.path.insert(0, "tests")
import numpy as np
import rlz_cohort_model as hm
from nolzss_amd.genomics import rlz
rng = random.Random(77)
ref = bytes(rng.choice(b"ACGT") for _ in range(300))
samples = [bytes(rng.choice(b"N-") if rng.random() < 0.3 else rng.choice(b"ACGT") for _ in range(300)) for _ in range(9)]
calls = [hm.calls_from_bytes(s, ref) for s in samples]
with rlz.RlzIndex.build([ref]) as ix, ix.cohort() as co:
    assert co.info["capacity"] == 0 and co.info["device_bytes"] == 0
    capacities = []
    for n, s in enumerate(samples):
        assert co.add_calls(s)["sample"] == n
        capacities.append(co.info["capacity"])
        for k in range(n + 1):  # every sample read back after every growth
            assert co.calls(k) == calls[k], (n, k)
    assert capacities == [1, 2, 4, 4, 8, 8, 8, 8, 16] and co.info["device_bytes"] == 16 * 24 * 5
    diff, comp = hm.distances(calls)
    got = co.distances()
    assert got["differences"].tolist() == diff and got["compared"].tolist() == comp
    print("ok", capacities[-1], int(got["differences"].sum()))
'''


def test_a_cohort_that_grows_from_one_sample_in_a_child_process(rlz):
    """NOLZSS_RLZ_COHORT_SAMPLES=1 for a whole process: the allocation doubles four times under nine samples, and every
    sample reads back after every growth"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, NOLZSS_RLZ_COHORT_SAMPLES="1")
    r = subprocess.run([sys.executable, "-c", CHILD], cwd=root, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("ok 16 "), r.stdout[-2000:] + r.stderr[-4000:]
    assert int(r.stdout.split()[2]) > 0
