"""Relative LZ on the device (rlz.hip, rlz_api.hip): every target against the reference block only.  Small and
tile-crossing inputs against the brute force of the definition, a mid-size input against the array model over the
device's own SA / LCP (tests/rlz_model.py), and the properties the parse is built for: counts without records, FASTA
input, independence from the order and the number of the targets."""
import functools

import numpy as np
import pytest

import gen
import genomes
import rlz_model as model

pytestmark = pytest.mark.gpu

RC_BIT = np.uint32(1 << 31)


@pytest.fixture(scope="module")
def native():
    from nolzss_amd import _noLZSS
    assert _noLZSS.device_count() >= 1, "no MI355X visible"
    return _noLZSS


def _dna(n, seed, alphabet=b"ACGT"):
    rng = np.random.default_rng(seed)
    return np.frombuffer(alphabet, dtype=np.uint8)[rng.integers(0, len(alphabet), n)].tobytes()


def check_against_brute(native, refs, targets, with_rc, codes=False):
    """every record, the counts-only form and the rebased Python form against the definition"""
    from nolzss_amd.genomics import rlz
    got = native.rlz_factorize_arrays(refs, targets, with_rc=with_rc)
    rebased = rlz.rlz_factorize(refs, targets, with_rc=with_rc)
    refs = [refs] if isinstance(refs, bytes) else refs  # (the entry points take one sequence or a list)
    exp = model.brute_absolute(refs, targets, with_rc)
    lay = model.layout(refs, targets, with_rc)
    assert got["target_offsets"] == lay["target_offsets"] and got["block_length"] == lay["block_length"]
    assert got["target_lengths"] == [len(t) for t in targets]
    assert got["counts"] == [len(e) for e in exp]
    for j, e in enumerate(exp):
        assert np.array_equal(got["factors"][j], e), f"target {j}"
    assert native.rlz_factorize_arrays(refs, targets, with_rc=with_rc, want_factors=False)["counts"] == got["counts"]
    for j, t in enumerate(targets):
        rows = [tuple(r) for r in rebased[j].tolist()]
        assert rows == model.brute_parse(refs, t, with_rc), f"target {j}"
    if codes:
        code = native.debug_rlz_codes(refs, targets, with_rc=with_rc)
        for j, (t, off) in enumerate(zip(targets, lay["target_offsets"])):
            assert np.array_equal(code[off:off + len(t)], model.brute_codes(refs, t, with_rc)), f"codes of target {j}"
    return got


# ---- hand cases ----------------------------------------------------------------------------------------------------
R1 = b"ACGGTCATTGCAAGCTTAGGCATCGA"
R2 = b"TTGACCGGTAAGGCCTTTAGACCA"


@pytest.mark.parametrize("with_rc", [True, False])
def test_target_equal_to_the_reference_is_one_factor(native, with_rc):
    got = check_against_brute(native, [R1], [R1], with_rc)
    f = got["factors"][0]
    assert len(f) == 1 and int(f["length"][0]) == len(R1) and int(f["ref"][0]) == 0


def test_reverse_complement_of_the_reference_is_one_rc_factor(native):
    got = check_against_brute(native, [R1], [model.revcomp(R1)], True)
    f = got["factors"][0]
    assert len(f) == 1 and int(f["length"][0]) == len(R1) and int(f["ref"][0]) == model.RC_MASK
    check_against_brute(native, [R1], [model.revcomp(R1)], False)


def test_forward_wins_on_a_palindromic_site(native):
    site = b"GAATTC"  # its own reverse complement: Lf == Lr
    ref = b"CC" + site + b"CC"
    got = check_against_brute(native, [ref], [site], True)
    f = got["factors"][0]
    assert len(f) == 1 and int(f["ref"][0]) == 2, "forward, no mask"


@pytest.mark.parametrize("with_rc", [True, False])
def test_base_in_neither_strand_is_a_literal(native, with_rc):
    ref = b"ATTATAATTTA"  # A and T only, on both strands
    got = check_against_brute(native, [ref], [b"ATGAT", b"GCG"], with_rc)
    assert got["counts"] == [3, 3]
    g = got["factors"][1]
    assert all(int(r["ref"]) == int(r["start"]) and int(r["length"]) == 1 for r in g)


@pytest.mark.parametrize("with_rc", [True, False])
def test_target_across_the_record_boundary_splits_there(native, with_rc):
    target = R1[-9:] + R2[:9]
    got = check_against_brute(native, [R1, R2], [target], with_rc)
    f = got["factors"][0]
    assert int(f["length"][0]) == 9 and int(f["ref"][0]) == len(R1) - 9
    assert int(f["ref"][1]) == len(R1) + 1, "the second factor starts behind the separator"


@pytest.mark.parametrize("with_rc", [True, False])
def test_empty_target_between_two_others(native, with_rc):
    got = check_against_brute(native, [R1, R2], [R2[3:17], b"", model.revcomp(R1[2:20]) + b"A"], with_rc)
    assert got["counts"][1] == 0 and len(got["factors"][1]) == 0


@pytest.mark.parametrize("with_rc", [True, False])
def test_one_target(native, with_rc):
    check_against_brute(native, [R1], [R1[5:15] + b"T" + R1[1:8]], with_rc, codes=True)
    check_against_brute(native, R1, [b"A"], with_rc, codes=True)


@pytest.mark.parametrize("with_rc", [True, False])
def test_two_hundred_short_targets(native, with_rc):
    rng = np.random.default_rng(200)
    ref = _dna(300, 11)
    targets = []
    for j in range(200):
        n = int(rng.integers(1, 31))
        a = int(rng.integers(0, len(ref) - n))
        piece = ref[a:a + n]
        targets.append([piece, model.revcomp(piece), _dna(n, 1000 + j)][j % 3])
    check_against_brute(native, [ref], targets, with_rc, codes=True)


# ---- several scan tiles with a ragged tail --------------------------------------------------------------------------
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
                t += model.revcomp(piece)
            else:
                t += _dna(int(rng.integers(1, 30)), int(rng.integers(1 << 30)))
        targets.append(t[:n])
    return targets


@pytest.mark.parametrize("with_rc", [True, False])
def test_tile_crossing_against_the_brute_force(native, with_rc):
    ref = _dna(6000, 60)
    targets = _cut_targets(ref, 61, [5000, 0, 3777, 4096, 4999])  # |S| about 30 000 with the mirror: 8 tiles, ragged
    check_against_brute(native, [ref[:2500], ref[2500:]], targets, with_rc, codes=True)


def test_tiles_without_a_flagged_rank_forward(native):
    """reference over {A, C}, 18 000 target bases over {G, T}: more than four whole tiles of consecutive ranks hold no
    reference suffix, and the state carried across them must not invent a match"""
    ref = _dna(3000, 70, b"AC")
    block = _dna(18000, 71, b"GT")
    targets = [ref[100:900], ref[5:300] + block + ref[2000:2600], _dna(500, 72)]
    got = check_against_brute(native, [ref], targets, False)
    code = native.debug_rlz_codes([ref], targets, with_rc=False)
    off = got["target_offsets"][1] + 295
    assert not code[off:off + len(block)].any()
    assert code[got["target_offsets"][1]] == 295


def test_tiles_without_a_flagged_rank_with_rc(native):
    """reference over {A}: its mirror is over {T}, and the 18 000 ranks of a target block over {C, G} lie between the
    two flagged runs with no flagged rank among them"""
    ref = b"A" * 700
    block = _dna(18000, 73, b"CG")
    targets = [b"A" * 30 + block + b"T" * 40, b"TTTTAAAA", block[:50]]
    got = check_against_brute(native, [ref], targets, True)
    code = native.debug_rlz_codes([ref], targets, with_rc=True)
    off = got["target_offsets"][0] + 30
    assert not code[off:off + len(block)].any()
    assert code[got["target_offsets"][0]] == 30 and code[off + len(block)] == (40 | RC_BIT)


# ---- mid size against the array model ---------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _mid_inputs():
    ref = gen.random_dna(560_000, seed=80).tobytes()
    targets = _cut_targets(ref, 81, [90_000, 70_001, 60_000])
    return [ref[:300_000], ref[300_000:]], targets


@pytest.mark.parametrize("with_rc", [True, False])
def test_mid_size_against_the_array_model(native, with_rc):
    refs, targets = _mid_inputs()
    if not with_rc:  # keep |S| near 1.3 * 2^20 without the mirror
        refs = refs + [gen.random_dna(560_000, seed=82).tobytes()]
    lay = native.rlz_prepare(refs, targets, with_rc=with_rc)
    S, B = lay["S"], lay["block_length"]
    assert 1.2 * 2 ** 20 < len(S) < 1.4 * 2 ** 20
    chain_end = lay["target_offsets"][-1] + len(targets[-1])
    arrays = native.debug_arrays(S)  # (pinned to the oracle by the pipeline tests)
    code = model.array_codes(arrays["sa"], arrays["lcp"], B, lay["rc_block_start"], with_rc)
    recs = model.array_records(arrays["sa"], arrays["lcp"], code, B, chain_end, lay["rcN"])
    got_code = native.debug_rlz_codes(refs, targets, with_rc=with_rc)
    got = native.rlz_factorize_arrays(refs, targets, with_rc=with_rc)
    for j, (t, off) in enumerate(zip(targets, lay["target_offsets"])):
        assert np.array_equal(got_code[off:off + len(t)], code[off:off + len(t)]), f"codes of target {j}"
        exp = model.records_of_target(recs, off, len(t))
        assert got["counts"][j] == len(exp)
        assert np.array_equal(got["factors"][j], exp), f"records of target {j}"
    assert native.rlz_factorize_arrays(refs, targets, with_rc=with_rc, want_factors=False)["counts"] == got["counts"]
    if with_rc:
        assert any((f["ref"] >> np.uint64(63)).any() for f in got["factors"]), "the input must exercise the other strand"


# ---- FASTA input, order and number of the targets --------------------------------------------------------------------
@pytest.mark.parametrize("with_rc", [True, False])
@pytest.mark.parametrize("ref_name, tgt_name", [("short_dna2", "short_dna1"), ("test_bacterial_dna", "T7"),
                                                ("T3", "test_bacterial_dna")])
def test_fasta_entry_point(native, tmp_path, ref_name, tgt_name, with_rc):
    from nolzss_amd.genomics import rlz
    ref_path, tgt_path = genomes.materialize(ref_name, tmp_path), genomes.materialize(tgt_name, tmp_path)
    res = rlz.rlz_factorize_fasta(ref_path, tgt_path, with_rc=with_rc)
    ref_recs, tgt_recs = native.debug_parse_fasta(ref_path), native.debug_parse_fasta(tgt_path)
    assert res["reference_ids"] == [i.decode() for i, _ in ref_recs] == [i for i, _ in genomes.records(ref_name)]
    assert res["target_ids"] == [i.decode() for i, _ in tgt_recs] == [i for i, _ in genomes.records(tgt_name)]
    assert res["target_lengths"] == [len(s) for _, s in tgt_recs]
    exp = rlz.rlz_factorize([s for _, s in ref_recs], [s for _, s in tgt_recs], with_rc=with_rc)
    assert res["counts"] == [len(e) for e in exp]
    for a, b in zip(res["factors"], exp):
        assert np.array_equal(a, b)
    counts_only = rlz.rlz_factorize_fasta(ref_path, tgt_path, with_rc=with_rc, want_factors=False)
    assert counts_only["counts"] == res["counts"] and counts_only["factors"] is None
    summary = rlz.rlz_summary(res["factors"])
    for s, n in zip(summary, res["target_lengths"]):
        assert s["forward_bases"] + s["rc_bases"] + s["literal_bases"] == n


@pytest.mark.parametrize("with_rc", [True, False])
def test_a_target_does_not_depend_on_the_others(native, with_rc):
    from nolzss_amd.genomics import rlz
    ref = _dna(5000, 90)
    targets = _cut_targets(ref, 91, [1200, 800, 0, 1500, 700])
    refs = [ref[:1800], ref[1800:]]
    base = rlz.rlz_factorize(refs, targets, with_rc=with_rc)
    order = [3, 0, 4, 2, 1]
    permuted = rlz.rlz_factorize(refs, [targets[j] for j in order], with_rc=with_rc)
    for slot, j in enumerate(order):
        assert np.array_equal(permuted[slot], base[j]), f"target {j} changed when the targets were permuted"
    more = rlz.rlz_factorize(refs, targets[:2] + [targets[0] + targets[3]] + targets[2:], with_rc=with_rc)
    for j, slot in enumerate([0, 1, 3, 4, 5]):
        assert np.array_equal(more[slot], base[j]), f"target {j} changed when another target was added"
    alone = rlz.rlz_factorize(refs, [targets[3]], with_rc=with_rc)
    assert np.array_equal(alone[0], base[3])
    assert rlz.rlz_count_factors(refs, targets, with_rc=with_rc) == [len(b) for b in base]
