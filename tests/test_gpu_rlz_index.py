"""The relative-LZ index on the device (rlz_index.hip, rlz_index_api.hip): target batches matched against a resident
reference.  Oracles: the brute force of the definition (tests/rlz_model.py) and, wherever it accepts the input, the
existing path nolzss_rlz_factorize record for record."""
import re
import threading
from pathlib import Path

import numpy as np
import pytest

import rlz_model as model

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def native():
    from nolzss_amd import _noLZSS
    assert _noLZSS.device_count() >= 1, "no MI355X visible"
    return _noLZSS


@pytest.fixture(scope="module")
def rlz():
    from nolzss_amd.genomics import rlz
    return rlz


def _dna(n, seed, alphabet=b"ACGT"):
    rng = np.random.default_rng(seed)
    return np.frombuffer(alphabet, dtype=np.uint8)[rng.integers(0, len(alphabet), n)].tobytes()


def _as_list(refs):
    return [refs] if isinstance(refs, (bytes, str)) else list(refs)


def _offsets(refs, targets):
    """(B, the absolute first position of every target): B + 1 + its position in T1 s T2 s .. Tk s"""
    B = sum(len(r) for r in refs) + len(refs) - 1
    offs, at = [], B + 1
    for t in targets:
        offs.append(at)
        at += len(t) + 1
    return B, offs


def brute_absolute(refs, targets, with_rc):
    """model.brute_absolute for any number of targets (its layout runs out of sentinels beyond 250)"""
    B, offs = _offsets(refs, targets)
    out = []
    for t, off in zip(targets, offs):
        e = model.brute_absolute(refs, [t], with_rc)[0].copy()
        literal = e["ref"] == e["start"]
        e["start"] += np.uint64(off - (B + 1))
        e["ref"][literal] = e["start"][literal]
        out.append(e)
    return out


def check_index(native, rlz, refs, targets, with_rc, prefix_syms=0, codes=False, existing=True, exp=None):
    """records, counts-only, (codes) and the rebased rows of one index against the definition and the existing path"""
    refs = _as_list(refs)
    B, offs = _offsets(refs, targets)
    exp = brute_absolute(refs, targets, with_rc) if exp is None else exp
    with rlz.RlzIndex.build(refs, with_rc=with_rc, prefix_syms=prefix_syms) as ix:
        info = ix.info()
        assert info["block_length"] == B and info["num_references"] == len(refs) and info["with_rc"] == int(with_rc)
        assert info["index_length"] == (2 * B + 2 if with_rc else B + 1) and info["device_bytes"] > 0
        assert info["prefix_syms"] == prefix_syms or (prefix_syms == 0 and 4 <= info["prefix_syms"] <= 12)
        got = ix._live().factorize_arrays(targets)
        assert got["block_length"] == B and got["target_offsets"] == offs
        assert got["target_lengths"] == [len(t) for t in targets]
        assert got["counts"] == [len(e) for e in exp]
        for j, e in enumerate(exp):
            assert np.array_equal(got["factors"][j], e.astype(native.FACTOR_DTYPE)), f"target {j}"
        assert ix.count_factors(targets) == got["counts"]
        rows = ix.factorize(targets)
        for j, t in enumerate(targets):
            assert np.array_equal(rows[j], rlz.rebase(got["factors"][j], offs[j])), f"rebased target {j}"
        if codes:
            code = ix.codes(targets)
            assert len(code) == sum(map(len, targets)) + len(targets)
            for j, (t, off) in enumerate(zip(targets, offs)):
                p = off - (B + 1)
                assert np.array_equal(code[p:p + len(t)], model.brute_codes(refs, t, with_rc)), f"codes of target {j}"
    if existing:
        old = native.rlz_factorize_arrays(refs, targets, with_rc=with_rc)
        assert old["target_offsets"] == got["target_offsets"] and old["counts"] == got["counts"]
        for j in range(len(targets)):
            assert np.array_equal(old["factors"][j], got["factors"][j]), f"target {j} against the existing path"
    return got


# ---- 1. the hand cases of test_gpu_rlz.py ---------------------------------------------------------------------------
R1 = b"ACGGTCATTGCAAGCTTAGGCATCGA"
R2 = b"TTGACCGGTAAGGCCTTTAGACCA"


@pytest.mark.parametrize("with_rc", [True, False])
def test_hand_cases(native, rlz, with_rc):
    got = check_index(native, rlz, [R1], [R1], with_rc, codes=True)
    f = got["factors"][0]
    assert len(f) == 1 and int(f["length"][0]) == len(R1) and int(f["ref"][0]) == 0
    got = check_index(native, rlz, R1, [model.revcomp(R1)], with_rc, codes=True)
    if with_rc:
        f = got["factors"][0]
        assert len(f) == 1 and int(f["length"][0]) == len(R1) and int(f["ref"][0]) == model.RC_MASK
    site = b"GAATTC"  # its own reverse complement: Lf == Lr, forward wins
    got = check_index(native, rlz, [b"CC" + site + b"CC"], [site], with_rc, codes=True)
    assert len(got["factors"][0]) == 1 and int(got["factors"][0]["ref"][0]) == 2
    target = R1[-9:] + R2[:9]
    got = check_index(native, rlz, [R1, R2], [target, R2[3:17], b"", model.revcomp(R1[2:20]) + b"a"], with_rc, codes=True)
    f = got["factors"][0]
    assert int(f["length"][0]) == 9 and int(f["ref"][0]) == len(R1) - 9 and int(f["ref"][1]) == len(R1) + 1
    assert got["counts"][2] == 0
    got = check_index(native, rlz, [b"ATTATAATTTA"], [b"ATGAT", b"GCG"], with_rc, codes=True)
    assert got["counts"] == [3, 3]
    assert all(int(r["ref"]) == int(r["start"]) and int(r["length"]) == 1 for r in got["factors"][1])


# ---- 2. the edges of the prefix table ---------------------------------------------------------------------------------
@pytest.mark.parametrize("with_rc", [True, False])
@pytest.mark.parametrize("prefix_syms", [1, 2, 4, 0])
def test_prefix_table_edges(native, rlz, with_rc, prefix_syms):
    P = prefix_syms or 4  # (0 picks 4 on index texts this small)
    ref = _dna(90, 5)
    lengths = sorted({0, 1, max(P - 1, 0), P, P + 1})
    targets = [ref[7:7 + n] for n in lengths] + [model.revcomp(ref[20:20 + n]) for n in lengths] + [_dna(n, 60 + n) for n in lengths]
    targets += [b"A" * 9, b"T" * 9, b"A", b"T", b"AAAAC", b"TTTTG"]  # the first and the last table entry
    check_index(native, rlz, [ref], targets, with_rc, prefix_syms, codes=True)
    # a reference shorter than P, and records shorter than P (short suffixes at the front of their buckets) with an
    # empty record among m = 3
    check_index(native, rlz, [b"AC"], [b"ACAC", b"GT", b"A", b"", b"CA"], with_rc, prefix_syms, codes=True)
    check_index(native, rlz, [b"ACA", b"", b"CAAT"], [b"ACAAT", b"ACACAAT", b"ATTG", b"AAAA", b"TGT", b"CA"], with_rc,
                prefix_syms, codes=True)
    check_index(native, rlz, [b"A", b"AA", b"AAA" + ref[:P + 2]], [b"AAAA", b"AAA" + ref[:P], b"TTTT", ref[:P + 2]], with_rc,
                prefix_syms, codes=True)
    # a target P-mer that X does not hold: over an A/C reference a target with G or T matches nothing forward, its
    # mirror matches with reverse complement, and its short matches come from a bucket's edge neighbours
    ac = _dna(70, 9, b"AC")
    mixed = [ac[5:5 + P + 3] + b"G" + ac[30:40], b"GT" * 5, model.revcomp(ac[10:10 + P + 6]), ac[3:3 + P - 1] + b"T" + ac[3:9],
             b"G" + ac[50:50 + P], model.revcomp(ac[0:P]) + b"A"]
    got = check_index(native, rlz, [ac], mixed, with_rc, prefix_syms, codes=True)
    g = got["factors"][1]  # GT GT ..: literals without the mirror, copies of the mirror with it
    assert bool(np.all(g["ref"] == g["start"])) == (not with_rc)


# ---- 3. word alignment -------------------------------------------------------------------------------------------------
MATCH_LENGTHS = [31, 32, 33, 63, 64, 65, 200]
ALIGN = [0, 1, 31]


def _alignment_case():
    """Reference records built so that for every match length and every residue c the block holds a start = c mod 32
    whose match ends at a record separator (the last record: at the end of Rblk), and an interior start = c mod 32.
    Targets are placed so that the match starts at a batch position = ct mod 32, for ct in ALIGN, and ends by a
    mismatch, by the target's end, or by the separator / block end; reverse-complemented copies end at the mirror's."""
    rng = np.random.default_rng(77)
    refs, plan, at = [], [], 0
    for L in MATCH_LENGTHS:
        for c in ALIGN:
            head = (c - at) % 32
            n = head + 32 + L  # interior start at + head = c, tail start at + head + 32 = c (mod 32)
            refs.append(_dna(n, int(rng.integers(1 << 30))))
            plan.append((len(refs) - 1, L, head))
            at += n + 1
    targets, expect, pos = [], [], 0  # pos: position of the next target in T1 s T2 s ..

    def add(piece, tail, rc=False):
        nonlocal pos
        for ct in ALIGN:
            pre = _dna((ct - pos) % 32, int(rng.integers(1 << 30)))
            body = model.revcomp(piece) if rc else piece
            targets.append(pre + body + tail)
            expect.append((len(pre), len(piece), rc))
            pos += len(targets[-1]) + 1

    other = {65: b"C", 67: b"G", 71: b"T", 84: b"A"}
    for j, L, head in plan:
        r = refs[j]
        inner = r[head:head + L]
        add(inner, other[r[head + L]] + _dna(6, j))  # ends by a mismatch
        add(inner, b"")                               # ends by the target's end
        add(r[-L:], _dna(5, 100 + j))                 # ends by the separator (the last record: by the end of Rblk)
        add(r[:L], _dna(5, 200 + j), rc=True)         # mirrored: ends by a separator of the mirror
    add(refs[0][:64], _dna(7, 3), rc=True)            # ... and by the end of the mirror, which closes with rc(R1)
    add(refs[-1][-33:], b"")                          # the end of Rblk and the target's end at once
    return refs, targets, expect


@pytest.mark.parametrize("with_rc", [True, False])
def test_matches_across_word_boundaries(native, rlz, with_rc):
    refs, targets, expect = _alignment_case()
    assert len(targets) > 250  # (more than the existing path takes in one call)
    B, offs = _offsets(refs, targets)
    block = model.SEP.join(refs)
    residues = set()
    for (pre, L, rc), off, t in zip(expect, offs, targets):
        if rc and not with_rc:
            continue
        assert model._longest(block, t, pre, rc) == L, "the case is built for a match of exactly L"
        piece = model.revcomp(t[pre:pre + L]) if rc else t[pre:pre + L]
        residues.add(((off - B - 1 + pre) % 32, block.find(piece) % 32, rc))
    for rc in ([False, True] if with_rc else [False]):
        assert {a for a, _, r in residues if r == rc} == set(ALIGN)
    assert {b for _, b, r in residues if not r} >= set(ALIGN)
    check_index(native, rlz, refs, targets, with_rc, codes=True, existing=False)


# ---- 4. deep buckets, leftmost occurrences -------------------------------------------------------------------------------
@pytest.mark.parametrize("prefix_syms", [2, 0])
def test_repeats_give_the_leftmost_occurrence(native, rlz, prefix_syms):
    rng = np.random.default_rng(4)
    unit = bytearray(_dna(40, 44))
    ref = bytearray()
    for _ in range(300):  # the unit with one substitution each
        u = bytearray(unit)
        q = int(rng.integers(40))
        u[q] = b"ACGT"[(b"ACGT".index(u[q]) + 1 + int(rng.integers(3))) % 4]
        ref += u
    ref = bytes(ref)
    targets = [bytes(unit), model.revcomp(bytes(unit))]
    for i in (0, 7, 150, 298):
        targets += [ref[40 * i:40 * i + 40], model.revcomp(ref[40 * i:40 * i + 40])]
    for i in (3, 100, 297):
        targets += [ref[40 * i:40 * i + 120], model.revcomp(ref[40 * i + 5:40 * i + 125])]
    for with_rc in (True, False):
        got = check_index(native, rlz, [ref], targets, with_rc, prefix_syms)
        for t, f in zip(targets, got["factors"]):  # (the brute force is the leftmost occurrence; said once more)
            for r in f:
                if int(r["ref"]) != int(r["start"]) and not int(r["ref"]) >> 63:
                    p = int(r["start"]) - int(f["start"][0])
                    assert ref.find(t[p:p + int(r["length"])]) == int(r["ref"])


# ---- 5. more targets than sentinels ------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_rc", [True, False])
def test_six_hundred_targets(native, rlz, with_rc):
    rng = np.random.default_rng(600)
    ref = _dna(2000, 6)
    targets = []
    for j in range(600):
        n = int(rng.integers(0, 41))
        a = int(rng.integers(0, len(ref) - 40))
        t = bytearray(ref[a:a + n])
        if j % 3 == 1 and n:
            t[int(rng.integers(n))] = b"ACGT"[int(rng.integers(4))]
        targets.append(model.revcomp(bytes(t)) if j % 3 == 2 else bytes(t))
    with pytest.raises(ValueError, match="Too many sequences"):
        rlz.rlz_factorize([ref], targets, with_rc=with_rc)
    check_index(native, rlz, [ref], targets, with_rc, existing=False)
    with rlz.RlzIndex.build(ref, with_rc=with_rc) as ix:  # several batches give the same rows
        whole = ix.factorize(targets)
        parts = ix.factorize(targets, batch_bases=1500)
        assert len(parts) == 600 and all(np.array_equal(a, b) for a, b in zip(whole, parts))
        assert ix.count_factors(targets, batch_bases=700) == [len(f) for f in whole]


# ---- 6. mid-size against the existing path --------------------------------------------------------------------------------
def _mutated(ref, rng, n, invert):
    a = int(rng.integers(0, len(ref) - n))
    t = bytearray(ref[a:a + n])
    for q in rng.integers(0, n, n // 200):  # 0.5 % substitutions
        t[int(q)] = b"ACGT"[int(rng.integers(4))]
    for q in sorted((int(x) for x in rng.integers(1, n - 1, 4)), reverse=True):  # a few indels
        if q % 2:
            del t[q:q + 3]
        else:
            t[q:q] = b"GATTACA"
    t = bytes(t)
    if invert:  # an inverted tenth
        lo = len(t) // 3
        t = t[:lo] + model.revcomp(t[lo:lo + len(t) // 10]) + t[lo + len(t) // 10:]
    return t


@pytest.fixture(scope="module")
def midsize(native):
    rng = np.random.default_rng(17)
    block = _dna(1 << 17, 1717)
    refs = [block[:70001], block[70001:]]
    joined = model.SEP.join(refs)
    targets = [_mutated(joined.replace(model.SEP, b""), rng, int(rng.integers(1 << 15, (1 << 16) + 1)), j % 3 == 0)
               for j in range(12)]
    out = {"refs": refs, "targets": targets}
    for with_rc in (True, False):
        out[with_rc] = (native.rlz_factorize_arrays(refs, targets, with_rc=with_rc),
                        native.debug_rlz_codes(refs, targets, with_rc=with_rc))
    return out


@pytest.mark.parametrize("with_rc", [True, False])
def test_midsize_equals_the_existing_path(native, rlz, midsize, with_rc):
    refs, targets = midsize["refs"], midsize["targets"]
    old, old_code = midsize[with_rc]
    B, offs = _offsets(refs, targets)
    with rlz.RlzIndex.build(refs, with_rc=with_rc) as ix:
        assert ix.info()["prefix_syms"] == (8 if with_rc else 7)  # floor(log4 |X|) - 1, |X| = 2^18 + 4 or 2^17 + 2
        got = ix._live().factorize_arrays(targets)
        code = ix.codes(targets)
        counts = ix.count_factors(targets)
    assert got["target_offsets"] == old["target_offsets"] and got["counts"] == old["counts"] == counts
    for j, (t, off) in enumerate(zip(targets, offs)):
        assert np.array_equal(got["factors"][j], old["factors"][j]), f"target {j}"
        assert np.array_equal(code[off - B - 1:off - B - 1 + len(t)], old_code[off:off + len(t)]), f"codes of target {j}"
    for j in (0, 7):
        rows = [tuple(r) for r in rlz.rebase(got["factors"][j], offs[j]).tolist()]
        assert rows == model.brute_parse(refs, targets[j], with_rc), f"target {j}"


# ---- 7. the life of a handle -------------------------------------------------------------------------------------------
def test_handle_life(native, rlz):
    ref = [_dna(3000, 70), _dna(1500, 71)]
    rng = np.random.default_rng(7)
    block = b"".join(ref)
    targets = []
    for j in range(40):
        a, n = int(rng.integers(0, len(block) - 300)), int(rng.integers(0, 300))
        targets.append([block[a:a + n], model.revcomp(block[a:a + n]), _dna(n, 700 + j)][j % 3])
    ix = rlz.RlzIndex.build(ref)
    assert ix.info()["device_bytes"] > 0 and ix.info()["device"] == native.get_device()
    whole = ix.factorize(targets)
    first, second = ix.factorize(targets[:13]), ix.factorize(targets[13:])  # two successive batches
    assert all(np.array_equal(a, b) for a, b in zip(whole, first + second))
    perm = [int(x) for x in rng.permutation(len(targets))]
    shuffled = ix.factorize([targets[i] for i in perm])
    assert all(np.array_equal(shuffled[q], whole[i]) for q, i in enumerate(perm))
    # other calls between two matches leave the handle intact
    import nolzss_amd
    assert len(nolzss_amd.factorize(block)) > 0
    with rlz.RlzArchive.build(ref, targets[:5]) as arc:
        assert arc.target(3) == targets[3]
    again = ix.factorize(targets)
    assert all(np.array_equal(a, b) for a, b in zip(whole, again))
    # two threads at once agree with the serial result
    results, errors = {}, []

    def work(name, part):
        try:
            results[name] = ix.factorize(part)
        except Exception as e:  # pragma: no cover
            errors.append(e)

    threads = [threading.Thread(target=work, args=("a", targets[:20])), threading.Thread(target=work, args=("b", targets[20:]))]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors
    assert all(np.array_equal(a, b) for a, b in zip(whole, results["a"] + results["b"]))
    assert ix.factorize([]) == [] and ix.count_factors([]) == [] and len(ix.codes([])) == 0
    ix.close()
    ix.close()
    with pytest.raises(ValueError, match="closed"):
        ix.factorize(targets[:2])
    with pytest.raises(ValueError, match="closed"):
        ix.info()


def test_from_fasta(native, rlz, tmp_path):
    path = tmp_path / "ref.fa"
    path.write_text(">one\n" + R1.decode() + "\n>two\n" + R2.decode().lower() + "\n")
    targets = [R1[-9:] + R2[:9], model.revcomp(R2)]
    with rlz.RlzIndex.from_fasta(path) as ix, rlz.RlzIndex.build([R1, R2]) as iy:
        assert ix.info()["block_length"] == len(R1) + 1 + len(R2) and ix.info()["num_references"] == 2
        assert all(np.array_equal(a, b) for a, b in zip(ix.factorize(targets), iy.factorize(targets)))
        with ix.archive(targets) as arc:
            assert [arc.target(j) for j in range(2)] == targets


# ---- 8. no sort in a match -----------------------------------------------------------------------------------------------
def test_a_match_runs_no_suffix_sort(native, rlz):
    scopes = set()
    for name in ("suffix_array.hip", "sa_regroup.hip", "sa_direct.hip", "sa_repeats.hip"):
        src = (ROOT / "nolzss_amd" / "csrc" / name).read_text()
        scopes |= set(re.findall(r'ProfScope\s+\w+\([^"\n]*"([a-z_0-9]+)"', src))
    assert {"sa_sort_initial", "sa_regroup", "sa_direct_sort"} <= scopes
    ref = _dna(20000, 80)
    targets = [ref[100:4100], model.revcomp(ref[9000:12000]), _dna(500, 81)]
    with rlz.RlzIndex.build(ref) as ix:
        warm = ix.factorize(targets)
        native.profile_enable(True)
        try:
            native.profile_reset()
            got = ix.factorize(targets)
            report = native.profile_report()
        finally:
            native.profile_enable(False)
            native.profile_reset()
    assert all(np.array_equal(a, b) for a, b in zip(warm, got))
    assert report["rlz_index_search"][0] == 1 and report["rlz_index_records"][0] >= 1
    assert not scopes & set(report), sorted(scopes & set(report))


# ---- 9. the archive of a batch ---------------------------------------------------------------------------------------------
def test_archive_of_the_midsize_targets(native, rlz, midsize):
    refs, targets = midsize["refs"], midsize["targets"]
    with rlz.RlzIndex.build(refs) as ix, ix.archive(targets, ids=[f"t{j}" for j in range(len(targets))]) as arc:
        assert arc.target_lengths == [len(t) for t in targets]
        got = arc.extract([(j, 0, len(t)) for j, t in enumerate(targets)])
        assert got == targets
        assert arc.target("t5") == targets[5]


# ---- 10. refusals with a device ----------------------------------------------------------------------------------------
def test_refusals_of_a_match(native, rlz):
    import ctypes as C
    from nolzss_amd import _lib
    with rlz.RlzIndex.build([R1, R2]) as ix:
        with pytest.raises(RuntimeError, match="Invalid nucleotide 'N' found in sequence 3"):
            ix.factorize([b"ACGT", b"ACNT"])  # j = m + the target's index
        with pytest.raises(RuntimeError, match="Invalid nucleotide 'x' found in sequence 2"):
            ix.codes([b"xA"])
        with pytest.raises(RuntimeError, match="Invalid nucleotide"):
            ix.count_factors([b"AC GT"])
        # a batch over the length rule: the lengths alone decide, the 4 bytes behind the pointer are never read
        h = ix._live()._handle()
        tg, ln, res = (C.c_char_p * 1)(b"ACGT"), (C.c_size_t * 1)(rlz.MAX_TEXT - ix.info()["block_length"] - 1), _lib.RlzResult()
        assert _lib.lib.nolzss_rlz_index_factorize(h, tg, ln, 1, 1, C.byref(res)) == _lib.ERR_INVALID_ARGUMENT
        assert b"text too long" in _lib.lib.nolzss_last_error()
        assert _lib.lib.nolzss_rlz_index_factorize(h, None, None, 1, 1, C.byref(res)) == _lib.ERR_INVALID_ARGUMENT
        assert len(ix.factorize([R1])[0]) == 1  # the handle is still good
