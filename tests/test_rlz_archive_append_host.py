"""CPU tests (no GPU) of the append path of the relative-LZ archive: the numpy model of the conversion
(tests/rlz_append_model.py) against genomics.rlz.absolute_records and rlz_literals, the id rules of RlzArchive.append and
the batch planning against the room an archive has left."""
import numpy as np
import pytest

import rlz_append_model as am
import rlz_model as model
from rlz_index_model import IndexModel


@pytest.fixture(scope="module")
def rlz():
    from nolzss_amd.genomics import rlz
    return rlz


def _dna(rng, n, alphabet=b"ACGT"):
    return np.frombuffer(alphabet, dtype=np.uint8)[rng.integers(0, len(alphabet), n)].tobytes()


def _rows(rlz, refs, targets, with_rc):
    out = []
    for t in targets:
        rows = model.brute_parse(refs, t, with_rc)
        a = np.zeros(len(rows), dtype=rlz.RLZ_DTYPE)
        for q, r in enumerate(rows):
            a[q] = r
        out.append(a)
    return out


def _case(seed):
    """-> (refs, targets, with_rc, cut): 1 to 3 reference records, 0 to 6 targets with empty ones in every position (a
    third of the cases) or only empty ones (every tenth case), both strand settings; the targets go up as two batches
    [0, cut) and [cut, k)"""
    rng = np.random.default_rng(seed)
    m = 1 + seed % 3
    ref_alphabet = [b"ACGT", b"AC", b"ACG"][(seed // 3) % 3]
    refs = [_dna(rng, int(rng.integers(0, 12)), ref_alphabet) for _ in range(m)]
    if not any(refs):
        refs[int(rng.integers(m))] = b"A"
    block = b"".join(refs)
    k = int(rng.integers(0, 7))
    targets = []
    for _ in range(k):
        kind = int(rng.integers(4))
        n = int(rng.integers(0, 16))
        if kind == 0:
            t = _dna(rng, n)
        elif kind == 1:
            a = int(rng.integers(0, len(block)))
            t = block[a:a + n] + _dna(rng, int(rng.integers(0, 3)))
        elif kind == 2:
            a = int(rng.integers(0, len(block)))
            t = model.revcomp(block[a:a + n]) + _dna(rng, int(rng.integers(0, 3)))
        else:
            t = b""
        targets.append(t.lower() if rng.integers(5) == 0 else t)
    if seed % 3 == 0 and k:  # an empty target in a chosen position: first, last, doubled in the middle
        where = (seed // 3) % 4
        if where == 0:
            targets[0] = b""
        elif where == 1:
            targets[-1] = b""
        elif where == 2:
            targets[k // 2:k // 2] = [b"", b""]
        else:
            targets = [b""] + targets + [b""]
    if seed % 10 == 9:
        targets = [b""] * (1 + seed % 4)
    return refs, targets, bool(seed % 2), int(rng.integers(0, len(targets) + 1))


def _check(rlz, refs, targets, with_rc, cut, parse=model.brute_parse):
    arc = am.ArchiveModel(refs)
    arc.append(targets[:cut], with_rc, parse)
    arc.append(targets[cut:], with_rc, parse)
    rows = _rows(rlz, refs, targets, with_rc)
    block, records, lengths = rlz.absolute_records(refs, rows)
    got, literals = arc.export()
    assert arc.block_length == len(block) and arc.lengths == lengths == [len(t) for t in targets]
    assert got.tobytes() == records.tobytes() and got.dtype == records.dtype, "record for record, byte for byte"
    assert literals == b"".join(rlz.rlz_literals(targets, rows))
    # the sample of both appends is the sample of the whole: entry s = the last record with start <= 256 s
    starts = arc.records["start"].astype(np.int64)
    assert len(arc.sample) == -(-arc.decoded // am.SAMPLE)
    for s, r in enumerate(arc.sample.tolist()):
        assert starts[r] <= am.SAMPLE * s and (r + 1 == len(starts) or starts[r + 1] > am.SAMPLE * s)
    return arc


@pytest.mark.parametrize("chunk", range(10))
def test_model_equals_absolute_records(rlz, chunk):
    empties = 0
    for seed in range(30 * chunk, 30 * chunk + 30):  # 300 seeded cases
        refs, targets, with_rc, cut = _case(seed)
        _check(rlz, refs, targets, with_rc, cut)
        empties += any(len(t) == 0 for t in targets)
    assert empties >= 5


def test_model_cases_cover_what_they_claim():
    cases = [_case(seed) for seed in range(300)]
    assert {len(c[0]) for c in cases} == {1, 2, 3}
    assert {c[2] for c in cases} == {True, False}
    assert any(c[1] and not any(c[1]) for c in cases), "batches of empty targets only"
    assert any(c[1] and c[1][0] == b"" and any(c[1]) for c in cases) and any(c[1] and c[1][-1] == b"" and any(c[1]) for c in cases)
    assert any(any(a == b"" and b == b"" for a, b in zip(c[1][1:-1], c[1][2:-1])) for c in cases if len(c[1]) > 3)
    assert any(not c[1] for c in cases), "k == 0"


def test_model_sample_across_appends(rlz):
    """targets long enough for several sample entries per append, seams off and on multiples of 256"""
    rng = np.random.default_rng(5)
    refs = [_dna(rng, 600), _dna(rng, 200, b"AC")]
    block = b"".join(refs)
    for first in (0, 255, 256, 257, 512):
        long_copy = block[10:10 + 290]
        literals = b"GT" * 150  # short copies and literals
        targets = [block[:first], long_copy, model.revcomp(block[300:480]) + literals, b"", _dna(rng, 300)]
        arc = _check(rlz, refs, targets, True, 1)
        assert arc.decoded == first + 290 + 480 + 300 and len(arc.sample) == -(-arc.decoded // 256)


def test_model_takes_the_parse_of_the_index_model(rlz):
    refs = [b"ACGGTCATTG", b"", b"TTGACC"]
    targets = [b"GGTCAT", b"", model.revcomp(b"CATTG") + b"A", b"GGTCAA"]
    for with_rc in (True, False):
        ix = IndexModel(refs, with_rc)
        _check(rlz, refs, targets, with_rc, 2, parse=lambda r, t, w: ix.parse(t))


def test_export_of_hand_records():
    resident = np.array([(0, 4, 0, am.FORWARD), (4, 1, 0, am.LITERAL | (ord("G") << 8)), (5, 3, 6, am.RC)], dtype=am.ARCHIVE_DTYPE)
    recs, lits = am.export(10, resident)
    assert recs.tolist() == [(10, 4, 0), (14, 1, 14), (15, 3, 4 | am.RC_MASK)] and lits == b"G"


# ---- the id rules of append (pure Python) -----------------------------------------------------------------------------
def test_append_id_rules(rlz):
    chk = rlz._check_append_ids
    assert chk(None, None, 3) is None
    assert chk([], ["a", b"b"], 2) == ["a", "b"]
    assert chk(["a"], ["b", "c"], 2) == ["b", "c"]
    assert chk(["a"], [], 0) == []
    with pytest.raises(ValueError, match="carries no ids"):
        chk(None, ["a"], 1)
    with pytest.raises(ValueError, match="carries ids"):
        chk([], None, 1)
    with pytest.raises(ValueError, match="2 ids for 3 targets"):
        chk([], ["a", "b"], 3)
    with pytest.raises(ValueError, match="distinct"):
        chk([], ["a", "a"], 2)
    with pytest.raises(ValueError, match="distinct.*'a' is in the archive"):
        chk(["a", "z"], ["b", b"a"], 2)
    with pytest.raises(ValueError, match="NUL"):
        chk([], ["a\0"], 1)


def test_from_index_refuses_ids_before_the_device(rlz):
    with pytest.raises(ValueError, match="ids must be None or empty"):
        rlz.RlzArchive.from_index(None, ids=["a"])  # (the index is never looked at)


# ---- batch planning against the room left ------------------------------------------------------------------------------
def test_plan_append_batches(rlz):
    plan, ref = rlz._plan_append_batches, rlz.plan_index_batches
    rng = np.random.default_rng(3)
    for _ in range(50):  # with room to spare it is plan_index_batches
        lengths = [int(x) for x in rng.integers(0, 50, int(rng.integers(0, 30)))]
        bb = [None, 40, 100][int(rng.integers(3))]
        assert plan(lengths, 10, 0, 10**6, bb) == ref(lengths, 10, 10**6, bb)
        assert plan(lengths, 10, 777, 10**6, bb) == ref(lengths, 10, 10**6, bb)
    assert plan([], 5, 0) == []
    # limit 100, 60 decoded: 40 left.  The batch closes in front of the target that no longer fits, and that target goes
    # alone: everything that fits is appended before the library refuses the rest
    assert plan([10, 20, 15, 5], 3, 60, 100) == [(0, 2), (2, 3), (3, 4)]
    assert plan([10, 20, 10], 3, 60, 100) == [(0, 3)]
    assert plan([50], 3, 60, 100) == [(0, 1)]
    assert plan([0, 0, 0], 3, 100, 100) == [(0, 3)]
    assert plan([30, 30], 3, 60, 100, batch_bases=30) == [(0, 1), (1, 2)]
    for lo, hi in plan([5] * 20, 3, 0, 10**6, batch_bases=12):
        assert hi - lo == 2
    # the library's own rule with the real limit: lengths only
    big = rlz.MAX_TEXT - 100
    assert plan([big - 50, 10, 200], 20, 0) == [(0, 2), (2, 3)]
    assert plan([10, big], 20, 200) == [(0, 1), (1, 2)]
