"""Maximal match seeds on the relative-LZ index, on the device (rlz_seeds.hip, rlz_index_seeds_api.hip).  Every case
compares RlzIndex.seeds with tests/rlz_seeds_model.expected -- the ms formulation over bytes.find, the hits from the
brute force of a locate -- by integer equality of every field: target, start, length, counts, offsets, and every hit field in order."""
import ctypes as C
import random
import threading

import numpy as np
import pytest

import rlz_locate_model as lm
import rlz_model as model
import rlz_seeds_model as sm

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rlz():
    from nolzss_amd import _noLZSS
    assert _noLZSS.device_count() >= 1, "no MI355X visible"
    from nolzss_amd.genomics import rlz
    return rlz


def _dna(n, seed, alphabet=b"ACGT"):
    rng = np.random.default_rng(seed)
    return np.frombuffer(alphabet, dtype=np.uint8)[rng.integers(0, len(alphabet), n)].tobytes()


def _other(base):
    return bytes([b"ACGT"[(b"ACGT".index(base) + 1) % 4]])


def same(got, exp):
    assert sorted(got) == sorted(exp)
    for key, e in exp.items():
        assert got[key].dtype == e.dtype, key
        if not np.array_equal(got[key], e):
            raise AssertionError(f"{key} differs: {len(got[key])} entries {got[key][:16]} != {len(e)} entries {e[:16]}")


def check_query(ix, refs, targets, with_rc, min_length=1, max_hits=0):
    got = ix.seeds(targets, min_length=min_length, max_hits=max_hits)
    same(got, sm.expected(refs, targets, with_rc, min_length, max_hits))
    return got


def check(rlz, refs, targets, with_rc, prefix_syms=0, **kw):
    with rlz.RlzIndex.build(refs, with_rc=with_rc, prefix_syms=prefix_syms) as ix:
        return check_query(ix, refs, targets, with_rc, **kw)


def triples(got):
    return list(zip(got["target"].tolist(), got["start"].tolist(), got["length"].tolist()))


def _profiled(fn):
    from nolzss_amd import _noLZSS as native
    native.profile_enable(True)
    try:
        native.profile_reset()
        out = fn()
        return out, native.profile_report()
    finally:
        native.profile_enable(False)
        native.profile_reset()


# ---- 1. hand cases ---------------------------------------------------------------------------------------------------
R1 = b"ACGGTCATTGCAAGCTTAGGCATCGA"
R2 = b"TTGACCGGTAAGGCCTTTAGACCA"


@pytest.mark.parametrize("with_rc", [True, False])
def test_hand_cases(rlz, with_rc):
    refs = [R1, R2]
    with rlz.RlzIndex.build(refs, with_rc=with_rc) as ix:
        got = check_query(ix, refs, [R1], with_rc)  # a whole record: one seed of its length
        assert triples(got) == [(0, 0, len(R1))] and got["counts"].tolist() == [1] and got["position"].tolist() == [0]
        got = check_query(ix, refs, [R1 + R2], with_rc)  # no seed crosses the record boundary
        assert (0, 0, len(R1)) in triples(got) and (0, len(R1), len(R2)) in triples(got)
        assert int(got["length"].max()) == len(R1)
        got = check_query(ix, refs, [model.revcomp(R1)], with_rc)
        if with_rc:
            assert triples(got) == [(0, 0, len(R1))] and got["is_rc"].tolist() == [True] and got["position"].tolist() == [0]
        else:
            assert int(got["length"].max()) < len(R1)
        # targets of length 1 and 0 between others; a seed at the first and at the last batch position; lower case
        got = check_query(ix, refs, [R1[:9], b"", b"G", b"", R2[3:11].lower(), b"t", R1[-6:], b"c"], with_rc)
        assert got["target"].tolist() == [0, 2, 4, 5, 6, 7] and got["start"].tolist() == [0] * 6
        assert got["length"].tolist() == [9, 1, 8, 1, 6, 1]
        assert ix.seeds([])["offsets"].tolist() == [0] and ix.seeds([b"", b""])["offsets"].tolist() == [0]
        assert len(ix.seeds([b"", b""])["target"]) == 0
    # no base of the reference's alphabet: no seeds (without reverse complement T does not match A either)
    got = check(rlz, [b"AAAAAAAA", b"AAA"], [b"CCGCG", b"GG"] + ([] if with_rc else [b"TTT"]), with_rc)
    assert len(got["target"]) == 0 and got["offsets"].tolist() == [0] and len(got["position"]) == 0


@pytest.mark.parametrize("with_rc", [True, False])
def test_the_separator_breaks_a_match_between_adjacent_targets(rlz, with_rc):
    refs = [R1, R2]
    got = check(rlz, refs, [b"C" + R1[:13], R1[13:] + b"C", R2[:10], R2[10:]], with_rc)
    assert (0, 1, 13) in triples(got) and (1, 0, 13) in triples(got) and (2, 0, 10) in triples(got)
    assert int(got["length"].max()) == len(R2) - 10


@pytest.mark.parametrize("with_rc", [True, False])
def test_a_site_that_is_its_own_reverse_complement(rlz, with_rc):
    site = b"GAATTC"
    got = check(rlz, [b"CC" + site + b"CC"], [b"T" + site + b"A"], with_rc)
    j = triples(got).index((0, 1, 6))
    lo, hi = int(got["offsets"][j]), int(got["offsets"][j + 1])
    assert got["position"][lo:hi].tolist() == [2, 2][:2 if with_rc else 1]
    assert got["is_rc"][lo:hi].tolist() == [False, True][:2 if with_rc else 1] and got["counts"][j] == hi - lo


# ---- 2. geometry of the search the seeds rest on ---------------------------------------------------------------------
@pytest.mark.parametrize("with_rc", [True, False])
@pytest.mark.parametrize("P", [1, 4, 7, 0])
def test_lengths_around_the_table_key(rlz, P, with_rc):
    refs = [_dna(150, 11), b"", _dna(90, 12, b"AC"), _dna(9, 13)]
    with rlz.RlzIndex.build(refs, with_rc=with_rc, prefix_syms=P) as ix:
        key = ix.info()["prefix_syms"]
        assert key == (P or 4)
        targets = []
        for j, m in enumerate((key - 1, key, key + 1) * 6):
            r = refs[(0, 2, 3)[j % 3]]
            r = r if len(r) >= m + 3 else refs[0]
            a = 1 + (j * 13) % (len(r) - m - 1)
            p = r[a:a + m]  # a cut whose neighbours in the target are not its neighbours in the record
            targets += [_other(r[a - 1]) + p + _other(r[a + m]), p, model.revcomp(p), r[len(r) - m:], r[:max(key - 2, 0)]]
        got = check_query(ix, refs, targets, with_rc)
        assert {key - 1, key, key + 1} - {0} <= set(got["length"].tolist())
        check_query(ix, refs, targets, with_rc, min_length=key, max_hits=3)


@pytest.mark.parametrize("with_rc", [True, False])
def test_word_edges(rlz, with_rc):
    refs = [_dna(420, 21), _dna(300, 22)]
    targets, want = [], []
    for j, m in enumerate((31, 32, 33, 63, 64, 65, 127, 128, 129, 257)):
        r = refs[j % 2]
        a = len(r) - m  # the seed ends exactly at the record's end, and at its target's end
        targets += [_other(r[a - 1]) + r[a:], r[a:] + b"A", _other(r[a - 1]) + model.revcomp(r[a:])]
        want += [(3 * j, 1, m), (3 * j + 1, 0, m)] + ([(3 * j + 2, 1, m)] if with_rc else [])
    got = check(rlz, refs, targets, with_rc)
    assert set(want) <= set(triples(got))


# ---- 3. runs, many hits and the cap ----------------------------------------------------------------------------------
@pytest.mark.parametrize("with_rc", [True, False])
def test_runs(rlz, with_rc):
    refs = [b"A" * 3000]
    targets = [b"A" * 10, b"A" * 3000, b"A" * 3001, b"T" * 7, b"AC"]
    with rlz.RlzIndex.build(refs, with_rc=with_rc) as ix:
        got = check_query(ix, refs, targets, with_rc)
        # one seed per target -- and the two ends of the run that is one base longer than the record
        exp = [(0, 0, 10), (1, 0, 3000), (2, 0, 3000), (2, 1, 3000)] + ([(3, 0, 7)] if with_rc else []) + [(4, 0, 1)]
        assert triples(got) == exp
        assert got["counts"].tolist() == [3000 - L + 1 for _, _, L in exp]
        if with_rc:
            j = exp.index((3, 0, 7))
            assert got["is_rc"][int(got["offsets"][j]):int(got["offsets"][j + 1])].all()
        assert int(got["is_rc"].sum()) == (2994 if with_rc else 0)
        check_query(ix, refs, targets, with_rc, max_hits=2991)
        check_query(ix, refs, targets, with_rc, min_length=8, max_hits=1)


@pytest.mark.parametrize("with_rc", [True, False])
def test_the_cap_in_a_batch_of_capped_and_uncapped_seeds(rlz, with_rc):
    refs = [b"AC" * 1500]
    targets = [b"ACACG", b"GCACACACAG", b"AC" * 1500, b"TCAT", b"AA", b"", b"CACACACACACACACACACACACACACACACACACACACAT"]
    with rlz.RlzIndex.build(refs, with_rc=with_rc) as ix:
        got = check_query(ix, refs, targets, with_rc)
        assert len(set(got["counts"].tolist())) >= 4 and int(got["counts"].max()) >= 1499
        for c in sorted({int(c) for c in got["counts"] if c > 1}):
            for cap in (c - 1, c, c + 1):  # the offsets skip the capped seeds
                capped = check_query(ix, refs, targets, with_rc, max_hits=cap)
                assert np.array_equal(capped["counts"], got["counts"])
                assert int(capped["offsets"][-1]) == sum(int(x) for x in got["counts"] if x <= cap)


@pytest.mark.parametrize("with_rc", [True, False])
def test_min_length(rlz, with_rc):
    from nolzss_amd import _noLZSS as native
    rng = random.Random(31)
    refs = lm.case(rng, lo=60, hi=120, records=3)
    targets = sm.targets(rng, refs, 40, longest=30)
    with rlz.RlzIndex.build(refs, with_rc=with_rc) as ix:
        whole = check_query(ix, refs, targets, with_rc)
        longest = int(whole["length"].max())
        assert longest >= 12
        for m in (0, 1, 2, longest // 2, longest):
            got = check_query(ix, refs, targets, with_rc, min_length=m)
            keep = whole["length"] >= max(m, 1)  # the filter never creates a seed
            assert triples(got) == [t for t, k in zip(triples(whole), keep) if k] and len(got["target"]) >= 1
            assert np.array_equal(got["counts"], whole["counts"][keep])
        got, report = _profiled(lambda: check_query(ix, refs, targets, with_rc, min_length=longest + 1))
        assert len(got["target"]) == 0 and got["offsets"].tolist() == [0] and len(got["position"]) == 0
        assert report["rlz_index_search"][0] == report["rlz_seed_flags"][0] == report["rlz_index_seeds"][0] == 1
        for stage in ("rlz_seed_intervals", "rlz_seed_hits", "rlz_seed_sort", "rlz_index_hit_records", "hits_d2h", "seeds_d2h"):
            assert stage not in report or report[stage][0] == 0, stage
        assert native.SEED_DTYPE.itemsize == 32


# ---- 4. geometry of the new kernels ----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def large():
    """one batch of 2^16 + 3 positions: about 400 targets cut from a 3 000-base reference (a block of 200 bases fifteen times
    over, so that every seed has many hits) with 2 % substitutions -> (refs, targets, expected), computed once"""
    rng = np.random.default_rng(61)
    ref = _dna(200, 60) * 15
    lengths = rng.integers(100, 221, size=400)
    rest = (1 << 16) + 3 - 400 - int(lengths.sum())  # spread over the targets so that the batch has exactly that size
    lengths = (lengths + rest // 400 + (np.arange(400) < rest % 400)).tolist()
    assert min(lengths) >= 50 and max(lengths) <= 400
    targets = []
    for n in lengths:
        a = int(rng.integers(0, len(ref) - n))
        t = np.frombuffer(ref[a:a + n], dtype=np.uint8).copy()
        if rng.random() < 0.5:
            t = np.frombuffer(model.revcomp(t.tobytes()), dtype=np.uint8).copy()
        where = rng.random(n) < 0.02
        t[where] = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, int(where.sum()))]
        targets.append(t.tobytes())
    assert sum(map(len, targets)) + len(targets) == (1 << 16) + 3
    return [ref], targets, sm.expected([ref], targets, True)


def test_one_batch_across_workgroups_scan_tiles_and_the_high_sort_digit(rlz, large):
    refs, targets, exp = large
    assert len(exp["target"]) > 256 and len(exp["position"]) > 1 << 16
    with rlz.RlzIndex.build(refs) as ix:
        got = ix.seeds(targets)
        same(got, exp)
        codes = ix.codes(targets)
        first = np.cumsum([0] + [len(t) + 1 for t in targets[:-1]])
        at = first[got["target"].astype(np.int64)] + got["start"].astype(np.int64)
        assert np.array_equal(got["length"], (codes[at] & 0x7fffffff).astype(np.uint64))
        pick = np.arange(len(at))  # every seed's hits are those of a locate of its bytes
        pieces = [targets[int(got["target"][j])][int(got["start"][j]):int(got["start"][j] + got["length"][j])] for j in pick]
        loc = ix.locate(pieces)
        for n, j in enumerate(pick):
            lo, hi = int(got["offsets"][j]), int(got["offsets"][j + 1])
            llo, lhi = int(loc["offsets"][n]), int(loc["offsets"][n + 1])
            assert loc["counts"][n] == got["counts"][j] == hi - lo == lhi - llo
            for key in ("position", "record", "record_offset", "is_rc"):
                assert np.array_equal(got[key][lo:hi], loc[key][llo:lhi]), (key, j)
        same(ix.seeds(targets, min_length=20, max_hits=24), sm.expected(refs, targets, True, 20, 24))


# ---- 5. chunks, the arena, batches, threads ---------------------------------------------------------------------------
BLOCK60 = _dna(60, 31)


@pytest.mark.parametrize("chunk", [1, 7, 64])
def test_chunk_seams(rlz, monkeypatch, chunk):
    refs = [BLOCK60 * 20, _dna(300, 32, b"AC"), BLOCK60[5:45] * 3]
    targets = [b"T" + BLOCK60[:20] + b"G", b"", BLOCK60[30:50] + b"ACACAC" + model.revcomp(BLOCK60[8:30]), b"ACAGT", BLOCK60[40:] + BLOCK60[:9],
               b"A", b"g"]
    exp = sm.expected(refs, targets, True)
    S, T = len(exp["target"]), int(exp["offsets"][-1])
    assert 1000 <= T <= 6000 and S >= 8
    with rlz.RlzIndex.build(refs) as ix:
        whole = ix.seeds(targets)
        same(whole, exp)
        monkeypatch.setenv("NOLZSS_RLZ_LOCATE_CHUNK", str(chunk))
        cut, report = _profiled(lambda: ix.seeds(targets))  # the knob is read on every call
        same(cut, exp)
        assert report["rlz_index_hit_records"][0] == report["hits_d2h"][0] == -(-T // chunk)
        assert report["rlz_seed_intervals"][0] == report["seeds_d2h"][0] == -(-S // chunk)
        assert report["rlz_index_search"][0] == report["rlz_seed_flags"][0] == report["rlz_seed_hits"][0] == 1
        assert report["rlz_seed_sort"][0] == report["rlz_index_seeds"][0] == 1
        same(ix.seeds(targets, min_length=3, max_hits=100), sm.expected(refs, targets, True, 3, 100))


def test_the_batch_is_searched_again_when_the_arena_grows_for_the_hits(rlz):
    """an open leaves the arena empty: the first query reserves for the batch, learns the number of hits, reserves again
    -- the slab is replaced -- and searches the batch a second time in it; the next call finds room"""
    from nolzss_amd import _noLZSS as native
    refs = [BLOCK60 * 20, _dna(300, 51)]
    targets = [BLOCK60[:12] + b"T" + model.revcomp(BLOCK60[20:40]), b"", b"G", BLOCK60[7:33]]
    exp = sm.expected(refs, targets, True)
    assert int(exp["offsets"][-1]) > 0
    with rlz.RlzIndex.build(refs) as ix:
        native.debug_trim_arenas()
        first, report = _profiled(lambda: ix.seeds(targets))
        assert report["rlz_index_search"][0] == 2 and report["rlz_seed_hits"][0] == 1 and report["rlz_seed_flags"][0] == 2
        assert report["seeds_d2h"][0] == 1 and report["rlz_seed_intervals"][0] == 2
        again, report = _profiled(lambda: ix.seeds(targets))
        assert report["rlz_index_search"][0] == 1 and report["rlz_seed_intervals"][0] == 1
        same(first, exp)
        same(again, exp)


def test_a_target_list_in_several_batches(rlz, monkeypatch):
    refs = [R1, R2]
    targets = [R1[3:14], b"", R2[2:9] + b"A", model.revcomp(R1[4:15]), b"G", R2[-9:], b"TTACG"]
    with rlz.RlzIndex.build(refs) as ix:
        whole = check_query(ix, refs, targets, True, max_hits=9)
        monkeypatch.setattr(rlz, "MAX_TEXT", ix.info()["block_length"] + 1 + 22)  # sum(len) + k <= 22 per batch
        assert len(rlz.plan_index_batches([len(t) for t in targets], ix.info()["block_length"], rlz.MAX_TEXT)) >= 3
        cut = check_query(ix, refs, targets, True, max_hits=9)
        assert all(np.array_equal(whole[k], cut[k]) for k in whole)
        assert sorted(set(cut["target"].tolist())) == [0, 2, 3, 4, 5, 6]


def test_two_threads_query_one_handle(rlz):
    rng = random.Random(77)
    refs = lm.case(rng, lo=100, hi=300, records=4)
    batches = [sm.targets(rng, refs, 60, longest=40), sm.targets(rng, refs, 45, longest=25)]
    with rlz.RlzIndex.build(refs) as ix:
        single = [ix.seeds(b, min_length=2, max_hits=50) for b in batches]
        out, errors = [[None] * 6, [None] * 6], []

        def work(t):
            try:
                for rep in range(6):
                    out[t][rep] = ix.seeds(batches[t], min_length=2, max_hits=50)
            except Exception as e:  # noqa: BLE001
                errors.append(e)

        threads = [threading.Thread(target=work, args=(t,)) for t in range(2)]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
        assert not errors, errors
        for t in range(2):
            for got in out[t]:
                assert all(np.array_equal(got[k], single[t][k]) for k in single[t])
    for t in range(2):
        same(single[t], sm.expected(refs, batches[t], True, 2, 50))


# ---- 6. refusals, and the handle -------------------------------------------------------------------------------------
def test_refusals(rlz):
    ix = rlz.RlzIndex.build([R1, R2])
    with pytest.raises(RuntimeError, match="Invalid nucleotide 'N' found in sequence 4"):
        ix.seeds([b"ACG", b"", b"ACNT"])
    with pytest.raises(RuntimeError, match="Invalid nucleotide 'N' found in sequence 4"):
        ix.factorize([b"ACG", b"", b"ACNT"])  # (as a match names it)
    with pytest.raises(ValueError, match="min_length"):
        ix.seeds([b"A"], min_length=-1)
    with pytest.raises(ValueError, match="max_hits"):
        ix.seeds([b"A"], max_hits=-1)
    assert ix.seeds([b"GG"])["counts"].tolist() == [len(lm.brute_locate([R1, R2], b"GG"))]  # (the handle is still good)
    ix.close()
    with pytest.raises(ValueError, match="closed"):
        ix.seeds([b"ACG"])


def test_a_total_beyond_the_pipeline_is_refused_before_anything_is_expanded(rlz):
    from nolzss_amd import _lib
    from nolzss_amd import _noLZSS as native
    ref = _dna(1 << 16, 41)
    per = len(lm.brute_locate([ref], b"A", True))
    q = rlz.MAX_TEXT // per + 2
    assert q < 200_000
    with rlz.RlzIndex.build(ref) as ix:
        with pytest.raises(ValueError, match=rf"seeds would report {q * per} hits.*max_hits.*min_length"):
            ix.seeds([b"A"] * q)
        # the C ABI still returns the seeds and their counts, and no hits
        res = _lib.RlzSeedsResult()
        rc = _lib.lib.nolzss_rlz_index_seeds(ix._live()._handle(), *native._seq_args([b"A"] * q, "target"), 1, 0, C.byref(res))
        try:
            assert rc == _lib.ERR_INVALID_ARGUMENT and res.num_seeds == q and res.num_hits == 0 and not res.hits
            seeds = np.ctypeslib.as_array(C.cast(res.seeds, C.POINTER(C.c_uint64)), shape=(4 * q,)).view(rlz.SEED_DTYPE)
            assert (seeds["count"] == per).all() and np.array_equal(seeds["target"], np.arange(q, dtype=np.uint64))
            offsets = np.ctypeslib.as_array(C.cast(res.hit_offsets, C.POINTER(C.c_uint64)), shape=(q + 1,))
            assert int(offsets[-1]) == q * per
        finally:
            _lib.lib.nolzss_free_rlz_seeds_result(C.byref(res))
        got = ix.seeds([b"A"] * q, max_hits=per - 1)  # every seed capped: counts, and no hits
        assert got["counts"].tolist() == [per] * q and got["offsets"].tolist() == [0] * (q + 1) and len(got["position"]) == 0
        assert got["length"].tolist() == [1] * q and len(ix.seeds([b"A"] * 3)["position"]) == 3 * per


def test_the_handle_is_untouched_by_a_query(rlz):
    rng = random.Random(91)
    refs = lm.case(rng, lo=150, hi=400, records=3)
    targets = [refs[0][20:120] + model.revcomp(refs[-1] or refs[0])[:80], b"", refs[0][::-1]]
    with rlz.RlzIndex.build(refs) as ix:
        before = ix.factorize(targets)
        info = ix.info()
        check_query(ix, refs, targets, True)
        check_query(ix, refs, sm.targets(rng, refs, 30, longest=30), True, min_length=3, max_hits=3)
        after = ix.factorize(targets)
        assert ix.info() == info and len(before) == len(after)
        assert all(np.array_equal(a, b) for a, b in zip(before, after))
