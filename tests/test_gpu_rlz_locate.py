"""Pattern count and locate on the relative-LZ index, on the device (rlz_locate.hip, rlz_index_query_api.hip).  Every
case compares count and locate with the brute force of the definition (tests/rlz_locate_model.brute_locate: bytes.find
per record and strand) by integer equality: counts, offsets, and every hit field in the stated order."""
import random
import threading

import numpy as np
import pytest

import rlz_locate_model as lm
import rlz_model as model

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
    return b"ACGT"[(b"ACGT".index(base) + 1) % 4]


def expected(refs, patterns, with_rc, max_hits=0):
    """dict as RlzIndex.locate returns it, from the brute force"""
    starts = lm.record_starts(refs)
    counts, offsets, hits = [], [0], []
    for p in patterns:
        h = lm.brute_locate(refs, p, with_rc)
        counts.append(len(h))
        if max_hits == 0 or len(h) <= max_hits:
            hits += h
        offsets.append(len(hits))
    return {"counts": np.array(counts, dtype=np.uint64), "offsets": np.array(offsets, dtype=np.uint64),
            "position": np.array([h[0] for h in hits], dtype=np.uint64),
            "record": np.array([h[1] for h in hits], dtype=np.uint32),
            "record_offset": np.array([h[0] - starts[h[1]] for h in hits], dtype=np.uint64),
            "is_rc": np.array([h[2] for h in hits], dtype=bool)}


def check_query(ix, refs, patterns, with_rc, max_hits=0):
    exp = expected(refs, patterns, with_rc, max_hits)
    counts = ix.count(patterns)
    assert counts.dtype == np.uint64 and np.array_equal(counts, exp["counts"]), "count"
    got = ix.locate(patterns, max_hits=max_hits)
    assert sorted(got) == sorted(exp)
    for key, e in exp.items():
        assert got[key].dtype == e.dtype, key
        if not np.array_equal(got[key], e):
            j = int(np.flatnonzero(got["counts"] != exp["counts"])[0]) if key == "counts" else None
            raise AssertionError(f"{key} differs (max_hits {max_hits}, first pattern {j}): {got[key][:16]} != {e[:16]}")
    return got


def check(rlz, refs, patterns, with_rc, prefix_syms=0, max_hits=0):
    with rlz.RlzIndex.build(refs, with_rc=with_rc, prefix_syms=prefix_syms) as ix:
        return check_query(ix, refs, patterns, with_rc, max_hits)


# ---- 1. hand cases ---------------------------------------------------------------------------------------------------
R1 = b"ACGGTCATTGCAAGCTTAGGCATCGA"
R2 = b"TTGACCGGTAAGGCCTTTAGACCA"
R3 = b"GGTAAGGCATCGA"  # ends like R1, starts inside R2
R4 = b"CC" + R2[-7:] + b"GT"  # the end of R2 inside another record


@pytest.mark.parametrize("with_rc", [True, False])
def test_hand_cases(rlz, with_rc):
    got = check(rlz, [R1], [R1, model.revcomp(R1)], with_rc)  # the whole reference, and its reverse complement
    assert got["counts"].tolist() == ([1, 1] if with_rc else [1, 0])
    assert got["position"].tolist() == ([0, 0] if with_rc else [0]) and got["is_rc"].tolist() == ([False, True] if with_rc else [False])
    site = b"GAATTC"  # its own reverse complement: both strands, both at position 2, forward first
    got = check(rlz, [b"CC" + site + b"CC"], [site], with_rc)
    assert got["counts"].tolist() == [2 if with_rc else 1]
    assert got["position"].tolist() == [2, 2][:2 if with_rc else 1] and got["is_rc"].tolist() == [False, True][:2 if with_rc else 1]
    refs = [R1, R2, R3, R4]
    patterns = [R1[-5:] + R2[:5],        # spans R1 | R2: no hit
                R2,                      # a whole record
                R3[-8:],                 # a record's suffix that also ends R1
                R3[:7],                  # a record's prefix that occurs inside R2
                R1 + b"A",               # longer than every record
                b"A", b"C", b"G", b"T",  # the single bases
                b"", b"GGC", b"",        # empty patterns between others
                b"ggtaagg", b"GgCaTc",   # lower case
                b"AGG", b"AGG", b"AGG",  # the same pattern three times
                model.revcomp(R2[4:15]),
                R2[-7:]]                 # a record's suffix that also occurs inside another record
    got = check(rlz, refs, patterns, with_rc)
    assert got["counts"][0] == 0 and got["counts"][4] == 0 and got["counts"][9] == 0 and got["counts"][11] == 0
    assert got["counts"][1] == 1 and got["counts"][2] == 2 and got["counts"][3] == 2
    assert got["counts"][14] == got["counts"][15] == got["counts"][16] > 0
    lo = int(got["offsets"][18])
    assert got["counts"][18] == 2 and got["record"][lo:lo + 2].tolist() == [1, 3] and not got["is_rc"][lo:lo + 2].any()
    check(rlz, refs, patterns, with_rc, max_hits=2)


# ---- 2. geometry -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_rc", [True, False])
@pytest.mark.parametrize("P", [1, 4, 7])
def test_lengths_around_the_table_key(rlz, P, with_rc):
    refs = [_dna(150, 11), b"", _dna(90, 12, b"AC"), _dna(9, 13)]
    patterns = []
    for j, m in enumerate((P - 1, P, P + 1) * 6):
        r = refs[(0, 2, 3)[j % 3]]
        a = (j * 13) % (len(r) - m + 1)
        p = r[a:a + m]
        patterns += [p, model.revcomp(p), p[:-1] + bytes([_other(p[-1])]) if p else p, r[len(r) - m:]]
    check(rlz, refs, patterns, with_rc, prefix_syms=P)


@pytest.mark.parametrize("with_rc", [True, False])
def test_word_edges_and_the_comparison_step(rlz, with_rc):
    refs = [_dna(420, 21), _dna(300, 22)]
    patterns = []
    for j, m in enumerate((31, 32, 33, 63, 64, 65, 127, 128, 129, 257)):
        r = refs[j % 2]
        for a in ((j * 7) % (len(r) - m + 1), len(r) - m):  # somewhere, and ending exactly at the record's end
            p = r[a:a + m]
            patterns += [p, p[:-1] + bytes([_other(p[-1])]), model.revcomp(p)]  # present, absent by its last base
    got = check(rlz, refs, patterns, with_rc)
    assert got["counts"][0::3].min() >= 1 and got["counts"][1::3].max() == 0


@pytest.mark.parametrize("with_rc", [True, False])
@pytest.mark.parametrize("P", [0, 2, 7])
def test_runs_of_a_at_record_ends_and_all_t_patterns(rlz, P, with_rc):
    # the zero padding of the packed text reads as A: records (the last one, and the mirror's last one) ending in A's
    refs = [b"TTTTTCGTAAAA", b"GGAAA", b"TTTTTTTTTTTTTTT", b"AAAAAAAAAAAAAAAAAA", b"TTCAAAAA"]
    patterns = [b"A" * k for k in range(1, 21)] + [b"T" * k for k in range(1, 18)]
    patterns += [b"GTAAAA", b"GTAAAAA", b"GAAA", b"GAAAA", b"CAAAAA", b"CAAAAAA", b"CAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAA",
                 b"TTTTTCG", b"TTTTTTCG", b"TTTACG", b"TTTTACG", b"AAAAACGA", b"CGAAAAA", b"TTTTTG", b"TTTTTTTTTTTTTTTG"]
    check(rlz, refs, patterns, with_rc, prefix_syms=P)
    check(rlz, refs[:1], patterns, with_rc, prefix_syms=P)
    check(rlz, [refs[4], refs[2]], patterns, with_rc, prefix_syms=P)


@pytest.mark.parametrize("with_rc", [True, False])
@pytest.mark.parametrize("records", [1, 2, 5, 64])
def test_record_counts_and_the_mirrored_record_order(rlz, records, with_rc):
    rng = random.Random(500 + records)
    refs = lm.case(rng, hi=30, records=records)
    if records >= 5:
        refs[1] = b""
        refs[-2] = b""
    patterns = lm.patterns(rng, refs, 300)
    got = check(rlz, refs, patterns, with_rc)
    assert len(set(got["record"].tolist())) >= min(records, 3) - 1
    if with_rc:
        assert got["is_rc"].any() and not got["is_rc"].all()


# ---- 3. many hits ----------------------------------------------------------------------------------------------------
BLOCK60 = _dna(60, 31)
MANY = {
    "a3000": ([b"A" * 3000], [b"A", b"AA", b"A" * 100, b"A" * 2999, b"A" * 3000, b"A" * 3001, b"T", b"TTT", b"AC"]),
    "ac1500": ([b"AC" * 1500], [b"AC", b"CA", b"ACAC", b"CACACACACACACACACACACACACACACACACACACACA", b"GT", b"TGT", b"AA", b"C"]),
    "block40": ([BLOCK60 * 40], [BLOCK60, BLOCK60[10:40], model.revcomp(BLOCK60), BLOCK60[50:] + BLOCK60[:10], BLOCK60 * 40,
                                 BLOCK60[:30] + b"A"]),
}


@pytest.mark.parametrize("with_rc", [True, False])
@pytest.mark.parametrize("name", sorted(MANY))
def test_many_hits_and_the_cap(rlz, name, with_rc):
    refs, patterns = MANY[name]
    with rlz.RlzIndex.build(refs, with_rc=with_rc) as ix:
        got = check_query(ix, refs, patterns, with_rc)
        assert int(got["counts"].max()) >= 40
        for c in sorted({int(c) for c in got["counts"] if c > 1}):
            for cap in (c - 1, c, c + 1):  # a batch that mixes capped and uncapped patterns: the offsets skip the capped
                capped = check_query(ix, refs, patterns, with_rc, max_hits=cap)
                assert int(capped["offsets"][-1]) == sum(int(x) for x in got["counts"] if x <= cap)
        one = [patterns[int(np.argmax(got["counts"]))]]
        c = int(got["counts"].max())
        assert len(check_query(ix, refs, one, with_rc, max_hits=c - 1)["position"]) == 0
        assert len(check_query(ix, refs, one, with_rc, max_hits=c)["position"]) == c
        assert len(check_query(ix, refs, one, with_rc, max_hits=0)["position"]) == c


@pytest.mark.parametrize("chunk", [1, 7, 64])
def test_chunk_seams_inside_one_patterns_hits(rlz, monkeypatch, chunk):
    refs = [BLOCK60 * 20, _dna(300, 32, b"AC"), BLOCK60[5:45] * 3]
    patterns = [BLOCK60[:20], b"AC", b"", BLOCK60[30:50], b"CA", model.revcomp(BLOCK60[8:30]), b"A", b"GT", b"ACA"]
    exp = expected(refs, patterns, True)
    assert 1000 <= int(exp["offsets"][-1]) <= 6000
    with rlz.RlzIndex.build(refs) as ix:
        whole = check_query(ix, refs, patterns, True)
        monkeypatch.setenv("NOLZSS_RLZ_LOCATE_CHUNK", str(chunk))
        cut = check_query(ix, refs, patterns, True)
        assert all(np.array_equal(whole[k], cut[k]) for k in whole)
        from nolzss_amd import _noLZSS as native
        native.profile_enable(True)
        try:
            native.profile_reset()
            ix.locate(patterns)
            report = native.profile_report()
        finally:
            native.profile_enable(False)
            native.profile_reset()
        total = int(exp["offsets"][-1])  # the knob is read on every call: one unpack launch and one download per chunk
        assert report["rlz_index_hit_records"][0] == report["hits_d2h"][0] == -(-total // chunk)
        assert report["rlz_index_pattern"][0] == report["rlz_index_hits"][0] == report["rlz_index_locate"][0] == 1
        check_query(ix, refs, patterns, True, max_hits=100)


# ---- 4. seeded batches -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed, hi, with_rc", [(1, 80, True), (2, 250, False), (3, 800, True), (4, 500, True), (5, 90, False)])
def test_seeded_batches(rlz, seed, hi, with_rc):
    rng = random.Random(seed)
    refs = lm.case(rng, lo=hi // 2, hi=hi, records=5 if hi >= 250 else None)
    while not 200 <= sum(map(len, refs)) <= 4000:
        refs = lm.case(rng, lo=hi // 2, hi=hi, records=5)
    patterns = lm.patterns(rng, refs, 2000, longest=12 if hi < 250 else 40)
    got = check(rlz, refs, patterns, with_rc)
    assert (got["counts"] > 0).mean() >= 0.3
    check(rlz, refs, patterns, with_rc, max_hits=8)


def test_a_pattern_list_in_several_batches(rlz, monkeypatch):
    refs = [R1, R2, R3]
    patterns = [b"AGG", b"", R2[3:9], b"TTTTT", b"GC", b"A", model.revcomp(R1[4:9]), b"CATCGA"]
    with rlz.RlzIndex.build(refs) as ix:
        whole = check_query(ix, refs, patterns, True, max_hits=9)
        monkeypatch.setattr(rlz, "MAX_TEXT", 12)  # sum(len) + q <= 12 per batch: several batches, the offsets stitched
        assert len(ix._pattern_batches(patterns)[1]) >= 3
        cut = check_query(ix, refs, patterns, True, max_hits=9)
        assert all(np.array_equal(whole[k], cut[k]) for k in whole)
        assert ix.count([]).tolist() == [] and ix.locate([])["offsets"].tolist() == [0]


# ---- 5. other behaviour ------------------------------------------------------------------------------------------------
def test_two_threads_query_one_handle(rlz):
    rng = random.Random(77)
    refs = lm.case(rng, lo=100, hi=300, records=4)
    batches = [lm.patterns(rng, refs, 400), lm.patterns(rng, refs, 400)]
    with rlz.RlzIndex.build(refs) as ix:
        single = [ix.locate(b, max_hits=50) for b in batches]
        out, errors = [[None] * 6, [None] * 6], []

        def work(t):
            try:
                for rep in range(6):
                    out[t][rep] = ix.locate(batches[t], max_hits=50)
                    assert np.array_equal(ix.count(batches[t]), single[t]["counts"])
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
        e = expected(refs, batches[t], True, 50)
        assert all(np.array_equal(single[t][k], e[k]) for k in e)


def test_refusals(rlz):
    ix = rlz.RlzIndex.build([R1, R2])
    with pytest.raises(RuntimeError, match="Invalid nucleotide 'N' found in pattern 2"):
        ix.count([b"ACG", b"", b"ACNT"])
    with pytest.raises(RuntimeError, match="Invalid nucleotide 'x' found in pattern 0"):
        ix.locate([b"xA", b"N"])
    with pytest.raises(ValueError, match="max_hits"):
        ix.locate([b"A"], max_hits=-1)
    assert ix.count([b"GG"]).tolist() == [len(lm.brute_locate([R1, R2], b"GG"))]  # (the handle is still good)
    ix.close()
    with pytest.raises(ValueError, match="closed"):
        ix.count([b"ACG"])
    with pytest.raises(ValueError, match="closed"):
        ix.locate([b"ACG"])


def test_a_total_beyond_the_pipeline_is_refused_before_anything_is_expanded(rlz):
    ref = _dna(1 << 16, 41)
    per = len(lm.brute_locate([ref], b"A", True))
    q = rlz.MAX_TEXT // per + 2
    assert q < 200_000
    with rlz.RlzIndex.build(ref) as ix:
        with pytest.raises(ValueError, match=rf"locate would report {q * per} hits.*max_hits"):
            ix.locate([b"A"] * q)
        got = ix.locate([b"A"] * q, max_hits=per - 1)  # every pattern capped: counts, and no hits
        assert got["counts"].tolist() == [per] * q and got["offsets"].tolist() == [0] * (q + 1) and len(got["position"]) == 0
        assert len(ix.locate([b"A"] * 3)["position"]) == 3 * per


def test_the_handle_is_untouched_by_a_query(rlz):
    rng = random.Random(91)
    refs = lm.case(rng, lo=150, hi=400, records=3)
    targets = [refs[0][20:120] + model.revcomp(refs[-1] or refs[0])[:80], b"", refs[0][::-1]]
    patterns = lm.patterns(rng, refs, 500)
    with rlz.RlzIndex.build(refs) as ix:
        before = ix.factorize(targets)
        info = ix.info()
        check_query(ix, refs, patterns, True)
        check_query(ix, refs, patterns, True, max_hits=3)
        after = ix.factorize(targets)
        assert ix.info() == info and len(before) == len(after)
        assert all(np.array_equal(a, b) for a, b in zip(before, after))


def _profiled(native, fn):
    native.profile_enable(True)
    try:
        native.profile_reset()
        out = fn()
        return out, native.profile_report()
    finally:
        native.profile_enable(False)
        native.profile_reset()


def test_the_patterns_are_searched_again_when_the_arena_grows_for_the_hits(rlz):
    """an open leaves the arena empty: the first locate reserves for the batch, learns the number of hits, reserves
    again -- the slab is replaced -- and runs the pattern kernel a second time in it; the next call finds room"""
    from nolzss_amd import _noLZSS as native
    refs = [BLOCK60 * 20, _dna(300, 51)]
    patterns = [BLOCK60[:12], b"AC", model.revcomp(BLOCK60[20:40]), b"", b"G"]
    exp = expected(refs, patterns, True)
    with rlz.RlzIndex.build(refs) as ix:
        native.debug_trim_arenas()
        first, report = _profiled(native, lambda: ix.locate(patterns))
        assert report["rlz_index_pattern"][0] == 2 and report["rlz_index_hits"][0] == 1
        again, report = _profiled(native, lambda: ix.locate(patterns))
        assert report["rlz_index_pattern"][0] == 1
        for got in (first, again):
            assert all(np.array_equal(got[k], exp[k]) for k in exp)


def test_more_than_2_to_the_24_patterns_in_one_batch(rlz):
    """the pattern index reaches bit 57 of the sort key: the digit at bit 56 runs.  Three one-base patterns in turn, one
    hit each, so any hit that left its pattern's segment shows in the positions"""
    import ctypes as C
    from nolzss_amd import _lib
    q = (1 << 24) + 2
    bases = [C.create_string_buffer(b) for b in (b"A", b"G", b"T")]
    ptrs = np.array([C.addressof(b) for b in bases], dtype=np.uint64)[np.arange(q) % 3]
    lens = np.ones(q, dtype=np.uint64)
    counts, offsets = np.zeros(q, dtype=np.uint64), np.zeros(q + 1, dtype=np.uint64)
    out, z = C.c_void_p(), C.c_size_t()
    with rlz.RlzIndex.build(b"CAGT", with_rc=False) as ix:
        rc = _lib.lib.nolzss_rlz_index_locate(ix._live()._handle(), ptrs.ctypes.data_as(C.POINTER(C.c_char_p)),
                                              lens.ctypes.data_as(C.POINTER(C.c_size_t)), q, 0, counts.ctypes.data,
                                              offsets.ctypes.data, C.byref(out), C.byref(z))
        message = _lib.lib.nolzss_last_error()
    try:
        assert rc == _lib.OK, message
        assert z.value == q and (counts == 1).all() and np.array_equal(offsets, np.arange(q + 1, dtype=np.uint64))
        hits = np.ctypeslib.as_array(C.cast(out, C.POINTER(C.c_uint64)), shape=(2 * q,)).view(rlz.HIT_DTYPE)
        assert np.array_equal(hits["position"], (1 + np.arange(q) % 3).astype(np.uint64))
        assert not hits["record"].any() and not hits["is_rc"].any()
    finally:
        _lib.lib.nolzss_free(out)
