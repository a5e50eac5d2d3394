"""Locate through the parse of a relative-LZ archive, on the device (rlz_find.hip, rlz_find_api.hip; DESIGN.md 5,
"Relative-LZ archive: locate through the parse").  Every case compares count and locate with the brute force of the
definition over the plain targets (tests/rlz_find_model.brute_find) and the `primary` flag with the archive's exported
records, by integer equality of counts, offsets and every hit field in order."""
import ctypes as C
import threading

import numpy as np
import pytest

import genomes
import rlz_find_model as fm

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def native():
    from nolzss_amd import _noLZSS
    assert _noLZSS.device_count() >= 1, "no MI355X visible"
    return _noLZSS


@pytest.fixture(scope="module")
def rlz(native):
    from nolzss_amd.genomics import rlz
    return rlz


KEYS = ("counts", "offsets", "target", "position", "is_rc", "primary")


def same(got, exp, what=""):
    for k in KEYS:
        assert got[k].dtype == exp[k].dtype and np.array_equal(got[k], exp[k]), (what, k)


def check_finder(finder, arc, targets, patterns, with_rc, max_hits=0):
    """count and locate of `patterns` against the model -> the locate's dict"""
    block, records, _ = arc._live().export()
    exp = fm.expected(targets, records, len(block), patterns, with_rc, max_hits)
    got = finder.locate(patterns, max_hits=max_hits)
    same(got, exp, (with_rc, max_hits))
    counts = finder.count(patterns)
    assert counts.dtype == np.uint64 and np.array_equal(counts, exp["counts"])
    return got


def check_kernel(finder, arc, targets, M):
    """nolzss_rlz_finder_kernel against the numpy interval model"""
    block, records, _ = arc._live().export()
    starts = records["start"].astype(np.int64) - len(block)
    K, kstart, dstart = fm.kernel_text(targets, starts, M)
    got = finder.kernel()
    assert got[0] == K and np.array_equal(got[1], kstart) and np.array_equal(got[2], dstart)
    info = finder.info
    assert info["kernel_length"] == len(K) and info["intervals"] == len(kstart) - 1 and info["max_pattern_length"] == M
    assert info["z"] == len(records) and info["num_targets"] == len(targets) and info["device_bytes"] > 0


class Case:
    """an index, an archive of `targets` appended to it, and finders over it"""

    def __init__(self, rlz, refs, targets, with_rc):
        self.refs, self.targets, self.with_rc = refs, [bytes(t).upper() for t in targets], with_rc
        self.ix = rlz.RlzIndex.build(refs, with_rc=with_rc)
        self.arc = self.ix.archive_on_device(targets)

    def run(self, patterns, M, max_hits=0, prefix_syms=0, kernel=True):
        with self.arc.finder(max_pattern_length=M, prefix_syms=prefix_syms) as f:
            assert f.info["with_rc"] == int(self.with_rc)
            if kernel:
                check_kernel(f, self.arc, self.targets, M)
            return check_finder(f, self.arc, self.targets, patterns, self.with_rc, max_hits)

    def close(self):
        self.arc.close()
        self.ix.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def hits_of(got, j):
    lo, hi = int(got["offsets"][j]), int(got["offsets"][j + 1])
    return [(int(got["target"][i]), int(got["position"][i]), int(got["is_rc"][i]), int(got["primary"][i])) for i in range(lo, hi)]


# ---- 1. hand cases -----------------------------------------------------------------------------------------------------
R = fm.dna(np.random.default_rng(11), 60)


@pytest.mark.parametrize("with_rc", [True, False])
def test_hand_cases_inside_copies_and_across_records(rlz, with_rc):
    targets = [R[10:40], fm.revcomp(R[5:45]), R[0:20] + R[44:60]]  # (R[20] != R[44]: the first copy ends at 20)
    joint = targets[2]
    patterns = [R[15:25], fm.revcomp(R[10:30]), R[10:30], joint[19:27], joint[13:21], b"", R[15:25].lower()]
    with Case(rlz, R, targets, with_rc) as c:
        got = c.run(patterns, M=20)
        # inside one forward copy: secondary, on the pattern's own strand
        assert (0, 5, 0, 0) in hits_of(got, 0) and hits_of(got, 6) == hits_of(got, 0)
        if with_rc:
            # target 1 is ONE reverse-complement copy: the pattern cut from it is found forward, its reverse complement
            # (the reference's own strand) as is_rc, both secondary; and R[15:25] inside it on the other strand
            block, records, _ = c.arc._live().export()
            assert sum(1 for r in records if r["ref"] >> 63) >= 1
            assert (1, 15, 0, 0) in hits_of(got, 1) and (1, 15, 1, 0) in hits_of(got, 2)
            assert (1, 20, 1, 0) in hits_of(got, 0)
            assert (0, 0, 1, 0) in hits_of(got, 1) and (0, 0, 0, 0) in hits_of(got, 2)
        else:
            assert all(h[2] == 0 for j in range(len(patterns)) for h in hits_of(got, j))
            assert (1, 15, 0) in [h[:3] for h in hits_of(got, 1)]
        # across the two records of target 2, at split 1 and split m - 1: primary
        assert (2, 19, 0, 1) in hits_of(got, 3) and (2, 13, 0, 1) in hits_of(got, 4)
        assert got["counts"][5] == 0


@pytest.mark.parametrize("with_rc", [True, False])
def test_hand_cases_literal_palindrome_and_target_ends(rlz, with_rc):
    # a single literal with m = 1
    with Case(rlz, b"AAAAAAAAAA", [b"AAGAA", b"G", b""], with_rc) as c:
        got = c.run([b"G", b"C", b"A", b"T"], M=1)
        assert hits_of(got, 0) == [(0, 2, 0, 1), (1, 0, 0, 1)]
        assert hits_of(got, 1) == ([(0, 2, 1, 1), (1, 0, 1, 1)] if with_rc else [])
        assert got["counts"][2] == 4 and got["counts"][3] == (4 if with_rc else 0)
    # a palindromic site: both strands, forward first; an index without reverse complement reports no is_rc hit
    ref = R[:30] + b"GAATTC" + R[30:]
    with Case(rlz, ref, [ref[20:50], b"TT" + ref[28:40]], with_rc) as c:
        got = c.run([b"GAATTC", b"gaattc"], M=6)
        want = [(0, 10, 0, 0), (0, 10, 1, 0), (1, 4, 0), (1, 4, 1)] if with_rc else [(0, 10, 0, 0), (1, 4, 0)]
        assert [h[:len(w)] for h, w in zip(hits_of(got, 0), want)] == want and len(hits_of(got, 0)) == len(want)
        assert hits_of(got, 1) == hits_of(got, 0)
    # the end of target i joined to the start of target i + 1 is no occurrence
    with Case(rlz, R, [R[0:20], R[20:40], b"", R[40:44]], with_rc) as c:
        got = c.run([R[15:25], R[17:23], R[36:43], R[16:20], R[20:24]], M=10)
        assert got["counts"][:3].tolist() == [0, 0, 0]
        assert (0, 16, 0) in [h[:3] for h in hits_of(got, 3)] and (1, 0, 0) in [h[:3] for h in hits_of(got, 4)]


# ---- 2. exhaustive -----------------------------------------------------------------------------------------------------
def exhaustive_case():
    rng = np.random.default_rng(2024)
    refs = [fm.dna(rng, 180), fm.dna(rng, 120)]
    targets = [fm.mosaic(rng, refs, int(n)) for n in rng.integers(100, 401, 8)]
    targets.insert(3, b"")
    targets.insert(6, refs[0][50:53])  # shorter than W for M in {5, 16}
    return refs, targets


def exhaustive_patterns(targets, M, seed=5):
    rng = np.random.default_rng(seed)
    lengths = sorted({m for m in (1, 2, 3, M - 1, M) if 1 <= m <= M})
    cut = fm.substrings(targets, lengths)
    rnd = [fm.dna(rng, int(rng.integers(1, M + 1))) for _ in range(200)]
    return cut + [fm.revcomp(p) for p in cut] + rnd


@pytest.fixture(scope="module")
def exhaustive(rlz):
    refs, targets = exhaustive_case()
    cases = {rc: Case(rlz, refs, targets, rc) for rc in (True, False)}
    yield cases
    for c in cases.values():
        c.close()


@pytest.mark.parametrize("with_rc", [True, False])
@pytest.mark.parametrize("M", [1, 2, 5, 16])
def test_exhaustive(exhaustive, M, with_rc):
    c = exhaustive[with_rc]
    assert len(c.targets) == 10 and min(map(len, c.targets)) == 0
    got = c.run(exhaustive_patterns(c.targets, M), M)
    assert got["primary"].any() == (M > 1) and not got["primary"].all()  # (every base occurs in the references: no literal)
    assert got["is_rc"].any() == with_rc


# ---- 3. literal runs ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("alphabet, with_rc", [(b"AC", False), (b"A", True)])
def test_literal_runs(rlz, alphabet, with_rc):
    """the targets hold runs of bases the index cannot match: adjacent literals, record starts one apart, merged windows"""
    rng = np.random.default_rng(9)
    ref = fm.dna(rng, 300, alphabet)
    foreign = b"GT" if alphabet == b"AC" else b"CG"
    targets = []
    for _ in range(5):
        t = bytearray(ref[int(rng.integers(0, 100)):int(rng.integers(150, 300))])
        for _ in range(4):
            at = int(rng.integers(0, len(t)))
            t[at:at] = fm.dna(rng, int(rng.integers(2, 9)), foreign)
        targets.append(bytes(t))
    targets.append(fm.dna(rng, 12, foreign))
    with Case(rlz, ref, targets, with_rc) as c:
        block, records, literals = c.arc._live().export()
        lit = records["ref"] == records["start"]
        assert (lit[1:] & lit[:-1]).sum() >= 10  # adjacent literals
        for M in (1, 3, 8):
            patterns = fm.substrings(targets, sorted({min(2, M), M})) + [fm.dna(rng, M) for _ in range(50)]
            patterns += [fm.revcomp(p) for p in patterns[:200]]
            got = c.run(patterns, M)
            assert got["primary"].any()


# ---- 4. depth and multiplicity -----------------------------------------------------------------------------------------
def test_depth_and_multiplicity(rlz):
    """z > 4096: the max pyramid has four levels; 80 targets share pieces, so a block hit inside a shared piece is
    covered by more than 64 records"""
    rng = np.random.default_rng(4)
    ref = fm.dna(rng, 2000)

    def pieces(n):
        out = []
        for _ in range(n):
            m = int(rng.integers(12, 50))
            at = int(rng.integers(0, len(ref) - m))
            out.append(fm.revcomp(ref[at:at + m]) if rng.integers(0, 2) else ref[at:at + m])
        return out

    shared = pieces(60)
    targets = [b"".join(shared)] * 40 + [b"".join(shared[:10] + pieces(50)) for _ in range(40)]
    patterns, at = [], 0
    for j, p in enumerate(shared[:30]):
        patterns.append(p[2:2 + min(20, len(p) - 2)])                     # inside a piece
        patterns.append(targets[0][at + len(p) - 6:at + len(p) + 6])       # across its joint with the next
        patterns.append(fm.revcomp(patterns[-2]))
        at += len(p)
    patterns += [fm.dna(rng, 8) for _ in range(40)]
    with Case(rlz, ref, targets, True) as c:
        assert c.arc.info["z"] > 4096
        got = c.run(patterns, M=24, kernel=False)
        inside = [j for j in range(0, 30, 3)]  # pieces of the first ten: in all 80 targets
        assert all(int(got["counts"][j]) >= 80 for j in inside)
        lo, hi = int(got["offsets"][0]), int(got["offsets"][1])
        assert (~got["primary"][lo:hi]).sum() > 64
        c.run(patterns, M=24, max_hits=79, kernel=False)


# ---- 5. chunk seams ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chunk", [1, 7, 64])
def test_chunk_seams(exhaustive, monkeypatch, chunk):
    c = exhaustive[True]
    patterns = exhaustive_patterns(c.targets, 5)[::17]
    whole = c.run(patterns, 5, kernel=False)
    assert len(whole["target"]) > 64
    monkeypatch.setenv("NOLZSS_RLZ_LOCATE_CHUNK", str(chunk))
    cut = c.run(patterns, 5, kernel=False)
    same(cut, whole)


# ---- 6. max_hits -------------------------------------------------------------------------------------------------------
def test_max_hits(exhaustive):
    c = exhaustive[True]
    patterns = [b"A", c.targets[0][5:10], b"ACG", b"", c.targets[1][7:12], b"TT"]
    with c.arc.finder(max_pattern_length=5) as f:
        free = check_finder(f, c.arc, c.targets, patterns, True)
        cap = int(np.sort(free["counts"])[-2])
        got = check_finder(f, c.arc, c.targets, patterns, True, max_hits=cap)
    over = free["counts"] > cap
    assert over.sum() == 1 and np.array_equal(got["counts"], free["counts"])
    for j in range(len(patterns)):
        assert hits_of(got, j) == ([] if over[j] else hits_of(free, j))
    assert got["counts"].dtype == got["offsets"].dtype == got["target"].dtype == got["position"].dtype == np.uint64
    assert got["is_rc"].dtype == got["primary"].dtype == bool
    assert len(got["offsets"]) == len(patterns) + 1 and got["offsets"][0] == 0 and got["offsets"][-1] == len(got["target"])
    assert rlz_dtype_fields(c) == ("target", "position", "is_rc", "primary")


def rlz_dtype_fields(c):
    from nolzss_amd.genomics import rlz
    assert rlz.TARGET_HIT_DTYPE.itemsize == 24
    return rlz.TARGET_HIT_DTYPE.names


# ---- 7. snapshot -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prefix_syms", [1, 12])
def test_snapshot_and_forced_prefix(rlz, prefix_syms):
    rng = np.random.default_rng(70 + prefix_syms)
    refs = [fm.dna(rng, 150)]
    first = [fm.mosaic(rng, refs, 120), fm.mosaic(rng, refs, 90)]
    more = [fm.mosaic(rng, refs, 100) + b"GATTACAGATTACA"]
    patterns = [b"GATTACAGAT", first[0][30:40], more[0][50:58], b"AC"]
    with Case(rlz, refs, first, True) as c:
        old = c.arc.finder(max_pattern_length=10, prefix_syms=prefix_syms)
        check_finder(old, c.arc, c.targets, patterns, True)
        c.arc.append(more)
        for call in (old.count, old.locate):
            with pytest.raises(ValueError, match="grown since the finder was opened.*open a new finder"):
                call(patterns)
        old.close()
        c.targets += more
        got = c.run(patterns, 10, prefix_syms=prefix_syms)
        assert 2 in got["target"][int(got["offsets"][0]):int(got["offsets"][1])].tolist()


# ---- 8. refusals -------------------------------------------------------------------------------------------------------
# (one refusal of the open has no test: a kernel text whose index text could pass the 32-bit pipeline takes an archive of
# more than 2^31 decoded bases with reverse complement, which no test of a few seconds can append)
def test_refusals_of_open(rlz, native):
    from nolzss_amd import _lib
    with rlz.RlzIndex.build(R) as ix, rlz.RlzIndex.build(R) as other, rlz.RlzArchive.from_index(ix) as arc:
        arc.append([R[5:50]])
        with rlz.RlzArchive.build(R, [R[5:50]]) as host:
            with pytest.raises(ValueError, match="finder needs an archive made by RlzArchive.from_index: this one was built from host records"):
                host.finder()
            with pytest.raises(ValueError, match="archive opened by nolzss_rlz_archive_open_index"):
                native.RlzFinderHandle.open(host._live(), ix._live())
        with pytest.raises(ValueError, match="bound to another index"):
            native.RlzFinderHandle.open(arc._live(), other._live())
        for M in (0, 4097):
            with pytest.raises(ValueError, match=f"max_pattern_length must be 1 .. 4096, it is {M}"):
                arc.finder(max_pattern_length=M)
        with pytest.raises(ValueError, match="prefix_syms must be 0"):
            arc.finder(prefix_syms=13)
        h = C.c_void_p()
        a, i = arc._live()._handle(), ix._live()._handle()
        for args in ((None, i, 8, 0, C.byref(h)), (a, None, 8, 0, C.byref(h)), (a, i, 8, 0, None)):
            assert _lib.lib.nolzss_rlz_finder_open(*args) == _lib.ERR_INVALID_ARGUMENT
        assert _lib.lib.nolzss_rlz_finder_info(None, None) == _lib.ERR_INVALID_ARGUMENT
        assert _lib.lib.nolzss_rlz_finder_close(None) == _lib.OK
        with arc.finder(max_pattern_length=4096) as f:  # the bounds of M are served
            assert f.count([R[5:50]]).tolist() == [1]
        with arc.finder(max_pattern_length=1) as f:
            assert f.info["max_pattern_length"] == 1


def test_an_archive_without_records(rlz):
    with rlz.RlzIndex.build(R) as ix, rlz.RlzArchive.from_index(ix) as arc:
        for targets in ([], [b"", b""]):
            if targets:
                arc.append(targets)
            with arc.finder() as f:
                assert f.info["z"] == 0 and f.info["kernel_length"] == 0 and f.info["device_bytes"] == 0
                assert f.count([b"ACG", b""]).tolist() == [0, 0]
                got = f.locate([b"ACG", R[:20]])
                assert got["offsets"].tolist() == [0, 0, 0] and len(got["target"]) == 0
                K, kstart, dstart = f.kernel()
                assert K == b"" and kstart.tolist() == [0] and dstart.tolist() == [0]
                with pytest.raises(RuntimeError, match="Invalid nucleotide 'N' found in pattern 0"):
                    f.count([b"N"])


def test_refusals_of_a_query(rlz):
    from nolzss_amd import _lib
    with Case(rlz, R, [R[5:50], R[20:30]], True) as c, c.arc.finder(max_pattern_length=5) as f:
        with pytest.raises(RuntimeError, match="Invalid nucleotide 'N' found in pattern 2"):
            f.count([b"ACG", b"", b"ACNT"])
        with pytest.raises(RuntimeError, match="Invalid nucleotide 'x' found in pattern 0"):
            f.locate([b"xA", b"N"])
        with pytest.raises(ValueError, match="max_hits"):
            f.locate([b"A"], max_hits=-1)
        # a pattern of M + 1 bases beside one of M bases: the batch is refused naming it, the M bases alone are served
        with pytest.raises(ValueError, match="pattern 1 has 6 bases, the finder was opened with max_pattern_length 5"):
            f.locate([R[10:15], R[10:16], R[10:17]])
        with pytest.raises(ValueError, match="pattern 0 has 6 bases"):
            f.count([R[10:16]])
        assert f.count([R[10:15]]).tolist() == [len(fm.brute_find(c.targets, R[10:15]))] and f.count([R[10:15]])[0] >= 1
        h = f._live()._handle()
        counts, offsets = np.zeros(1, dtype=np.uint64), np.zeros(2, dtype=np.uint64)
        out, n = C.c_void_p(), C.c_size_t()
        one = (C.c_char_p * 1)(b"AC")
        lens = (C.c_size_t * 1)(2)
        lib = _lib.lib
        assert lib.nolzss_rlz_finder_count(None, one, lens, 1, counts.ctypes.data) == _lib.ERR_INVALID_ARGUMENT
        assert lib.nolzss_rlz_finder_count(h, one, lens, 1, None) == _lib.ERR_INVALID_ARGUMENT
        assert lib.nolzss_rlz_finder_count(h, None, lens, 1, counts.ctypes.data) == _lib.ERR_INVALID_ARGUMENT
        assert lib.nolzss_rlz_finder_locate(h, one, lens, 1, 0, counts.ctypes.data, offsets.ctypes.data, None,
                                            C.byref(n)) == _lib.ERR_INVALID_ARGUMENT
        assert lib.nolzss_rlz_finder_locate(h, one, lens, 1, 0, counts.ctypes.data, None, C.byref(out),
                                            C.byref(n)) == _lib.ERR_INVALID_ARGUMENT
        assert lib.nolzss_rlz_finder_kernel(h, None, None, None, None, None) == _lib.ERR_INVALID_ARGUMENT
        assert f.count([]).tolist() == [] and f.locate([])["offsets"].tolist() == [0]
        assert f.count([b"AC"]).tolist() == [len(fm.brute_find(c.targets, b"AC"))]  # (the handle is still good)
        f.close()
        with pytest.raises(ValueError, match="closed"):
            f.count([b"AC"])


def test_block_occurrences_beyond_the_pipeline_are_refused_before_anything_is_expanded(rlz):
    ref = fm.dna(np.random.default_rng(41), 1 << 16)
    per = ref.count(b"A") + ref.count(b"T")
    q = rlz.MAX_TEXT // per + 2
    assert q < 200_000
    with Case(rlz, ref, [ref[100:140]], True) as c, c.arc.finder(max_pattern_length=1) as f:
        with pytest.raises(ValueError, match=rf"the batch has {q * per} occurrences in the block.*send fewer patterns"):
            f.locate([b"A"] * q)
        assert f.count([b"A"] * 3).tolist() == [len(fm.brute_find(c.targets, b"A"))] * 3


def test_a_total_of_hits_beyond_the_pipeline_is_refused_once_the_counts_are_known(rlz):
    """4096 copies of a 256-base reference: few block occurrences, each carried to every copy"""
    ref = fm.dna(np.random.default_rng(42), 256)
    copies = 4096
    per = (ref.count(b"A") + ref.count(b"T")) * copies
    q = rlz.MAX_TEXT // per + 2
    assert q < 20_000
    with rlz.RlzIndex.build(ref) as ix, ix.archive_on_device([ref] * copies) as arc, arc.finder(max_pattern_length=1) as f:
        assert arc.info["z"] == copies
        with pytest.raises(ValueError, match=rf"locate would report {q * per} hits.*max_hits"):
            f.locate([b"A"] * q)
        got = f.locate([b"A"] * q, max_hits=per - 1)  # every pattern capped: counts, and no hits
        assert got["counts"].tolist() == [per] * q and got["offsets"].tolist() == [0] * (q + 1) and len(got["target"]) == 0


# ---- 9. real genomes ---------------------------------------------------------------------------------------------------
def test_real_genomes(rlz):
    T7, T3 = genomes.records("T7")[0][1], genomes.records("T3")[0][1]
    rng = np.random.default_rng(37)
    patterns = []
    for j in range(2000):
        m = int(rng.integers(12, 33))
        at = int(rng.integers(0, len(T3) - m + 1))
        patterns.append(fm.revcomp(T3[at:at + m]) if j % 2 else T3[at:at + m])
    with Case(rlz, T7, [T3], True) as c:
        block, records, _ = c.arc._live().export()
        starts = (records["start"][:500].astype(np.int64) - len(block)).tolist()
        assert len(starts) == 500
        for b in starts:  # one pattern centred on each of the first 500 record starts
            lo = max(b - 12, 0)
            patterns.append(T3[lo:lo + 24])
        patterns += [fm.dna(rng, int(rng.integers(12, 33))) for _ in range(200)]
        got = c.run(patterns, M=32)
        assert (got["counts"][:2500] >= 1).all()
        centred = [hits_of(got, 2000 + j) for j in range(1, 500)]
        assert all(any(h[3] for h in hs) for hs in centred)  # each crosses its record start: a primary occurrence


# ---- 10. threads -------------------------------------------------------------------------------------------------------
def test_two_threads_query_one_finder(exhaustive):
    c = exhaustive[True]
    every = exhaustive_patterns(c.targets, 5)
    batches = [every[0::9], every[1::9]]
    with c.arc.finder(max_pattern_length=5) as f:
        single = [check_finder(f, c.arc, c.targets, b, True, max_hits=50) for b in batches]
        out, errors = [[None] * 4, [None] * 4], []

        def work(t):
            try:
                for rep in range(4):
                    out[t][rep] = f.locate(batches[t], max_hits=50)
                    assert np.array_equal(f.count(batches[t]), single[t]["counts"])
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
                same(got, single[t])
