"""Locate through the parse of a relative-LZ archive without a GPU: the brute force of the definition
(tests/rlz_find_model.brute_find) against bytes.find on real genomes, the invariants of the interval model, the
argument that every primary occurrence lies inside one interval, and what the library and the Python layers decide
before any device work."""
import ctypes as C

import numpy as np
import pytest

import genomes
import rlz_find_model as fm


def find_all(text, p):
    out, at = [], text.find(p)
    while at >= 0:
        out.append(at)
        at = text.find(p, at + 1)
    return out


def test_the_brute_force_is_bytes_find_on_t7_and_t3():
    T7, T3 = genomes.records("T7")[0][1], genomes.records("T3")[0][1]
    targets = [T7, b"", T3]
    texts = fm.Texts(targets)
    rng = np.random.default_rng(3)
    patterns = [b"GAATTC", b"A" * 7, b"ACGT", T7[-20:] + T3[:20], T7[-9:], T3[:11], b""]
    for _ in range(60):
        t = targets[int(rng.integers(0, 2)) * 2]
        m = int(rng.integers(4, 33))
        at = int(rng.integers(0, len(t) - m + 1))
        patterns.append(fm.revcomp(t[at:at + m]) if rng.integers(0, 2) else t[at:at + m])
    for p in patterns:
        for with_rc in (True, False):
            want = []
            for t, text in enumerate(targets):
                found = [(at, 0) for at in find_all(text, p)] if p else []
                if with_rc and p:
                    found += [(at, 1) for at in find_all(text, fm.revcomp(p))]
                want += [(t, at, rc) for at, rc in sorted(found)]
            got = fm.brute_find(texts, p, with_rc)
            assert got.shape == (len(want), 3) and [tuple(r) for r in got.tolist()] == want, (p, with_rc)
    assert len(fm.brute_find(texts, T7[-20:] + T3[:20])) == 0  # the end of a target joined to the start of the next
    assert [tuple(r) for r in fm.brute_find([b"ccGAATTCcc"], b"gaattc").tolist()] == [(0, 2, 0), (0, 2, 1)]
    assert [tuple(r) for r in fm.brute_find([b"CCGAATTCCC"], b"GAATTC", False).tolist()] == [(0, 2, 0)]


def random_parse(rng, lengths):
    """record starts that tile targets of these lengths: records of 1 .. 12 bases, runs of one-base records among them"""
    starts, at = [], 0
    for n in lengths:
        end = at + n
        while at < end:
            starts.append(at)
            at += min(int(rng.integers(1, 13)) if rng.random() < 0.7 else 1, end - at)
    return np.array(starts, dtype=np.int64)


def test_the_intervals_are_disjoint_ascending_and_inside_one_target():
    rng = np.random.default_rng(8)
    for _ in range(200):
        lengths = [int(x) for x in rng.integers(0, 60, int(rng.integers(1, 8)))]
        starts = random_parse(rng, lengths)
        bases = np.cumsum([0] + lengths)
        for M in (1, 2, 3, 7, 40):
            W = max(M - 1, 1)
            ds, de = fm.intervals(starts, lengths, M)
            assert (de > ds).all() and (ds[1:] >= de[:-1]).all()
            t = np.searchsorted(bases, ds, side="right") - 1
            assert (bases[t] <= ds).all() and (de <= bases[t + 1]).all()
            # intervals of one target that touch were merged; every window is inside an interval, and every interval
            # position within W of a record start of its target
            same_target = t[1:] == t[:-1]
            assert (ds[1:][same_target] > de[:-1][same_target]).all()
            for b in starts.tolist():
                j = int(np.searchsorted(bases, b, side="right")) - 1
                i = int(np.searchsorted(ds, b, side="right")) - 1
                assert ds[i] <= max(bases[j], b - W) and min(bases[j + 1], b + W) <= de[i]
            covered = np.zeros(int(bases[-1]) + 1, dtype=bool)
            for b in starts.tolist():
                j = int(np.searchsorted(bases, b, side="right")) - 1
                covered[max(bases[j], b - W):min(bases[j + 1], b + W)] = True
            inside = np.zeros_like(covered)
            for s, e in zip(ds.tolist(), de.tolist()):
                inside[s:e] = True
            assert np.array_equal(covered, inside)
    assert [x.tolist() for x in fm.intervals([], [0, 0], 5)] == [[], []]


def test_every_primary_occurrence_lies_inside_one_interval():
    """exhaustive over small parses: an occurrence [p, p + m) with m <= M that crosses a record start, or starts at a
    one-base record (what a literal is), lies inside one interval; so the kernel text holds it"""
    rng = np.random.default_rng(21)
    for _ in range(60):
        lengths = [int(x) for x in rng.integers(0, 40, int(rng.integers(1, 5)))]
        starts = random_parse(rng, lengths)
        ends = np.append(starts[1:], sum(lengths))
        bases = np.cumsum([0] + lengths)
        for M in (1, 2, 5, 9):
            ds, de = fm.intervals(starts, lengths, M)
            for j, n in enumerate(lengths):
                for m in range(1, M + 1):
                    for p in range(int(bases[j]), int(bases[j]) + n - m + 1):
                        k = int(np.searchsorted(starts, p, side="right")) - 1
                        primary = p + m > ends[k] or ends[k] - starts[k] == 1
                        if primary:
                            i = int(np.searchsorted(ds, p, side="right")) - 1
                            assert i >= 0 and ds[i] <= p and p + m <= de[i], (lengths, starts.tolist(), M, p, m)


def test_the_kernel_text_and_the_primary_flag_of_a_small_parse():
    targets = [b"ACGTACGTAC", b"", b"GGGTTT"]
    starts = [0, 4, 5, 10, 13]  # records [0,4) [4,5) [5,10) | [10,13) [13,16)
    K, kstart, dstart = fm.kernel_text(targets, starts, 3)
    assert (K, kstart.tolist(), dstart.tolist()) == (b"ACGTACGGGGTT", [0, 7, 12], [0, 10, 16])
    K, kstart, dstart = fm.kernel_text(targets, starts, 2)
    assert (K, kstart.tolist(), dstart.tolist()) == (b"ATACGGT", [0, 1, 4, 5, 7], [0, 3, 10, 12, 16])
    records = np.zeros(5, dtype=[("start", "<u8"), ("length", "<u8"), ("ref", "<u8")])
    records["start"] = np.array(starts) + 100
    records["length"] = [4, 1, 5, 3, 3]
    records["ref"] = [0, 104, 1 | (1 << 63), 7, 2]  # record 1 is a literal
    hits = [(0, 0, 0), (0, 2, 0), (0, 4, 0), (0, 5, 1), (2, 0, 0), (2, 2, 0)]
    assert fm.primary_flags(records, 100, [0, 10, 10], hits, 3).tolist() == [False, True, True, False, False, True]
    exp = fm.expected(targets, records, 100, [b"GT", b"acg", b"GGGTTTA"], True)
    assert exp["counts"].tolist() == [6, 4, 0] and exp["offsets"].tolist() == [0, 6, 10, 10]
    assert exp["target"].tolist() == [0, 0, 0, 0, 0, 2, 0, 0, 0, 0]
    assert exp["position"].tolist() == [0, 2, 4, 6, 8, 2, 0, 1, 4, 5]
    assert exp["is_rc"].tolist() == [1, 0, 1, 0, 1, 0, 0, 1, 0, 1]
    assert exp["primary"].tolist() == [0, 0, 1, 0, 0, 1, 0, 0, 1, 0]
    assert fm.expected(targets, records, 100, [b"GT", b"ACG"], True, max_hits=3)["offsets"].tolist() == [0, 0, 0]


def test_the_library_and_the_python_layers_carry_the_finder():
    from nolzss_amd import _lib
    from nolzss_amd import _noLZSS as native
    import noLZSS.genomics.rlz as ref_names
    import nolzss_amd.genomics.rlz as rlz
    names = ["nolzss_rlz_finder_open", "nolzss_rlz_finder_info", "nolzss_rlz_finder_count", "nolzss_rlz_finder_locate",
             "nolzss_rlz_finder_kernel", "nolzss_rlz_finder_close"]
    header = (genomes.DIR.parent.parent.parent / "include" / "nolzss_hip.h").read_text()
    for name in names:
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(_lib.lib, name) and f"int {name}(" in header
    assert native.TARGET_HIT_DTYPE.itemsize == 24
    assert native.TARGET_HIT_DTYPE.names == ("target", "position", "is_rc", "primary")
    assert C.sizeof(_lib.RlzFinderSummary) == 64
    for mod in (rlz, ref_names):
        assert "TARGET_HIT_DTYPE" in mod.__all__ and mod.TARGET_HIT_DTYPE is native.TARGET_HIT_DTYPE
        assert "RlzArchiveFinder" in mod.__all__ and callable(mod.RlzArchive.finder)
        assert callable(mod.RlzArchiveFinder.count) and callable(mod.RlzArchiveFinder.locate)
    assert callable(native.RlzFinderHandle.open) and callable(native.RlzFinderHandle.kernel)


def test_null_pointers_are_refused_without_a_device():
    from nolzss_amd import _lib
    lib = _lib.lib
    h = C.c_void_p()
    assert lib.nolzss_rlz_finder_open(None, None, 8, 0, C.byref(h)) == _lib.ERR_INVALID_ARGUMENT and not h.value
    assert lib.nolzss_last_error() == b"archive or index handle is null"
    assert lib.nolzss_rlz_finder_open(None, None, 8, 0, None) == _lib.ERR_INVALID_ARGUMENT
    assert lib.nolzss_rlz_finder_info(None, None) == _lib.ERR_INVALID_ARGUMENT
    counts = np.zeros(1, dtype=np.uint64)
    assert lib.nolzss_rlz_finder_count(None, None, None, 0, counts.ctypes.data) == _lib.ERR_INVALID_ARGUMENT
    out, n = C.c_void_p(), C.c_size_t()
    assert lib.nolzss_rlz_finder_locate(None, None, None, 0, 0, None, None, C.byref(out), C.byref(n)) == _lib.ERR_INVALID_ARGUMENT
    assert lib.nolzss_rlz_finder_locate(None, None, None, 0, 0, None, None, None, None) == _lib.ERR_INVALID_ARGUMENT
    assert lib.nolzss_rlz_finder_kernel(None, None, None, None, None, None) == _lib.ERR_INVALID_ARGUMENT
    assert lib.nolzss_rlz_finder_close(None) == _lib.OK


def test_an_archive_of_host_records_has_no_finder():
    import nolzss_amd.genomics.rlz as rlz
    arc = rlz.RlzArchive.__new__(rlz.RlzArchive)  # (no device: the state of an archive built from host records)
    arc._handle, arc._arrays, arc._bound = object(), {"block": b""}, None
    with pytest.raises(ValueError, match="finder needs an archive made by RlzArchive.from_index: this one was built from host records"):
        arc.finder()
    arc._handle = None
    with pytest.raises(ValueError, match="the archive is closed"):
        arc.finder()
