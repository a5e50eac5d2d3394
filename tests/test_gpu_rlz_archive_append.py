"""The relative-LZ archive grown from the index on the device (nolzss_rlz_archive_open_index / _append_index / _export;
rlz_archive.hip, rlz_archive_api.hip).  Oracles: plain slicing of the upper-cased targets, the host path
absolute_records(reference, ix.factorize(targets)) record for record, and the archive ix.archive(targets) opens."""
import re
import threading
from pathlib import Path

import numpy as np
import pytest

import rlz_archive_model as arcmodel
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


def exported(arc):
    """(block, records, literals) of the archive's handle: nolzss_rlz_archive_export"""
    return arc._live().export()


def host_form(rlz, ix, refs, targets):
    """the existing path: (block, records, literals, lengths) through the host"""
    rows = ix.factorize(targets)
    block, records, lengths = rlz.absolute_records(_as_list(refs), rows)
    return block, records, b"".join(rlz.rlz_literals(targets, rows)), lengths


def check_against_host(rlz, ix, arc, refs, targets, old_archive=True):
    """export, lengths and every whole target of `arc` against the host path and against slicing"""
    block, records, literals = exported(arc)
    eb, er, el, lengths = host_form(rlz, ix, refs, targets)
    assert block == eb
    assert records.dtype == er.dtype and np.array_equal(records, er)
    assert literals == el
    assert len(arc) == len(targets) and arc.target_lengths == lengths == [len(t) for t in targets]
    info = arc.info
    assert info["z"] == len(er) and info["n_literals"] == len(el) and info["block_length"] == len(eb)
    assert info["num_targets"] == len(targets) and info["total_length"] == sum(lengths)
    whole = [(j, 0, len(t)) for j, t in enumerate(targets)]
    want = [bytes(t).upper() for t in targets]
    assert arc.extract(whole) == want
    if old_archive:
        with ix.archive(targets) as old:
            assert old.extract(whole) == want
            assert old._arrays["block"].tobytes() == block and np.array_equal(old._arrays["records"], records)
            assert old._arrays["literals"].tobytes() == literals
    return block, records, literals


def edge_ranges(targets):
    """every target whole, and ranges across each target's first and last byte"""
    out = []
    for j, t in enumerate(targets):
        n = len(t)
        out += [(j, 0, n), (j, 0, min(1, n)), (j, max(n - 1, 0), n), (j, 0, min(17, n)), (j, max(n - 17, 0), n), (j, n, n)]
    return out


def sliced(targets, ranges):
    return [bytes(targets[j]).upper()[lo:hi] for j, lo, hi in ranges]


# ---- 1. the smallest cases ---------------------------------------------------------------------------------------------
def test_smallest_cases(native, rlz):
    with rlz.RlzIndex.build(b"ACGT") as ix, rlz.RlzArchive.from_index(ix) as arc:
        assert len(arc) == 0 and arc.info["z"] == 0 and arc.info["total_length"] == 0 and arc.info["device_bytes"] >= 4
        (info,) = arc.append([b"ACGT"])
        assert info["records_added"] == 1 and info["literals_added"] == 0 and info["bases_added"] == 4 and info["z"] == 1
        assert arc.target(0) == b"ACGT"
        block, records, literals = exported(arc)
        assert block == b"ACGT" and records.tolist() == [(4, 4, 0)] and literals == b""
    with rlz.RlzIndex.build(b"A", with_rc=True) as ix, rlz.RlzArchive.from_index(ix) as arc:
        arc.append([b"T"])
        _, records, literals = exported(arc)
        assert records.tolist() == [(1, 1, model.RC_MASK | 0)] and literals == b""  # length 1: src = ref
        assert arc.target(0) == b"T"
    with rlz.RlzIndex.build(b"ACA", with_rc=False) as ix, rlz.RlzArchive.from_index(ix) as arc:
        (info,) = arc.append([b"g"])
        assert info["literals_added"] == 1
        _, records, literals = exported(arc)
        assert records.tolist() == [(3, 1, 3)] and literals == b"G" and arc.target(0) == b"G"


def test_empty_batches(native, rlz):
    with rlz.RlzIndex.build(b"ACGT") as ix, rlz.RlzArchive.from_index(ix) as arc:
        native.profile_enable(True)
        try:
            native.profile_reset()
            assert arc.append([]) == []
            assert arc._live().append_index(ix._live(), [])["targets_added"] == 0
            report = native.profile_report()
        finally:
            native.profile_enable(False)
            native.profile_reset()
        # The empty report is the only observable of "the device is not touched": it holds because every device path of
        # the library runs inside a ProfScope (the session of an append opens one before its first device call).
        assert not report, "k == 0 touches no device"
        assert len(arc) == 0
        (info,) = arc.append([b""])
        assert info["targets_added"] == 1 and info["records_added"] == 0 and info["z"] == 0 and len(arc) == 1
        (info,) = arc.append([b"", b"", b""])
        assert info["num_targets"] == 4 and info["z"] == 0 and info["total_length"] == 0
        assert arc.extract([(1, 0, 0)]) == [b""]
        block, records, literals = exported(arc)
        assert block == b"ACGT" and len(records) == 0 and literals == b""
        arc.append([b"", b"ACG", b""])
        assert arc.target_lengths == [0, 0, 0, 0, 0, 3, 0] and arc.target(5) == b"ACG" and arc.target(6) == b""


# ---- 2. the block unpacked on the device -------------------------------------------------------------------------------
@pytest.mark.parametrize("with_rc", [True, False])
def test_block_unpack(native, rlz, with_rc):
    for n in (1, 31, 32, 33, 63, 64, 65, 200):
        r = _dna(n, 200 + n)
        r = r[:n // 2] + r[n // 2:].lower()
        for refs in ([r], [r, b"", _dna(n, 300 + n).lower()], [_dna(31, n), r, _dna(n + 1, 400 + n)]):
            with rlz.RlzIndex.build(refs, with_rc=with_rc) as ix, rlz.RlzArchive.from_index(ix) as arc:
                block = exported(arc)[0]
                assert block == rlz.absolute_records(refs, [])[0], (n, len(refs))
                assert arc.info["block_length"] == len(block) == ix.info()["block_length"]


# ---- 3. separators and empty targets in a batch --------------------------------------------------------------------------
@pytest.mark.parametrize("with_rc", [True, False])
def test_separators_and_empty_targets(native, rlz, with_rc):
    refs = [_dna(700, 31, b"AT"), _dna(500, 32, b"AT")]  # no C, no G: a target over C and G is all literals on both strands
    fwd, rc, lit = refs[0][100:400] + refs[1][5:90], model.revcomp(refs[1][200:460]), _dna(70, 33, b"CG")
    batches = [[b"", fwd, rc, lit], [fwd, rc, lit, b""], [fwd, b"", b"", rc], [b"", fwd, b"", rc, b"", lit, b""],
               [lit, b"", fwd.lower(), b"", b"", rc, lit[:1], b""]]
    with rlz.RlzIndex.build(refs, with_rc=with_rc) as ix:
        for targets in batches:
            with rlz.RlzArchive.from_index(ix) as arc:
                arc.append(targets)
                _, records, literals = check_against_host(rlz, ix, arc, refs, targets)
                if with_rc:
                    kinds = set(arcmodel.record_kinds(records).tolist())
                    assert {"F", "R"} <= kinds and ("L" in kinds) == any(t[:1] == lit[:1] for t in targets)
                ranges = edge_ranges(targets)
                assert arc.extract(ranges) == sliced(targets, ranges)
        with rlz.RlzArchive.from_index(ix) as arc:  # ... and the same batches one behind the other
            everything = [t for targets in batches for t in targets]
            for targets in batches:
                arc.append(targets)
            check_against_host(rlz, ix, arc, refs, everything)
            ranges = edge_ranges(everything)
            assert arc.extract(ranges) == sliced(everything, ranges)


# ---- 4. the sample at the seam of two appends ------------------------------------------------------------------------------
@pytest.mark.parametrize("first", [0, 255, 256, 257, 512])
def test_sample_boundaries(native, rlz, first):
    ref = _dna(3000, 41, b"AT")
    long_copy, literals = ref[1000:1700], _dna(600, 42, b"CG")  # a first record longer than 256; 600 literal records
    targets = ([ref[20:20 + first]] if first else []) + [long_copy, literals]
    with rlz.RlzIndex.build(ref) as ix, rlz.RlzArchive.from_index(ix) as arc:
        if first:
            arc.append(targets[:1])
            assert arc.info["total_length"] == first
        arc.append(targets[-2:-1])
        arc.append(targets[-1:])
        block, records, lits = check_against_host(rlz, ix, arc, ref, targets, old_archive=False)
        own = records[records["start"] >= len(block) + first]
        assert int(own["length"][0]) > 256 and len(lits) >= 600
        lengths = [len(t) for t in targets]
        bases = np.concatenate([[0], np.cumsum(lengths)]).tolist()
        total = bases[-1]
        anchors = {first, first + len(long_copy)} | set(range(-(-first // 256) * 256, total, 256))
        ranges = []
        for a in sorted(anchors):
            for g in range(max(a - 20, 0), min(a + 21, total)):
                j = int(np.searchsorted(bases, g, side="right")) - 1
                for n in (1, 15, 16, 17, 255, 256, 257):
                    ranges.append((j, g - bases[j], min(g - bases[j] + n, lengths[j])))
        got = arc.extract(ranges)
        assert got == sliced(targets, ranges)
        assert got == arcmodel.extract(block, records, lits, lengths, ranges)


# ---- 5. chunk seams ----------------------------------------------------------------------------------------------------------
def _forty_targets():
    rng = np.random.default_rng(55)
    ref = _dna(4000, 51)
    targets = []
    for j in range(40):
        a, n = int(rng.integers(0, 3500)), int(rng.integers(0, 160))
        t = bytearray(ref[a:a + n])
        for q in rng.integers(0, max(n, 1), n // 10):
            t[int(q)] = b"ACGT"[int(rng.integers(4))]
        targets.append([bytes(t), model.revcomp(bytes(t)), b""][j % 3 if j % 7 else 2])
    return ref, targets


def test_chunk_seams(native, rlz, monkeypatch):
    ref, targets = _forty_targets()
    with rlz.RlzIndex.build(ref) as ix:
        monkeypatch.delenv("NOLZSS_RLZ_APPEND_CHUNK", raising=False)
        with ix.archive_on_device(targets) as arc:
            base = check_against_host(rlz, ix, arc, ref, targets)
            assert 150 <= len(base[1]) <= 700, len(base[1])  # about 300 records
        for chunk in ("1", "7", "64"):
            monkeypatch.setenv("NOLZSS_RLZ_APPEND_CHUNK", chunk)
            with ix.archive_on_device(targets) as arc:
                got = exported(arc)
                assert got[0] == base[0] and np.array_equal(got[1], base[1]) and got[2] == base[2], chunk
                assert arc.extract(edge_ranges(targets)) == sliced(targets, edge_ranges(targets))


# ---- 6. growth -----------------------------------------------------------------------------------------------------------------
def test_growth(native, rlz):
    rng = np.random.default_rng(66)
    ref = _dna(2500, 61)

    def piece():
        a, n = int(rng.integers(0, 2400)), int(rng.integers(1, 60))
        t = bytearray(ref[a:a + n])
        t[int(rng.integers(len(t)))] = b"ACGT"[int(rng.integers(4))]
        return bytes(t)

    with rlz.RlzIndex.build(ref) as ix, rlz.RlzArchive.from_index(ix) as arc:
        targets, moved, last_bytes = [], 0, arc.info["device_bytes"]
        for step in range(41):
            batch = [piece() for _ in range(1 if step < 40 else 200)]
            (info,) = arc.append(batch)
            targets += batch
            moved += info["reallocated"]
            assert info["reallocated"] in (0, 1) and info["capacity_records"] >= info["z"] == arc.info["z"]
            assert info["device_bytes"] >= last_bytes and info["device_bytes"] == arc.info["device_bytes"]
            assert info["device_bytes"] >= arc.info["block_length"] + 16 * info["capacity_records"]
            last_bytes = info["device_bytes"]
            if step % 5 == 4 or step == 40:
                assert arc.extract([(j, 0, len(t)) for j, t in enumerate(targets)]) == targets, step
        assert moved >= 4
        check_against_host(rlz, ix, arc, ref, targets, old_archive=False)


# ---- 7. equivalence at mid size ------------------------------------------------------------------------------------------------
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
def midsize():
    rng = np.random.default_rng(17)
    block = _dna(1 << 17, 1717)
    refs = [block[:70001], block[70001:]]
    targets = [_mutated(block, rng, int(rng.integers(1 << 15, (1 << 16) + 1)), j % 3 == 0) for j in range(12)]
    return {"refs": refs, "targets": targets}


@pytest.mark.parametrize("with_rc", [True, False])
def test_midsize_equals_the_host_path(native, rlz, midsize, with_rc):
    refs, targets = midsize["refs"], midsize["targets"]
    with rlz.RlzIndex.build(refs, with_rc=with_rc) as ix:
        with ix.archive_on_device(targets) as arc:
            block, records, literals = check_against_host(rlz, ix, arc, refs, targets)
            with rlz.RlzArchive.from_index(ix) as three:  # ... and as three batches
                for lo, hi in ((0, 5), (5, 6), (6, 12)):
                    three.append(targets[lo:hi])
                got = exported(three)
                assert got[0] == block and np.array_equal(got[1], records) and got[2] == literals
                assert three.extract([(j, 0, len(t)) for j, t in enumerate(targets)]) == targets
            rng = np.random.default_rng(71)
            ranges = []
            for _ in range(2000):
                j = int(rng.integers(len(targets)))
                lo = int(rng.integers(0, len(targets[j])))
                ranges.append((j, lo, min(lo + int(rng.integers(0, 400)), len(targets[j]))))
            with rlz.RlzArchive(block, records, literals, arc.target_lengths) as reopened:  # (passes the open check)
                assert reopened.extract(ranges) == arc.extract(ranges) == sliced(targets, ranges)


# ---- 8. more targets than sentinels ------------------------------------------------------------------------------------------
def test_six_hundred_targets(native, rlz):
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
    ids = [f"t{j}" for j in range(600)]
    with pytest.raises(ValueError, match="Too many sequences"):
        rlz.RlzArchive.build([ref], targets)
    with rlz.RlzIndex.build(ref) as ix, ix.archive_on_device(targets, ids=ids, batch_bases=1500) as arc:
        assert len(arc) == 600 and arc.ids == ids
        assert arc.extract([(f"t{j}", 0, len(t)) for j, t in enumerate(targets)]) == targets
        assert arc.target("t599") == targets[599] and arc.target(b"t0") == targets[0]
        check_against_host(rlz, ix, arc, ref, targets, old_archive=False)
        with pytest.raises(ValueError, match="distinct"):
            arc.append([b"ACGT"], ids=["t7"])
        with pytest.raises(ValueError, match="carries ids"):
            arc.append([b"ACGT"])
        assert len(arc) == 600


# ---- 9. no record crosses PCIe -----------------------------------------------------------------------------------------------
def test_an_append_moves_no_record_over_pcie(native, rlz):
    scopes = set()
    for name in ("suffix_array.hip", "sa_regroup.hip", "sa_direct.hip", "sa_repeats.hip"):
        src = (ROOT / "nolzss_amd" / "csrc" / name).read_text()
        scopes |= set(re.findall(r'ProfScope\s+\w+\([^"\n]*"([a-z_0-9]+)"', src))
    assert {"sa_sort_initial", "sa_regroup", "sa_direct_sort"} <= scopes
    ref = _dna(20000, 80)
    targets = [ref[100:4100], model.revcomp(ref[9000:12000]), _dna(500, 81)]
    with rlz.RlzIndex.build(ref) as ix, rlz.RlzArchive.from_index(ix) as arc:
        arc.append(targets)  # warm
        native.profile_enable(True)
        try:
            native.profile_reset()
            arc.append(targets)
            report = native.profile_report()
        finally:
            native.profile_enable(False)
            native.profile_reset()
        assert arc.extract([(j, 0, len(targets[j % 3])) for j in range(6)]) == targets + targets
    assert "factors_d2h" not in report and "records_h2d" not in report, sorted(report)
    assert report["rlz_index_search"][0] == 1 and report["rlz_archive_append"][0] == 1
    assert report["rlz_index_records"][0] >= 1 and report["rlz_append_records"][0] >= 1
    assert not scopes & set(report), sorted(scopes & set(report))


# ---- 10. save and load ----------------------------------------------------------------------------------------------------------
def test_save_and_load(native, rlz, tmp_path):
    ref, targets = _forty_targets()
    ids = [f"s{j}" for j in range(len(targets))]
    with rlz.RlzIndex.build(ref) as ix:
        with ix.archive_on_device(targets, ids=ids) as arc:
            arc.save(tmp_path / "device.npz")
            whole = arc.extract([(j, 0, len(t)) for j, t in enumerate(targets)])
        with ix.archive(targets, ids=ids) as old:
            old.save(tmp_path / "host.npz")
    with rlz.RlzArchive.load(tmp_path / "device.npz") as back:
        assert back.ids == ids and back.target_lengths == [len(t) for t in targets]
        assert back.extract([(i, 0, len(t)) for i, t in zip(ids, targets)]) == whole == targets
        with pytest.raises(ValueError, match="from_index"):
            back.append([b"ACGT"], ids=["x"])
    with np.load(tmp_path / "device.npz") as a, np.load(tmp_path / "host.npz") as b:
        assert sorted(a.files) == sorted(b.files) == sorted(rlz.ARCHIVE_ARRAYS)
        for name in rlz.ARCHIVE_ARRAYS:
            assert a[name].dtype == b[name].dtype and np.array_equal(a[name], b[name]), name


# ---- 11. refusals leave the archive as it was ---------------------------------------------------------------------------------
def test_refusals_leave_the_archive_as_it_was(native, rlz):
    import ctypes as C
    from nolzss_amd import _lib
    ref = [_dna(30, 90), _dna(20, 91)]  # m = 2, B = 51
    targets = [ref[0][3:25] + _dna(150, 92), model.revcomp(ref[1]), _dna(9, 93)]
    with rlz.RlzIndex.build(ref) as ix, rlz.RlzIndex.build(ref) as twin, rlz.RlzArchive.from_index(ix) as arc:
        arc.append(targets)
        assert arc.info["total_length"] > ix.info()["block_length"] + 2  # (the room rule below is the archive's own)

        def state():
            return arc.info, len(arc), arc.extract([(j, 0, len(t)) for j, t in enumerate(targets)]), exported(arc)[1].tobytes()

        before = state()
        with pytest.raises(RuntimeError, match="Invalid nucleotide 'N' found in sequence 4"):  # m + 2
            arc.append([b"ACGT", b"AC", b"ACNT", b"A"])
        assert state() == before
        with pytest.raises(ValueError, match="bound to another index"):
            arc._live().append_index(twin._live(), [b"ACGT"])
        assert state() == before
        with rlz.RlzArchive.build(ref, targets) as built:
            with pytest.raises(ValueError, match="from_index"):
                built.append([b"ACGT"])
            with pytest.raises(ValueError, match="opened by nolzss_rlz_archive_open_index"):
                built._live().append_index(ix._live(), [b"ACGT"])
            assert built.extract([(0, 0, len(targets[0]))]) == [targets[0]]
        # beyond the room left under MAX_TEXT: the lengths alone decide, the 4 bytes behind the pointer are never read
        h, ih = arc._live()._handle(), ix._live()._handle()
        room = rlz.MAX_TEXT - arc.info["total_length"]
        tg, ln, info = (C.c_char_p * 1)(b"ACGT"), (C.c_size_t * 1)(room + 1), _lib.RlzArchiveAppendInfo()
        assert _lib.lib.nolzss_rlz_archive_append_index(h, ih, tg, ln, 1, C.byref(info)) == _lib.ERR_INVALID_ARGUMENT
        assert b"decoded length" in _lib.lib.nolzss_last_error()
        ln[0] = rlz.MAX_TEXT + 1
        assert _lib.lib.nolzss_rlz_archive_append_index(h, ih, tg, ln, 1, C.byref(info)) == _lib.ERR_INVALID_ARGUMENT
        assert b"text too long" in _lib.lib.nolzss_last_error()
        assert _lib.lib.nolzss_rlz_archive_append_index(h, ih, None, None, 1, None) == _lib.ERR_INVALID_ARGUMENT
        assert _lib.lib.nolzss_rlz_archive_append_index(None, ih, tg, ln, 1, None) == _lib.ERR_INVALID_ARGUMENT
        assert _lib.lib.nolzss_rlz_archive_append_index(h, None, tg, ln, 1, None) == _lib.ERR_INVALID_ARGUMENT
        assert state() == before
        (info,) = arc.append([targets[1]])  # a good append then succeeds
        assert info["targets_added"] == 1 and arc.target(3) == targets[1] and arc.target(0) == targets[0]
        arc.close()
        arc.close()
        for call in (lambda: arc.append([b"ACGT"]), lambda: arc._live().export(), lambda: arc.info, lambda: len(arc),
                     lambda: arc.save("unused.npz")):
            with pytest.raises(ValueError, match="closed"):
                call()


# ---- 12. the life of the handles ----------------------------------------------------------------------------------------------
def test_handle_life(native, rlz):
    import nolzss_amd
    ref = [_dna(3000, 70), _dna(1500, 71)]
    rng = np.random.default_rng(7)
    block = b"".join(ref)
    targets = []
    for j in range(40):
        a, n = int(rng.integers(0, len(block) - 300)), int(rng.integers(0, 300))
        targets.append([block[a:a + n], model.revcomp(block[a:a + n]), _dna(n, 700 + j)][j % 3])
    whole = [(j, 0, len(t)) for j, t in enumerate(targets)]
    with rlz.RlzIndex.build(ref) as ix, rlz.RlzArchive.from_index(ix) as arc:
        assert arc.info["device"] == ix.info()["device"] == native.get_device()
        arc.append(targets[:13])
        # other calls between two appends leave both handles intact
        assert len(nolzss_amd.factorize(block)) > 0
        with rlz.RlzArchive.build(ref, targets[:5]) as other:
            assert other.target(3) == targets[3]
        results, errors = {}, []

        def work(name, fn):
            try:
                results[name] = fn()
            except Exception as e:  # pragma: no cover
                errors.append(e)

        threads = [threading.Thread(target=work, args=("match", lambda: ix.factorize(targets[20:]))),
                   threading.Thread(target=work, args=("extract", lambda: arc.extract(whole[:13])))]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
        assert not errors and results["extract"] == targets[:13]
        arc.append(targets[13:])
        serial = arc.extract(whole)
        assert serial == targets
        assert all(np.array_equal(a, b) for a, b in zip(results["match"], ix.factorize(targets[20:])))
        threads = [threading.Thread(target=work, args=("a", lambda: arc.extract(whole[:20]))),
                   threading.Thread(target=work, args=("b", lambda: arc.extract(whole[20:])))]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
        assert not errors and results["a"] + results["b"] == serial
        check_against_host(rlz, ix, arc, ref, targets)
        ix.close()  # the archive outlives its index: extraction and export need no index
        assert arc.extract(whole) == serial and len(exported(arc)[1]) == arc.info["z"]
        with pytest.raises(ValueError, match="closed"):
            arc.append([b"ACGT"])
