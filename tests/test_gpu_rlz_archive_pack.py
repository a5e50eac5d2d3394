"""The compact container end to end: RlzArchive.save(path, compact=True) packs an archive on the device, RlzArchive.load
opens the file on the device, and the loaded archive serves every target (nolzss_amd/genomics/rlz.py; C ABI
nolzss_rlz_archive_pack / _open_packed).  The file is the sequential model's file for the exported records
(tests/rlz_archive_pack_model.py), and smaller than the .npz of the same archive."""
import os

import numpy as np
import pytest

import rlz_archive_pack_model as model
import rlz_model

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def native():
    from nolzss_amd import _noLZSS
    assert _noLZSS.device_count() >= 1, "no MI355X visible"
    return _noLZSS


@pytest.fixture(scope="module")
def rlz():
    from nolzss_amd.genomics import rlz
    return rlz


def _dna(n, seed):
    rng = np.random.default_rng(seed)
    return np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, n)].tobytes()


def _planted(refs, seed):
    """12 targets cut from the reference: substitutions, two indels, one reverse-complement segment, one empty.  (A target
    with an N is refused by the match itself, "Invalid nucleotide": test_a_target_with_an_n holds that case.)"""
    rng = np.random.default_rng(seed)
    whole = b"".join(refs)
    targets = []
    for j in range(12):
        a = int(rng.integers(0, len(whole) - 6_000))
        t = bytearray(whole[a:a + int(rng.integers(2_000, 6_000))])
        for p in rng.integers(0, len(t), 6):
            t[p] = b"ACGT"[(b"ACGT".index(t[p]) + 1) % 4]
        targets.append(t)
    del targets[3][700:709]                                         # a deletion
    targets[5][1_000:1_000] = b"GATTACAGATTACA"                     # an insertion
    targets[7][300:1_200] = rlz_model.revcomp(bytes(targets[7][300:1_200]))
    targets[10] = bytearray()
    return [bytes(t) for t in targets]


def _npz_entries(path):
    """the members of an .npz and their bytes (the zip directory carries the time of writing: it is left out)"""
    import zipfile
    with zipfile.ZipFile(path) as z:
        return [(n, z.read(n)) for n in z.namelist()]


def _check_loaded(rlz, arc, loaded, targets, ids):
    assert loaded.ids == ids and len(loaded) == len(targets)
    assert loaded.target_lengths == arc.target_lengths == [len(t) for t in targets]
    for key in ("num_targets", "block_length", "z", "n_literals", "total_length"):
        assert loaded.info[key] == arc.info[key], key
    for j, t in enumerate(targets):
        assert loaded.target(j) == t.upper()
    if ids is not None:
        assert loaded.target(ids[4]) == targets[4].upper()
    with pytest.raises(ValueError, match="append needs an archive made by RlzArchive.from_index"):
        loaded.append([b"ACGT"], ids=None if ids is None else ["another"])
    with pytest.raises(ValueError, match="finder needs an archive made by RlzArchive.from_index"):
        loaded.finder()


def _check_file(rlz, arc, path, ids):
    block, records, literals = arc._live().export()
    lengths = arc.target_lengths
    want = model.container_bytes(model.pack(block, records, literals, lengths), lengths, ids)
    assert path.read_bytes() == want
    return block, records, literals


def test_index_built_archive_through_a_compact_file(native, rlz, tmp_path):
    refs = [_dna(12_000, 1), _dna(8_000, 2)]
    targets = _planted(refs, 3)
    ids = [f"isolate-{j}" for j in range(len(targets))]
    with rlz.RlzIndex.build(refs) as ix, ix.archive_on_device(targets, ids=ids) as arc:
        compact, npz = tmp_path / "a.rlz", tmp_path / "a.npz"
        arc.save(compact, compact=True)
        arc.save(npz)
        block, records, literals = _check_file(rlz, arc, compact, ids)
        assert len(block) == 20_001 and block[12_000] == 1  # (two reference records: one separator)
        kinds = {bool(r & model.RC_MASK) for r in records["ref"].tolist()}
        assert kinds == {True, False}
        assert os.path.getsize(compact) < os.path.getsize(npz)
        with rlz.RlzArchive.load(compact) as loaded:
            _check_loaded(rlz, arc, loaded, targets, ids)
            assert loaded.info["device_bytes"] > 0
            # a loaded archive saves again, both ways, to the same bytes
            loaded.save(tmp_path / "b.rlz", compact=True)
            loaded.save(tmp_path / "b.npz")
            assert (tmp_path / "b.rlz").read_bytes() == compact.read_bytes()
            assert _npz_entries(tmp_path / "b.npz") == _npz_entries(npz)
        with rlz.RlzArchive.load(npz) as old:  # the .npz still loads, the existing way
            assert old.target(7) == targets[7].upper() and old.ids == ids
        # the archive over the index is untouched by the pack: it still takes an append
        arc.append([targets[0]], ids=["again"])
        assert arc.target("again") == targets[0].upper()


def test_host_built_archive_through_a_compact_file(native, rlz, tmp_path):
    refs = [_dna(12_000, 1), _dna(8_000, 2)]
    targets = _planted(refs, 4)
    with rlz.RlzArchive.build(refs, targets, with_rc=False) as arc:
        compact, npz = tmp_path / "h.rlz", tmp_path / "h.npz"
        arc.save(compact, compact=True)
        arc.save(npz)
        _, records, _ = _check_file(rlz, arc, compact, None)
        assert not any(r & model.RC_MASK for r in records["ref"].tolist())
        assert os.path.getsize(compact) < os.path.getsize(npz)
        with rlz.RlzArchive.load(compact) as loaded:
            _check_loaded(rlz, arc, loaded, targets, None)


def test_a_target_with_an_n(native, rlz, tmp_path):
    """The index and rlz_factorize refuse a target that holds an N, so no archive of theirs has one; an archive opened
    from records may: its N is a literal, the literal section goes out at one byte per symbol, and the file loads."""
    refs = [_dna(3_000, 5)]
    with rlz.RlzIndex.build(refs) as ix:
        with pytest.raises(RuntimeError, match="Invalid nucleotide 'N'"):
            ix.archive_on_device([refs[0][:50] + b"N" + refs[0][51:90]])
    b = model.Builder(refs[0])
    b.copy(100, 400).literal(b"N").copy_step(300).literal(b"T").copy(2_000, 77, rc=True)
    lengths, ids = [701, 0, 78], ["with n", "empty", "rc"]
    with rlz.RlzArchive(refs[0], b.records(), bytes(b.literals), lengths, ids=ids) as arc:
        arc.save(tmp_path / "n.rlz", compact=True)
        assert (tmp_path / "n.rlz").read_bytes() == model.container_bytes(
            model.pack(refs[0], b.records(), b.literals, lengths), lengths, ids)
        with rlz.RlzArchive.load(tmp_path / "n.rlz") as loaded:
            want = refs[0][100:500] + b"N" + refs[0][501:801]
            assert loaded.target("with n") == want == arc.target(0) and loaded.target(1) == b""
            assert loaded.target("rc") == arc.target(2) == b"T" + rlz_model.revcomp(refs[0][2_000:2_077])
            assert rlz.read_packed_archive(tmp_path / "n.rlz")[0]["literal_mode"] == 0


def test_empty_archive_over_an_index(native, rlz, tmp_path):
    with rlz.RlzIndex.build([b"ACGTACGTTT", b"GGA"]) as ix, rlz.RlzArchive.from_index(ix, ids=[]) as arc:
        arc.save(tmp_path / "e.rlz", compact=True)
        _check_file(rlz, arc, tmp_path / "e.rlz", [])
        with rlz.RlzArchive.load(tmp_path / "e.rlz") as loaded:
            assert len(loaded) == 0 and loaded.ids == [] and loaded.info["z"] == 0 and loaded.info["block_length"] == 14
            assert loaded._live().export()[0] == b"ACGTACGTTT\x01GGA"
