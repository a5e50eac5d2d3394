"""CPU tests of the relative-LZ archive (no GPU): the sequential model against plain slicing, the refusal rules of the
model, the .npz file form without a handle, the ids-to-index mapping, and the properties of the boundary input that
tests/test_gpu_rlz_archive.py relies on."""
import random

import numpy as np
import pytest

import gen
import rlz_archive_model as model
import rlz_model
from nolzss_amd import _lib, _noLZSS as native
from nolzss_amd.genomics import rlz

RC = model.RC_MASK


def _collection(seed):
    rng = random.Random(seed)
    refs = [gen.mixed_dna(rng, 120).encode(), gen.mixed_dna(rng, 80).encode()]
    whole = b"".join(refs)
    targets = []
    for _ in range(4):
        a = rng.randrange(0, len(whole) - 40)
        piece = bytearray(whole[a:a + 40] + rlz_model.revcomp(whole[a + 5:a + 30]) + b"NN" + whole[:17])
        piece[rng.randrange(len(piece))] = ord("C")
        targets.append(bytes(piece))
    targets.insert(2, b"")
    return refs, targets


@pytest.mark.parametrize("with_rc", [True, False])
def test_model_equals_slicing_of_the_targets(with_rc):
    refs, targets = _collection(31)
    block, records, literals, lengths = model.parse_to_absolute(refs, targets, with_rc)
    assert lengths == [len(t) for t in targets]
    assert model.open_refusal(len(block), records, len(literals), lengths) is None
    assert model.expand(block, records, literals) == b"".join(targets)
    kinds = set(model.record_kinds(records).tolist())
    assert kinds == ({"F", "R", "L"} if with_rc else {"F", "L"})
    rng = random.Random(5)
    ranges = [(j, 0, len(t)) for j, t in enumerate(targets)]
    for _ in range(300):
        j = rng.randrange(len(targets))
        lo = rng.randint(0, len(targets[j]))
        ranges.append((j, lo, rng.randint(lo, len(targets[j]))))
    assert model.extract_refusal(lengths, ranges) is None
    got = model.extract(block, records, literals, lengths, ranges)
    assert got == [targets[j][lo:hi] for j, lo, hi in ranges]


def test_model_open_rules():
    # block ACGT (4 bytes), one target of 6 bytes: copy 4, literal, literal
    good = [(4, 4, 0), (8, 1, 8), (9, 1, 9)]
    assert model.open_refusal(4, good, 2, [6]) is None
    assert model.open_refusal(4, good, 2, [4, 0, 2]) is None
    assert model.open_refusal(4, [(4, 4, 0), (9, 1, 9)], 1, [6]) == (model.TILING, 1)
    assert model.open_refusal(4, [(4, 4, 0), (8, 2, 8)], 1, [6]) == (model.LITERAL_LENGTH, 1)
    assert model.open_refusal(4, [(4, 4, 1), (8, 1, 8), (9, 1, 9)], 2, [6]) == (model.SOURCE_IN_BLOCK, 0)
    assert model.open_refusal(4, [(4, 4, 0), (8, 2, 4 | RC)], 0, [6]) == (model.SOURCE_IN_BLOCK, 1)  # self-referential
    assert model.open_refusal(4, good, 2, [3, 3]) == (model.TARGET_BOUNDARY, 0)  # straddles the end of target 0
    assert model.open_refusal(4, good, 2, [5]) == (model.TARGET_BOUNDARY, 2)     # behind the last target
    assert model.open_refusal(4, good, 2, [7]) == (model.TARGET_BOUNDARY, 3)     # lengths do not sum: z, behind the last
    assert model.open_refusal(4, good, 1, [6]) == (model.LITERAL_COUNT, 2)
    assert model.open_refusal(4, good, 3, [6]) == (model.LITERAL_COUNT, 3)
    assert model.open_refusal(4, [], 0, []) is None and model.open_refusal(4, [], 0, [0, 0, 0]) is None
    assert model.open_refusal(4, [], 0, [1]) == (model.TARGET_BOUNDARY, 0)
    assert model.open_refusal(4, good, 2, []) == (model.TARGET_BOUNDARY, 0)      # k == 0 holds no record


def test_model_extract_rules():
    lengths = [6, 0, 3]
    assert model.extract_refusal(lengths, [(0, 0, 6), (1, 0, 0), (2, 3, 3)]) is None
    assert model.extract_refusal(lengths, [(0, 0, 6), (3, 0, 0)]) == (model.BAD_TARGET, 1)
    assert model.extract_refusal(lengths, [(0, 4, 3)]) == (model.LO_ABOVE_HI, 0)
    assert model.extract_refusal(lengths, [(0, 0, 6), (0, 0, 7)]) == (model.HI_BEYOND, 1)
    assert model.extract_refusal(lengths, [(1, 0, 1)]) == (model.HI_BEYOND, 0)
    assert model.extract_refusal(lengths, [(0, 0, 6), (2, 0, 3)], capacity=8) == (model.CAPACITY, 2)
    assert model.extract_refusal(lengths, [(0, 0, 6), (2, 0, 3)], capacity=9) is None
    assert model.extract_refusal([1 << 31], [(0, 0, 1 << 31)] * 2) == (model.TOO_MANY_BYTES, 1)


def test_model_reports_the_complement_of_a_non_nucleotide():
    block = b"ACG\x01TTA"
    records = [(7, 3, 2 | RC), (10, 1, 10)]  # revcomp(block[2:5]) crosses the separator at its middle byte
    with pytest.raises(ValueError):
        model.expand(block, records, b"x")
    faults = []
    assert model.expand(block, records, b"x", faults) == b"A\x00Cx" and faults == [1]


def test_boundary_input_has_the_properties_the_gpu_tests_rely_on():
    inp = model.boundary_input()
    first, kinds = model.check_boundary_input(inp)
    assert model.open_refusal(len(inp["block"]), inp["records"], len(inp["literals"]), inp["lengths"]) is None
    # every kind of boundary the GPU test walks around
    pairs = {kinds[i] + kinds[i + 1] for i in range(len(kinds) - 1)}
    assert {"FL", "LF", "LR", "RL"} <= pairs
    cut = model.boundary_cut()
    assert len(cut["targets"][0]) == 300 and set(model.record_kinds(cut["records"]).tolist()) == {"F", "R", "L"}
    assert model.expand(cut["block"], cut["records"], cut["literals"]) == cut["targets"][0]


def test_file_round_trip_without_a_handle(tmp_path):
    inp = model.boundary_input()
    ids = ["first", "empty", "shifted"]
    arrays = rlz.archive_arrays(inp["block"], inp["records"], inp["literals"], inp["lengths"], ids)
    path = tmp_path / "a.npz"
    rlz.save_archive_arrays(path, arrays)
    block, records, literals, lengths, got_ids = rlz.load_archive_arrays(path)
    assert block == inp["block"] and literals == inp["literals"] and got_ids == ids
    assert np.array_equal(records, inp["records"]) and lengths.tolist() == inp["lengths"]
    assert records.dtype == native.FACTOR_DTYPE and lengths.dtype == np.uint64
    rlz.save_archive_arrays(path, rlz.archive_arrays(inp["block"], inp["records"], inp["literals"], inp["lengths"]))
    assert rlz.load_archive_arrays(path)[4] is None
    empty = rlz.archive_arrays(b"ACGT", np.zeros(0, dtype=native.FACTOR_DTYPE), b"", [])
    rlz.save_archive_arrays(path, empty)
    assert rlz.load_archive_arrays(path)[0] == b"ACGT" and len(rlz.load_archive_arrays(path)[3]) == 0


def test_load_refuses_missing_arrays_and_inconsistent_sizes(tmp_path):
    inp = model.boundary_input()
    good = rlz.archive_arrays(inp["block"], inp["records"], inp["literals"], inp["lengths"], ["a", "b", "c"])
    path = tmp_path / "bad.npz"

    def refused(arrays, match):
        with open(path, "wb") as fh:
            np.savez(fh, **arrays)
        with pytest.raises(ValueError, match=match):
            rlz.load_archive_arrays(path)
        with pytest.raises(ValueError, match=match):  # before any device call: this test runs without one
            rlz.RlzArchive.load(path)

    for name in rlz.ARCHIVE_ARRAYS:
        refused({k: v for k, v in good.items() if k != name}, "missing arrays")
    refused(dict(good, target_lengths=np.array([4911, 0, 4903], dtype=np.uint64)), "inconsistent sizes")
    refused(dict(good, literals=good["literals"][:-1]), "inconsistent sizes")
    refused(dict(good, block=good["block"][:-1]), "inconsistent sizes")
    refused(dict(good, records=good["records"][:-1]), "inconsistent sizes")
    refused(dict(good, ids=good["ids"][:2]), "inconsistent sizes")
    refused(dict(good, records=np.zeros((3, 3), dtype=np.uint64)), "FACTOR_DTYPE")
    refused(dict(good, block=good["block"].astype(np.uint16)), "uint8")
    refused(dict(good, target_lengths=good["target_lengths"].astype(np.float64)), "uint64")
    path.write_bytes(b"not a zip file")
    with pytest.raises(ValueError, match="not a relative-LZ archive"):
        rlz.load_archive_arrays(path)
    with open(path, "wb") as fh:
        np.savez(fh, **dict(good, ids=np.array(["a", None, 3], dtype=object)))
    with pytest.raises(ValueError):  # a pickled array: allow_pickle is off
        rlz.load_archive_arrays(path)


def test_ids_map_to_indices():
    index = rlz.target_index_map(["chrA", "chrB", "7"])
    assert rlz.resolve_target("chrB", index, 3) == 1 and rlz.resolve_target(b"chrA", index, 3) == 0
    assert rlz.resolve_target("7", index, 3) == 2 and rlz.resolve_target(2, index, 3) == 2
    assert rlz.resolve_target(np.int64(1), index, 3) == 1
    assert rlz.resolve_target(3, index, 3) == 3  # the library names the range it belongs to
    with pytest.raises(KeyError):
        rlz.resolve_target("chrC", index, 3)
    with pytest.raises(KeyError):
        rlz.resolve_target("chrA", rlz.target_index_map(None), 3)
    with pytest.raises(ValueError):
        rlz.resolve_target(-1, index, 3)
    with pytest.raises(TypeError):
        rlz.resolve_target(1.5, index, 3)
    with pytest.raises(ValueError, match="distinct"):
        rlz.archive_arrays(b"ACGT", np.zeros(0, dtype=native.FACTOR_DTYPE), b"", [0, 0], ["x", "x"])
    with pytest.raises(ValueError, match="2 targets"):
        rlz.archive_arrays(b"ACGT", np.zeros(0, dtype=native.FACTOR_DTYPE), b"", [0, 0], ["x"])


def test_interface_is_declared_and_exported():
    for name in ("nolzss_rlz_archive_open_records", "nolzss_rlz_archive_info", "nolzss_rlz_archive_extract",
                 "nolzss_rlz_archive_extract_device", "nolzss_rlz_archive_close"):
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(_lib.lib, name)
    import noLZSS.genomics.rlz as ref_path
    assert ref_path.RlzArchive is rlz.RlzArchive and "RlzArchive" in ref_path.__all__ and "RlzArchive" in rlz.__all__
    assert hasattr(native, "RlzArchiveHandle")
    import ctypes
    assert ctypes.sizeof(_lib.RlzRange) == 24 and ctypes.sizeof(_lib.RlzArchiveSummary) == 64
