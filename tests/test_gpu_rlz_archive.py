"""The relative-LZ archive on the device (rlz_archive.hip, rlz_archive_api.hip): batches of (target, lo, hi) ranges from
resident records.  Every comparison is byte equality with the sequential model (tests/rlz_archive_model.py), with plain
slicing of the targets, or with the decoder (rlz_decode); refusals are held against the model's (rule, index)."""
import random
import threading

import numpy as np
import pytest

import gen
import rlz_archive_model as model
import rlz_model

pytestmark = pytest.mark.gpu

RC = model.RC_MASK
LENGTHS = (0, 1, 15, 16, 17, 255, 256, 257)


@pytest.fixture(scope="module")
def native():
    from nolzss_amd import _noLZSS
    assert _noLZSS.device_count() >= 1, "no MI355X visible"
    return _noLZSS


@pytest.fixture(scope="module")
def rlz(native):
    from nolzss_amd.genomics import rlz
    return rlz


@pytest.fixture(scope="module")
def boundary(rlz):
    inp = model.boundary_input()
    model.check_boundary_input(inp)
    with rlz.RlzArchive(inp["block"], inp["records"], inp["literals"], inp["lengths"]) as archive:
        yield inp, archive


def check_against_model(archive, inp, ranges):
    """one call: bytes against the model, offsets against the prefix sums"""
    data, offsets = archive.extract_array(ranges)
    exp = model.extract(inp["block"], inp["records"], inp["literals"], inp["lengths"], ranges)
    sums = np.concatenate([[0], np.cumsum([hi - lo for _, lo, hi in ranges], dtype=np.uint64)]).astype(np.uint64)
    assert offsets.dtype == np.uint64 and np.array_equal(offsets, sums)
    assert data.dtype == np.uint8 and len(data) == int(sums[-1])
    raw = data.tobytes()
    if raw != b"".join(exp):
        bad = next(i for i, e in enumerate(exp) if raw[int(sums[i]):int(sums[i + 1])] != e)
        raise AssertionError(f"range {bad} = {ranges[bad]} differs from the model")
    return exp


# ---- the smallest cases ----------------------------------------------------------------------------------------------
def test_one_record_every_range(rlz):
    with rlz.RlzArchive(b"ACGT", np.array([(4, 4, 0)], dtype=rlz._native.FACTOR_DTYPE), b"", [4]) as a:
        assert len(a) == 1 and a.target_lengths == [4]
        info = a.info
        assert (info["num_targets"], info["block_length"], info["z"], info["n_literals"], info["total_length"]) == (1, 4, 1, 0, 4)
        assert info["device_bytes"] == 4 + 16 + 4  # the block, 16 bytes per record, one sample word
        ranges = [(0, lo, hi) for lo in range(5) for hi in range(lo, 5)]
        assert a.extract(ranges) == [b"ACGT"[lo:hi] for _, lo, hi in ranges]
        assert a.target(0) == b"ACGT" and a.fetch(0, 1, 3) == b"CG"


def test_reverse_complement_copy_of_one_base(rlz):
    with rlz.RlzArchive(b"A", np.array([(1, 1, 0 | RC)], dtype=rlz._native.FACTOR_DTYPE), b"", [1]) as a:
        assert a.target(0) == b"T" and a.extract([(0, 0, 1), (0, 1, 1), (0, 0, 0), (0, 0, 1)]) == [b"T", b"", b"", b"T"]


def test_one_literal_byte_from_host_records(native):
    with native.RlzArchiveHandle.open_records(b"ACGT", [(4, 1, 4)], b"\xff", [1]) as h:
        data, offsets = h.extract_array([(0, 0, 1)])
        assert data.tobytes() == b"\xff" and offsets.tolist() == [0, 1]
        assert h.info["n_literals"] == 1 and h.target_lengths.tolist() == [1]


def test_no_targets_empty_targets_and_no_ranges(rlz, boundary):
    none = np.zeros(0, dtype=rlz._native.FACTOR_DTYPE)
    with rlz.RlzArchive(b"ACGT", none, b"", []) as a:
        assert len(a) == 0 and a.extract([]) == [] and a.info["z"] == 0 and a.info["device_bytes"] == 0
        with pytest.raises(ValueError, match="range 0"):
            a.extract([(0, 0, 0)])
    with rlz.RlzArchive(b"ACGT", none, b"", [0, 0, 0]) as a:
        assert len(a) == 3 and a.target(1) == b""
        data, offsets = a.extract_array([(0, 0, 0), (2, 0, 0)])
        assert len(data) == 0 and offsets.tolist() == [0, 0, 0]
        with pytest.raises(ValueError, match="range 1"):
            a.extract([(0, 0, 0), (1, 0, 1)])
    inp, archive = boundary
    data, offsets = archive.extract_array([])
    assert len(data) == 0 and offsets.tolist() == [0]
    assert archive.extract([(1, 0, 0), (0, 5, 5)]) == [b"", b""]  # all empty: nothing to launch
    assert archive.target(1) == b""


# ---- the boundary input ----------------------------------------------------------------------------------------------
def test_ranges_around_every_record_boundary(boundary):
    inp, archive = boundary
    B = len(inp["block"])
    ranges = []
    for tgt, base in ((0, 0), (2, 4911)):
        n = inp["lengths"][tgt]
        rec = inp["records"][(inp["records"]["start"] >= B + base) & (inp["records"]["start"] < B + base + n)]
        kinds = model.record_kinds(rec)
        edges = [int(rec["start"][i + 1]) - B - base for i in range(len(rec) - 1) if kinds[i] != kinds[i + 1]]
        assert len(edges) == 6  # F|L, L|R, R|L, L|F, F|L, L|F
        for e in edges:
            for lo in range(max(e - 20, 0), min(e + 20, n)):
                ranges += [(tgt, lo, min(lo + length, n)) for length in LENGTHS]
        for length in LENGTHS + (4095,):
            ranges += [(tgt, 0, length), (tgt, n - length, n)]
        ranges.append((tgt, 0, n))
    ranges += [(0, 0, 4095), (0, 500, 4596), (0, 814, 4911), (2, 807, 4904), (1, 0, 0)]
    assert {hi - lo for _, lo, hi in ranges} >= {0, 1, 15, 16, 17, 255, 256, 257, 4095, 4096, 4097, 4911}
    exp = check_against_model(archive, inp, ranges)
    assert exp[-6] == inp["targets"][2] and exp[-3] == inp["targets"][0][814:]
    random.Random(3).shuffle(ranges)  # other residues against the 16-byte chunks
    check_against_model(archive, inp, ranges)


def test_all_ranges_of_a_target_in_one_call(rlz):
    cut = model.boundary_cut()
    target = cut["targets"][0]
    assert len(target) == 300 and set(model.record_kinds(cut["records"]).tolist()) == {"F", "R", "L"}
    ranges = [(0, lo, hi) for lo in range(300) for hi in range(lo + 1, 301)]
    assert len(ranges) == 45150
    rng = random.Random(11)
    rng.shuffle(ranges)
    ranges += ranges[:500] + ranges[7000:7100]  # duplicates
    for _ in range(1000):                        # empty ranges, runs of them too
        at = rng.randrange(len(ranges) + 1)
        lo = rng.randrange(301)
        ranges[at:at] = [(0, lo, lo)] * rng.choice((1, 1, 1, 40))
    with rlz.RlzArchive(cut["block"], cut["records"], cut["literals"], cut["lengths"]) as a:
        data, offsets = a.extract_array(ranges)
    lens = np.array([hi - lo for _, lo, hi in ranges], dtype=np.uint64)
    assert np.array_equal(offsets, np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64))
    assert int(offsets[-1]) > 4_500_000
    assert data.tobytes() == b"".join(target[lo:hi] for _, lo, hi in ranges)


# ---- against the device's own factorisations -------------------------------------------------------------------------
def _mutated(ref, seed, rate=0.003):
    rng = np.random.default_rng(seed)
    t = ref.copy()
    at = rng.random(len(t)) < rate
    t[at] = gen.ACGT[rng.integers(0, 4, size=int(at.sum()))]
    return t.tobytes()


@pytest.mark.parametrize("with_rc", [True, False])
def test_device_factorisations(rlz, with_rc):
    ref_arr = gen.repeat_dna(60_000, seed=9, lo=16, hi=512)
    ref = ref_arr.tobytes()
    inverted = ref[:20_000] + rlz_model.revcomp(ref[20_000:31_000]) + ref[31_000:45_000]
    targets = [_mutated(ref_arr, 1), _mutated(ref_arr, 2)[5_000:50_001].lower(), inverted, b"", ref,
               _mutated(ref_arr, 3, rate=0.05)[:9_999]]
    ids = [f"t{j}" for j in range(6)]
    factors = rlz.rlz_factorize(ref, targets, with_rc=with_rc)
    literals = rlz.rlz_literals(targets, factors)
    decoded = rlz.rlz_decode(ref, factors, literals)
    rng = random.Random(17)
    ranges = []
    for _ in range(20_000):
        j = rng.choice((0, 1, 2, 4, 5))
        length = rng.randint(1, 400)
        lo = rng.randrange(0, len(targets[j]) - length + 1)
        ranges.append((j, lo, lo + length))
    ranges += [(j, 0, len(t)) for j, t in enumerate(targets)]
    with rlz.RlzArchive.build(ref, targets, with_rc=with_rc, ids=ids) as a:
        assert a.ids == ids and a.target_lengths == [len(t) for t in targets]
        got = a.extract(ranges)
        assert got == [targets[j].upper()[lo:hi] for j, lo, hi in ranges]
        for j, name in enumerate(ids):
            assert a.target(j) == decoded[j] == a.target(name)
        assert a.fetch("t2", 19_990, 20_050) == inverted[19_990:20_050]
        kinds = model.record_kinds(a._arrays["records"])
        assert ("R" in kinds) == with_rc and "F" in kinds  # (a nucleotide target has no literal against this block)
        assert a.info["z"] == sum(len(f) for f in factors)
    with rlz.RlzArchive.from_factors(ref, factors, literals) as b:
        assert b.ids is None and b.extract(ranges[:50]) == got[:50]
        with pytest.raises(KeyError):
            b.fetch("t2", 0, 1)


def test_multi_record_reference_into_a_torch_tensor(rlz):
    import torch
    refs = [gen.random_dna(700, seed=21).tobytes(), gen.random_dna(900, seed=22).tobytes(),
            gen.random_dna(500, seed=23).tobytes()]
    target = (refs[0][50:350] + rlz_model.revcomp(refs[1][100:500]) + refs[2][10:410] +
              rlz_model.revcomp(refs[0][400:650]) + refs[1][600:880] + rlz_model.revcomp(refs[2][5:300]))
    with rlz.RlzArchive.build(refs, [target, target[33:]]) as a:
        rec = a._arrays["records"]
        src = rec["ref"][rec["ref"] != rec["start"]]
        which = np.searchsorted([701, 1602], src & np.uint64(RC - 1), side="right")
        for strand in (0, 1):  # copies from each of the three records, on each strand
            assert set(which[(src >> np.uint64(63)) == strand].tolist()) == {0, 1, 2}
        rng = random.Random(2)
        ranges = [(0, 0, len(target)), (1, 0, len(target) - 33)]
        for _ in range(500):
            j = rng.randrange(2)
            lo = rng.randrange(0, len(target) - 40)
            ranges.append((j, lo, min(lo + rng.randint(0, 333), a.target_lengths[j])))
        exp, offsets = a.extract_array(ranges)
        assert exp[:len(target)].tobytes() == target
        total = len(exp)
        device = torch.device("cuda", a.info["device"])
        stream = torch.cuda.Stream(device=device)
        for shift in (0, 1):  # a 16-byte aligned output, and one that is not (byte stores)
            buf = torch.full((total + 64,), 0x55, dtype=torch.uint8, device=device)
            out = buf[shift:shift + total]
            torch.cuda.synchronize(device)
            with torch.cuda.stream(stream):
                wrote = a.extract_device(ranges, out.data_ptr(), total, stream=stream.cuda_stream)
            assert wrote == total
            host = buf.cpu().numpy()
            assert np.array_equal(host[shift:shift + total], exp)
            assert (host[:shift] == 0x55).all() and (host[shift + total:] == 0x55).all()
        # one byte short: refused, nothing written
        buf = torch.full((total,), 0x55, dtype=torch.uint8, device=device)
        with pytest.raises(ValueError, match="d_out_capacity"):
            a.extract_device(ranges, buf.data_ptr(), total - 1)
        assert bool((buf == 0x55).all())
        assert a.extract_device(ranges, buf.data_ptr(), total) == total  # (the null stream: behind torch's default stream)
        assert np.array_equal(buf.cpu().numpy(), exp)


# ---- refusals --------------------------------------------------------------------------------------------------------
OPEN_REFUSALS = [
    # (records, literals, target lengths): block ACGT
    ([(4, 4, 1)], b"", [4]),                              # the source ends one byte past the block
    ([(4, 3, 2 | RC)], b"", [3]),                         # the same on the other strand
    ([(4, 4, 0), (8, 2, 4)], b"", [6]),                   # a copy from the target: self-referential
    ([(4, 4, 0), (8, 1, 8)], b"x", [3, 2]),               # straddles the end of target 0
    ([(4, 4, 0), (8, 1, 8)], b"x", [4]),                  # a record behind the last target
    ([(4, 4, 0), (8, 1, 8)], b"x", [6]),                  # lengths that do not sum
    ([(4, 4, 0), (8, 1, 8)], b"x", []),                   # k == 0 with records
    ([(4, 1, 4), (5, 1, 5)], b"x", [2]),                  # one literal symbol too few
    ([(4, 1, 4), (5, 1, 5)], b"xyz", [2]),                # one too many
    ([(4, 4, 0), (9, 1, 9)], b"x", [6]),                  # tiling
    ([(4, 4, 0), (8, 2, 8)], b"x", [6]),                  # literal length
    ([], b"", [1]),                                       # no records, a non-empty target
    ([], b"x", []),                                       # no records, a literal
]


@pytest.mark.parametrize("case", range(len(OPEN_REFUSALS)))
def test_open_refusals(native, case):
    records, literals, lengths = OPEN_REFUSALS[case]
    rule, index = model.open_refusal(4, records, len(literals), lengths)
    with pytest.raises(ValueError) as e:
        native.RlzArchiveHandle.open_records(b"ACGT", records, literals, lengths)
    msg = str(e.value)
    assert f"record {index} " in msg and f"breaks {rule}" in msg, msg
    if case == 2:
        assert rule == model.SOURCE_IN_BLOCK and "source range" not in msg


def test_open_refusal_names_the_first_record_of_many(native):
    inp = model.boundary_input()
    rec = inp["records"].copy()
    rec["ref"][601] += np.uint64(1200)  # the reverse-complement copy of 900 now ends 299 bytes past the block
    rec["ref"][900] = np.uint64(5001)   # and a later record copies from the first target
    assert model.open_refusal(5001, rec, len(inp["literals"]), inp["lengths"]) == (model.SOURCE_IN_BLOCK, 601)
    with pytest.raises(ValueError, match="record 601 breaks source inside the block"):
        native.RlzArchiveHandle.open_records(inp["block"], rec, inp["literals"], inp["lengths"])


def test_extract_refusals(boundary):
    inp, archive = boundary
    n = inp["lengths"][0]
    good = [(0, 0, 10), (2, 5, 5)]
    for bad, rule in (((3, 0, 0), model.BAD_TARGET), ((0, 11, 10), model.LO_ABOVE_HI), ((0, 0, n + 1), model.HI_BEYOND),
                      ((1, 0, 1), model.HI_BEYOND)):
        ranges = good + [bad]
        assert model.extract_refusal(inp["lengths"], ranges) == (rule, 2)
        with pytest.raises(ValueError, match=f"range 2: .*{rule}"):
            archive.extract(ranges)
    assert archive.extract(good + [(0, 0, n)])[2] == inp["targets"][0]  # hi == length passes
    # 2^32 bytes or more in one call: refused at the range that reaches them, before anything is launched
    many = np.tile(np.array([[0, 0, n]], dtype=np.uint64), (900_000, 1))
    reached = -(-(1 << 32) // n) - 1
    assert (reached + 1) * n >= 1 << 32 > reached * n
    with pytest.raises(ValueError, match=f"range {reached}: .*2\\^32 bytes"):
        archive.extract_array(many)
    data, offsets = archive.extract_array(many[:1000])
    assert len(data) == 1000 * n and data[-n:].tobytes() == inp["targets"][0] and int(offsets[-1]) == 1000 * n


def test_complement_of_a_non_nucleotide(native):
    block = b"ACG\x01TTA"
    records, literals = [(7, 3, 2 | RC), (10, 1, 10)], b"x"
    faults = []
    text = model.expand(block, records, literals, faults)
    assert faults == [1]
    with native.RlzArchiveHandle.open_records(block, records, literals, [4]) as h:
        ranges = [(0, 3, 4), (0, 0, 1), (0, 2, 4), (0, 0, 4), (0, 1, 2)]
        with pytest.raises(ValueError, match=r"range 3 breaks complement of a non-nucleotide: position 1 of target 0 "):
            h.extract_array(ranges)
        with pytest.raises(ValueError, match=r"range 0 breaks complement of a non-nucleotide: position 1 of target 0 "):
            h.extract_array([(0, 1, 4)] + ranges)
        data, offsets = h.extract_array(ranges[:3])  # the same handle, without the offending ranges
        assert data.tobytes() == b"xA" + text[2:4] and offsets.tolist() == [0, 1, 2, 4]


def test_complement_of_a_non_nucleotide_inside_a_whole_chunk(native):
    block = b"ACGT" * 5 + b"\x01" + b"TTGCA" * 4
    records = [(41, 40, 1 | RC)]  # the reverse complement of block[1:41]: the separator is the source of position 20
    faults = []
    text = model.expand(block, records, b"", faults)
    assert faults == [20] and len(text) == 40
    with native.RlzArchiveHandle.open_records(block, records, b"", [40]) as h:
        for ranges, where in (([(0, 0, 40)], "range 0 breaks complement of a non-nucleotide: position 20 "),
                              ([(0, 0, 16), (0, 3, 40), (0, 20, 21)], "range 1 breaks complement of a non-nucleotide: position 20 "),
                              ([(0, 0, 20), (0, 21, 40), (0, 5, 37)], "range 2 breaks complement of a non-nucleotide: position 20 ")):
            with pytest.raises(ValueError, match=where):
                h.extract_array(ranges)
        data, offsets = h.extract_array([(0, 0, 20), (0, 21, 40), (0, 4, 20)])
        assert data.tobytes() == text[:20] + text[21:] + text[4:20]


# ---- the handle ------------------------------------------------------------------------------------------------------
def test_two_handles_and_other_calls_in_between(rlz, native, boundary):
    inp, archive = boundary
    cut = model.boundary_cut()
    with rlz.RlzArchive(cut["block"], cut["records"], cut["literals"], cut["lengths"]) as other:
        for lo in (0, 100, 283):
            assert archive.fetch(0, lo, lo + 2000) == inp["targets"][0][lo:lo + 2000]
            assert other.fetch(0, lo, 300) == cut["targets"][0][lo:]
        text = gen.repeat_dna(50_000, seed=4, lo=16, hi=512).tobytes()
        z = native.count_factors(text)
        assert archive.fetch(2, 0, 4904) == inp["targets"][2] and z > 0
        assert len(native.factorize_array(text)) == z
        assert other.target(0) == cut["targets"][0] and archive.target(0) == inp["targets"][0]


def test_four_threads_on_one_handle(boundary):
    inp, archive = boundary
    errors = []

    def work(seed):
        try:
            rng = random.Random(seed)
            for _ in range(20):
                ranges = []
                for _ in range(200):
                    j = rng.choice((0, 2))
                    lo = rng.randrange(inp["lengths"][j])
                    ranges.append((j, lo, min(lo + rng.randint(0, 300), inp["lengths"][j])))
                if archive.extract(ranges) != [inp["targets"][j][lo:hi] for j, lo, hi in ranges]:
                    errors.append(seed)
        except Exception as e:  # noqa: BLE001 (reported below)
            errors.append(e)

    threads = [threading.Thread(target=work, args=(s,)) for s in range(4)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert errors == []


def test_use_after_close_and_file_round_trip(rlz, tmp_path):
    inp = model.boundary_input()
    ids = ["first", "empty", "shifted"]
    a = rlz.RlzArchive(inp["block"], inp["records"], inp["literals"], inp["lengths"], ids=ids)
    path = tmp_path / "archive.npz"
    a.save(path)
    assert a.fetch("shifted", 0, 9) == inp["targets"][2][:9]
    a.close()
    a.close()
    for call in (lambda: a.extract([(0, 0, 1)]), lambda: a.fetch(0, 0, 1), lambda: a.target("first"), lambda: a.info,
                 lambda: a.extract_array([]), lambda: a.extract_device([], 0, 0), lambda: a.save(path)):
        with pytest.raises(ValueError, match="closed"):
            call()
    with rlz.RlzArchive.load(path) as b:
        assert b.ids == ids and b.target_lengths == inp["lengths"] and len(b) == 3
        assert b.target("first") == inp["targets"][0] and b.fetch("shifted", 1390, 1400) == inp["targets"][2][1390:1400]
        assert b.info["z"] == len(inp["records"]) and b.info["device_bytes"] > 0
    with pytest.raises(ValueError, match="closed"):
        b.target(0)
