"""The maximal repeats of the reference on the device (rlz_repeats.hip, rlz_index_repeats_api.hip).  Every case compares
RlzIndex.repeats with the array model (tests/rlz_repeats_model.RepeatsModel, itself checked against the definition in
tests/test_rlz_repeats_host.py) by integer equality -- every record field, the offsets and every hit field in the stated
order -- and RlzIndex.repeat_count with the number of records."""
import os
import random
import subprocess
import sys
import threading
from pathlib import Path

import numpy as np
import pytest

import rlz_locate_model as lm
import rlz_model as model
import rlz_repeats_model as rm

pytestmark = pytest.mark.gpu

KEYS = ("position", "length", "count", "record", "record_offset", "palindrome", "offsets", "hit_position", "hit_record",
        "hit_record_offset", "hit_is_rc")


@pytest.fixture(scope="module")
def rlz():
    from nolzss_amd import _noLZSS
    assert _noLZSS.device_count() >= 1, "no MI355X visible"
    from nolzss_amd.genomics import rlz
    return rlz


def _dna(n, seed, alphabet=b"ACGT"):
    rng = np.random.default_rng(seed)
    return np.frombuffer(alphabet, dtype=np.uint8)[rng.integers(0, len(alphabet), n)].tobytes()


_MODELS = {}


def model_of(refs, with_rc):
    """the array model of a reference, computed once and shared"""
    key = (tuple(bytes(r) for r in refs), with_rc)
    if key not in _MODELS:
        _MODELS[key] = rm.RepeatsModel(list(key[0]), with_rc)
    return _MODELS[key]


def same(got, exp, what=""):
    assert sorted(got) == sorted(exp) == sorted(KEYS)
    for key in KEYS:
        assert got[key].dtype == exp[key].dtype, (key, got[key].dtype, exp[key].dtype)
        if not np.array_equal(got[key], exp[key]):
            at = int(np.flatnonzero(got[key] != exp[key])[0]) if got[key].shape == exp[key].shape else None
            raise AssertionError(f"{key} differs {what} (shapes {got[key].shape} {exp[key].shape}, first at {at}): "
                                 f"{got[key][:12]} != {exp[key][:12]}")


def check_query(ix, m, min_length=1, min_count=2, max_hits=0):
    exp = m.repeats(min_length, min_count, max_hits)
    got = ix.repeats(min_length, min_count, max_hits)
    same(got, exp, f"(min_length {min_length}, min_count {min_count}, max_hits {max_hits})")
    assert ix.repeat_count(min_length, min_count) == len(got["position"])
    return got


def check(rlz, refs, with_rc, prefix_syms=0, **rules):
    with rlz.RlzIndex.build(refs, with_rc=with_rc, prefix_syms=prefix_syms) as ix:
        return check_query(ix, model_of(refs, with_rc), **rules)


# ---- 1. hand cases -----------------------------------------------------------------------------------------------------
def test_hand_cases(rlz):
    got = check(rlz, [b"AAAAAA"], False)
    assert got["length"].tolist() == [1, 2, 3, 4, 5] and got["count"].tolist() == [6, 5, 4, 3, 2]
    assert len(check(rlz, [b"ACGT"], True)["position"]) == 0
    got = check(rlz, [b"ACGT", b"ACGT"], True)
    assert got["palindrome"].tolist() == [True] and got["count"].tolist() == [4]
    assert got["hit_position"].tolist() == [0, 0, 5, 5] and got["hit_is_rc"].tolist() == [False, True, False, True]
    got = check(rlz, [b"CAGGTTACCTG"], True, min_length=3)  # w T rc(w)
    assert (got["position"].tolist(), got["length"].tolist()) == ([0], [5])
    assert got["hit_position"].tolist() == [0, 6] and got["hit_is_rc"].tolist() == [False, True]
    got = check(rlz, [b"ACGTCC", b"GGACGT"], False, min_length=3)  # a record's start and another record's end
    assert got["hit_position"].tolist() == [0, 9] and got["hit_record"].tolist() == [0, 1] and got["hit_record_offset"].tolist() == [0, 2]
    got = check(rlz, [b"GGACG", b"TTTCC", b"AACGTTTA"], False, min_length=3)  # ACG | TTT: no repeat crosses the separator
    assert got["length"].tolist() == [3, 3] and got["record"].tolist() == [0, 1] and got["record_offset"].tolist() == [2, 0]
    check(rlz, [b"GGACG", b"TTTCC", b"AACGTTTA"], True)
    check(rlz, [b"A", b"", b"T"], True)


# ---- 2. geometry -------------------------------------------------------------------------------------------------------
# |X| = B + 1 ranks without the reverse complement and 2 B + 2 with it: the blocks of 16 entries of the pyramids and the
# tiles of 1024 ranks of the scans begin and end around these sizes, on one side or the other.  Without the reverse
# complement B = 14, 15, 16 and 1022, 1023, 1024 give 15, 16, 17 and 1023, 1024, 1025 ranks; an index of one rank does
# not exist (an empty reference block is refused at open), B = 1 gives the smallest, two ranks.
@pytest.mark.parametrize("with_rc", [True, False])
@pytest.mark.parametrize("B", [1, 2, 6, 7, 14, 15, 16, 17, 510, 511, 512, 1022, 1023, 1024, 1025])
def test_block_sizes_around_the_pyramid_blocks_and_the_tiles(rlz, B, with_rc):
    for alphabet, seed in ((b"AC", B), (b"ACGT", 1000 + B), (b"A", 0)):
        check(rlz, [_dna(B, seed, alphabet)], with_rc)
    if B >= 6:
        half = _dna(B // 2 - 1, 2000 + B, b"AT")
        check(rlz, [half, b"", half + b"A" * (B - 2 * len(half) - 2)], with_rc)  # B bases and separators in all


UNIT7 = b"ACGGTCA"
LONG = {"a1100": [b"A" * 1100], "unit7x1100": [UNIT7 * 1100]}


@pytest.mark.parametrize("with_rc", [True, False])
@pytest.mark.parametrize("name", sorted(LONG))
def test_intervals_beyond_a_tile_and_across_tile_seams(rlz, name, with_rc):
    refs = LONG[name]
    with rlz.RlzIndex.build(refs, with_rc=with_rc) as ix:
        m = model_of(refs, with_rc)
        got = check_query(ix, m)
        assert int(got["count"].max()) > 1024 and len(got["hit_position"]) > 100_000
        check_query(ix, m, max_hits=64)
        check_query(ix, m, min_length=500, min_count=3, max_hits=0)


# ---- 3. the rules at their edges ---------------------------------------------------------------------------------------
EDGE_REFS = [_dna(180, 61, b"AC"), _dna(120, 62), _dna(90, 63, b"AT") + b"GAATTC" + _dna(40, 64) + b"GAATTC"]


@pytest.mark.parametrize("with_rc", [True, False])
def test_min_length_min_count_and_max_hits_at_a_value_and_beside_it(rlz, with_rc):
    m = model_of(EDGE_REFS, with_rc)
    with rlz.RlzIndex.build(EDGE_REFS, with_rc=with_rc) as ix:
        everything = check_query(ix, m)
        lengths, counts = sorted(set(everything["length"].tolist())), sorted(set(everything["count"].tolist()))
        assert len(lengths) >= 6 and len(counts) >= 6
        if with_rc:
            assert everything["palindrome"].any() and not everything["palindrome"].all()
        for length in (lengths[0], lengths[len(lengths) // 2], lengths[-1]):
            kept = check_query(ix, m, min_length=length)
            assert int(kept["length"].min()) == length
            fewer = check_query(ix, m, min_length=length + 1)
            assert len(fewer["position"]) == int((everything["length"] > length).sum()) < len(kept["position"])
        for count in (counts[0], counts[len(counts) // 2], counts[-1]):
            kept = check_query(ix, m, min_count=count)
            assert int(kept["count"].min()) == count
            fewer = check_query(ix, m, min_count=count + 1)
            assert len(fewer["position"]) == int((everything["count"] > count).sum()) < len(kept["position"])
        for count in (counts[1], counts[len(counts) // 2], counts[-1]):
            for cap in (count - 1, count, 0):
                got = check_query(ix, m, max_hits=cap)
                reported = everything["count"] <= cap if cap else np.ones(len(everything["count"]), dtype=bool)
                assert int(got["offsets"][-1]) == int(everything["count"][reported].sum())
                assert np.array_equal(np.diff(got["offsets"]) > 0, reported)
        check_query(ix, m, min_length=10 ** 12)
        assert ix.repeat_count(min_length=1, min_count=10 ** 12) == 0 and ix.repeat_count(2 ** 32 - 1, 2 ** 32 - 1) == 0


@pytest.mark.parametrize("with_rc", [True, False])
@pytest.mark.parametrize("P", [1, 12])
def test_the_prefix_table_plays_no_part(rlz, P, with_rc):
    check(rlz, EDGE_REFS, with_rc, prefix_syms=P, min_length=2, max_hits=9)


@pytest.mark.parametrize("seed, with_rc", [(1, True), (2, False), (3, True), (4, False)])
def test_seeded_cases(rlz, seed, with_rc):
    rng = random.Random(7000 + seed)
    for i in range(12):
        refs = lm.case(rng, hi=24 if i % 3 else 200)
        check(rlz, refs, with_rc, min_length=rng.choice((1, 2, 4)), min_count=rng.choice((2, 3)), max_hits=rng.choice((0, 3, 64)))


# ---- 4. the download chunks, in child processes -------------------------------------------------------------------------
CHUNK_REFS = [_dna(70, 71, b"AC"), _dna(50, 72, b"AC") + b"ACGT", b"ACGT" + _dna(30, 73)]
CHILD = """
import sys
import numpy as np
from nolzss_amd.genomics import rlz
refs = [bytes.fromhex(h) for h in sys.argv[2:]]
with rlz.RlzIndex.build(refs) as ix:
    got = ix.repeats(min_length=2, min_count=2, max_hits=0)
    got["repeat_count"] = np.array([ix.repeat_count(2, 2)])
np.savez(sys.argv[1], **got)
"""


@pytest.mark.parametrize("chunk", [1, 3, 7])
def test_chunk_seams_inside_the_hits_of_a_record_and_between_records(rlz, tmp_path, chunk):
    exp = model_of(CHUNK_REFS, True).repeats(2, 2, 0)
    sizes = np.diff(exp["offsets"]).tolist()
    assert len(sizes) > 20 and max(sizes) > 7 and min(sizes) == 2  # seams fall inside a record's hits and between records
    out = tmp_path / "got.npz"
    root = Path(__file__).resolve().parent.parent
    env = dict(os.environ, NOLZSS_RLZ_LOCATE_CHUNK=str(chunk), PYTHONPATH=str(root))
    subprocess.run([sys.executable, "-c", CHILD, str(out)] + [r.hex() for r in CHUNK_REFS], check=True, env=env, cwd=str(root),
                   timeout=120)
    got = dict(np.load(out))
    assert got.pop("repeat_count").tolist() == [len(sizes)]
    same(got, exp, f"(chunk {chunk})")


# ---- 5. a block of 2^16 bases with planted copies -----------------------------------------------------------------------
def planted_block():
    rng = random.Random(81)
    block = bytearray(_dna(1 << 16, 82))
    for _ in range(60):  # forward and inverted copies with 1 % substitutions: nested repeats around every difference
        length = rng.randint(40, 600)
        src, dst = rng.randrange(len(block) - length), rng.randrange(len(block) - length)
        piece = bytes(block[src:src + length])
        if rng.random() < 0.5:
            piece = model.revcomp(piece)
        piece = bytearray(piece)
        for i in range(length):
            if rng.random() < 0.01:
                piece[i] = rng.choice(b"ACGT")
        block[dst:dst + length] = piece
    return bytes(block)


@pytest.mark.parametrize("with_rc", [True, False])
def test_a_block_of_2_to_the_16_bases_with_planted_copies(rlz, with_rc):
    refs = [planted_block()]
    m = model_of(refs, with_rc)
    with rlz.RlzIndex.build(refs, with_rc=with_rc) as ix:
        got = check_query(ix, m, min_length=20, max_hits=64)
        assert len(got["position"]) >= 40 and int(got["length"].max()) >= 100
        if with_rc:
            assert got["hit_is_rc"].any()
        got = check_query(ix, m, min_length=8, max_hits=0)  # more records than a tile of the sort holds
        assert len(got["position"]) > 8192
        check_query(ix, m, min_length=12, min_count=3, max_hits=2)


# ---- 6. other behaviour ------------------------------------------------------------------------------------------------
def test_two_threads_query_one_handle(rlz):
    m = model_of(EDGE_REFS, True)
    rules = [(1, 2, 0), (3, 3, 5)]
    exp = [m.repeats(*r) for r in rules]
    with rlz.RlzIndex.build(EDGE_REFS) as ix:
        out, errors = [[None] * 6, [None] * 6], []

        def work(t):
            try:
                for rep in range(6):
                    out[t][rep] = ix.repeats(*rules[t])
                    assert ix.repeat_count(*rules[t][:2]) == len(exp[t]["position"])
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
                same(got, exp[t])


def test_the_handle_is_untouched_by_a_query(rlz):
    rng = random.Random(91)
    refs = lm.case(rng, lo=150, hi=400, records=3)
    targets = [refs[0][20:120] + model.revcomp(refs[-1] or refs[0])[:80], b"", refs[0][::-1]]
    patterns = lm.patterns(rng, refs, 300)
    with rlz.RlzIndex.build(refs) as ix:
        factors, located, info = ix.factorize(targets), ix.locate(patterns, max_hits=20), ix.info()
        check_query(ix, model_of(refs, True))
        check_query(ix, model_of(refs, True), min_length=4, max_hits=3)
        after, located_after = ix.factorize(targets), ix.locate(patterns, max_hits=20)
        assert ix.info() == info and len(factors) == len(after)
        assert all(np.array_equal(a, b) for a, b in zip(factors, after))
        assert all(np.array_equal(located[k], located_after[k]) for k in located)


def _profiled(native, fn):
    native.profile_enable(True)
    try:
        native.profile_reset()
        out = fn()
        return out, native.profile_report()
    finally:
        native.profile_enable(False)
        native.profile_reset()


def test_the_flags_are_computed_again_when_the_arena_grows(rlz):
    """an open leaves the arena empty: the first query reserves for the ranks, learns the number of records, reserves
    again -- the slab is replaced -- and runs the flags a second time in it, and likewise for the hits; the next call finds
    room and runs every stage once"""
    from nolzss_amd import _noLZSS as native
    refs = [UNIT7 * 300, _dna(300, 51)]
    exp = model_of(refs, True).repeats(1, 2, 0)
    with rlz.RlzIndex.build(refs) as ix:
        native.debug_trim_arenas()
        first, report = _profiled(native, lambda: ix.repeats(1, 2, 0))
        assert report["rlz_repeat_flags"][0] > 1 and report["rlz_repeat_hits"][0] == 1 and report["rlz_index_repeats"][0] == 1
        again, report = _profiled(native, lambda: ix.repeats(1, 2, 0))
        assert report["rlz_repeat_flags"][0] == report["rlz_repeat_left"][0] == report["rlz_repeat_sort"][0] == 1
        assert report["rlz_repeat_hits"][0] == 1 and report["rlz_repeat_records"][0] == report["repeats_d2h"][0] == 1
        count, report = _profiled(native, lambda: ix.repeat_count(1, 2))
        assert count == len(exp["position"]) and report["rlz_repeat_flags"][0] == 1 and "rlz_repeat_sort" not in report
        for got in (first, again):
            same(got, exp)
