"""Who holds device memory, counted: every resident handle (index, archive, finder, pileup, cohort, dot plot) keeps its
allocations in DeviceBufs (device_buf.hpp), and nolzss_debug_device_buffers reads how many of them are live in the process
and the bytes they asked for.  Every case reads the counters before and after and compares the two -- a delta, because
module fixtures of other files may hold handles --: open, use and close; growth under the smallest first sizes, in a child
process; opens and appends that are refused after the handle's arrays were allocated; an index closed before what was
opened over it."""
import contextlib
import gc
import os
import random
import subprocess
import sys

import pytest

from test_gpu_rlz_archive_pack_refusals import CASES, LENGTHS, VALID

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


def dna(rng, n):
    return bytes(rng.choice(b"ACGT") for _ in range(n))


RNG = random.Random(2024)
REF = dna(RNG, 600)
SAMPLE = REF[:300] + b"GT" + REF[300:]  # two bases inserted: every read over them logs one insertion event
READS = [SAMPLE[lo:lo + 100] for lo in range(230, 275, 5)]  # 9 reads of 100 bases over the insertion
TARGETS = [REF[40:160], REF[200:230] + (b"T" if REF[230:231] != b"T" else b"A") + REF[231:330], REF[500:590]]
CALLS = [bytes(RNG.choice(b"N-") if RNG.random() < 0.3 else RNG.choice(b"ACGT") for _ in range(len(REF))) for _ in range(3)]


@contextlib.contextmanager
def nothing_kept(native):
    """-> the counters before the block; they are the same behind it"""
    gc.collect()
    before = native.debug_device_buffers()
    yield before
    gc.collect()
    assert native.debug_device_buffers() == before


def delta(native, before):
    now = native.debug_device_buffers()
    return now[0] - before[0], now[1] - before[1]


def test_an_index_holds_one_buffer_of_the_bytes_it_reports(native, rlz):
    with nothing_kept(native) as before:
        with rlz.RlzIndex.build([REF]) as ix:
            assert delta(native, before) == (1, ix.info()["device_bytes"]) and ix.info()["device_bytes"] > len(REF) // 4
            counts = [int(c) for c in ix.count_factors(TARGETS)]
            assert counts[0] == counts[2] == 1 and counts[1] >= 2
            assert delta(native, before) == (1, ix.info()["device_bytes"])  # (a match changes nothing)


def test_an_archive_of_host_records_holds_its_three_arrays(native, rlz):
    with nothing_kept(native) as before:
        with rlz.RlzArchive.build(REF, TARGETS) as arc:
            buffers, held = delta(native, before)
            # (the position sample may keep one word where it reports none: at most four bytes more)
            assert buffers == 3 and arc.info["device_bytes"] <= held <= arc.info["device_bytes"] + 4
            assert arc.info["device_bytes"] >= len(REF) + 16 * arc.info["z"]
            assert arc.extract([(j, 0, len(t)) for j, t in enumerate(TARGETS)]) == TARGETS
            assert delta(native, before) == (buffers, held)


def test_an_archive_over_an_index_and_its_finder(native, rlz):
    with nothing_kept(native) as start:
        with rlz.RlzIndex.build([REF]) as ix:
            with nothing_kept(native) as before:
                with rlz.RlzArchive.from_index(ix) as arc:
                    assert delta(native, before) == (1, arc.info["device_bytes"]) and arc.info["device_bytes"] == len(REF)
                    (info,) = arc.append(TARGETS)
                    assert info["reallocated"] == 1 and info["device_bytes"] == arc.info["device_bytes"]
                    buffers, held = delta(native, before)
                    assert buffers == 3 and held >= arc.info["device_bytes"] >= len(REF) + 16 * info["capacity_records"]
                    with nothing_kept(native) as around:
                        with arc.finder(max_pattern_length=16) as finder:
                            assert delta(native, around) == (3, finder.info["device_bytes"]) and finder.info["device_bytes"] > 0
                            assert finder.count([REF[50:60], b"ACGTACGTACGTACGT"]).tolist()[0] >= 1
                            assert delta(native, around) == (3, finder.info["device_bytes"])
                    assert arc.extract([(j, 0, len(t)) for j, t in enumerate(TARGETS)]) == TARGETS
            assert delta(native, start) == (1, ix.info()["device_bytes"])


def test_a_pileup_holds_counters_log_and_allele_table(native, rlz):
    with rlz.RlzIndex.build([REF]) as ix:
        with nothing_kept(native) as before:
            with ix.pileup(normalize_indels=True) as pile:
                assert delta(native, before) == (1, pile.info["device_bytes"]) and pile.info["log_bytes"] == 0
                pile.add(READS)
                info = pile.info
                assert info["insertion_events"] == len(READS) and info["log_bytes"] >= 24 * len(READS)
                assert delta(native, before) == (2, info["device_bytes"] + info["log_bytes"])  # (device_bytes leaves the log out)
                found = pile.insertions(1, (0, 1))
                assert len(found) == 1 and int(found[0]["count"]) == len(READS) and int(found[0]["length"]) == 2
                buffers, held = delta(native, before)
                assert buffers == 3 and held >= info["device_bytes"] + info["log_bytes"] + 32 * len(found)
                assert pile.consensus()["insertions"] == 1
                assert len(pile.variants(2, (1, 2))) >= 1 and delta(native, before) == (buffers, held)


def test_a_cohort_holds_its_planes(native, rlz):
    with rlz.RlzIndex.build([REF]) as ix:
        with nothing_kept(native) as before:
            with ix.cohort() as co, ix.pileup(normalize_indels=True) as pile:
                held_by_pileup = pile.info["device_bytes"]
                assert delta(native, before) == (1, held_by_pileup) and co.info["device_bytes"] == 0
                for n, calls in enumerate(CALLS):
                    assert co.add_calls(calls)["sample"] == n
                    assert delta(native, before) == (2, held_by_pileup + co.info["device_bytes"])
                pile.add(READS)
                co.add(pile)
                after_add = pile.info
                assert delta(native, before) == (3, held_by_pileup + after_add["log_bytes"] + co.info["device_bytes"])
                assert co.info["device_bytes"] == co.info["capacity"] * 3 * 8 * ((len(REF) + 63) // 64) > 0
                assert co.distances()["differences"].shape == (4, 4) and len(co.sites(0)) > 0
                assert delta(native, before) == (3, held_by_pileup + after_add["log_bytes"] + co.info["device_bytes"])


def test_a_dot_plot_holds_its_records(native):
    with nothing_kept(native) as before:
        with native.DotPlot.from_text(REF + REF[100:400]) as plot:
            assert delta(native, before) == (1, 24 * plot.info["z"]) and plot.info["z"] > 1
            out = plot.render((0, 900), (0, 900), width=30, height=30)
            assert out["max_forward"].shape == (30, 30) and int(out["max_forward"].max()) > 0
            assert delta(native, before) == (1, 24 * plot.info["z"])


CHILD = r'''
import random, sys
sys.path.insert(0, "tests")
import numpy as np
import rlz_cohort_model as hm
from nolzss_amd import _noLZSS as native
from nolzss_amd.genomics import rlz
live = native.debug_device_buffers
start = live()
assert start == (0, 0)
rng = random.Random(99)
ref = bytes(rng.choice(b"ACGT") for _ in range(600))
with rlz.RlzIndex.build([ref]) as ix:
    base = live()
    assert base == (1, ix.info()["device_bytes"])

    # nine samples into a cohort that starts with room for one
    samples = [bytes(rng.choice(b"N-") if rng.random() < 0.3 else rng.choice(b"ACGT") for _ in range(600)) for _ in range(9)]
    calls = [hm.calls_from_bytes(s, ref) for s in samples]
    with ix.cohort() as co:
        capacities = []
        for n, s in enumerate(samples):
            assert co.add_calls(s)["sample"] == n
            capacities.append(co.info["capacity"])
            assert live() == (base[0] + 1, base[1] + co.info["device_bytes"]), (n, live())  # replaced, none added
            for k in range(n + 1):
                assert co.calls(k) == calls[k], (n, k)
        assert capacities == [1, 2, 4, 4, 8, 8, 8, 8, 16]
        diff, comp = hm.distances(calls)
        got = co.distances()
        assert got["differences"].tolist() == diff and got["compared"].tolist() == comp
    assert live() == base

    # batches with a planted insertion each into a pileup whose log starts with room for one event
    batches, total = [], []
    for b in range(4):
        at = 100 + 120 * b
        sample = ref[:at] + (b"ACG", b"CGT", b"GTA", b"TAC")[b] + ref[at:]
        batches.append([sample[lo:lo + 100] for lo in range(at - 70, at - 30, 10)])
        total += batches[-1]
    with ix.pileup(normalize_indels=True) as pile, ix.pileup(normalize_indels=True) as once:
        held = live()
        assert held == (base[0] + 2, base[1] + 2 * pile.info["device_bytes"])
        log_sizes, seen = [], []
        for b, reads in enumerate(batches):
            pile.add(reads)
            info = pile.info
            log_sizes.append(info["log_bytes"])
            assert info["insertion_events"] == 4 * (b + 1) and info["log_bytes"] >= 24 * info["insertion_events"]
            assert live()[0] == held[0] + (1 if b == 0 else 2), (b, live())  # the log; the allele table from the first read on
            found = pile.insertions(1, (0, 1))
            assert live()[0] == held[0] + 2 and live()[1] >= held[1] + info["log_bytes"] + 32 * len(found)
            rows = [(int(r["position"]), int(r["length"]), int(r["count"])) for r in found]
            assert rows[:len(seen)] == seen and len(rows) == b + 1 and rows[-1][1:] == (3, 4), rows  # earlier events read back
            seen = rows
        assert sum(1 for a, b in zip(log_sizes, log_sizes[1:]) if b > a) >= 2, log_sizes
        once.add(total)
        assert np.array_equal(pile.counts(), once.counts())
        assert np.array_equal(pile.insertions(1, (0, 1)), once.insertions(1, (0, 1)))
        a, b = pile.consensus(return_map=True), once.consensus(return_map=True)
        assert a["records"] == b["records"] and np.array_equal(a["starts"], b["starts"]) and a["insertions"] == 4
    assert live() == base

    # appends into an archive until its arrays have been replaced three times
    with rlz.RlzArchive.from_index(ix) as arc:
        assert live() == (base[0] + 1, base[1] + arc.info["device_bytes"])
        targets, moved, steps = [], 0, 0
        while moved < 3:
            lo, n = rng.randrange(0, 500), rng.randrange(20, 90)
            piece = bytearray(ref[lo:lo + n])
            piece[n // 2] = rng.choice(b"ACGT")
            (info,) = arc.append([bytes(piece)])
            targets.append(bytes(piece))
            moved += info["reallocated"]
            steps += 1
            assert steps <= 40 and info["capacity_records"] >= info["z"] and info["device_bytes"] == arc.info["device_bytes"]
            assert live()[0] == base[0] + 3 and live()[1] >= base[1] + info["device_bytes"], (steps, live())
            assert arc.extract([(j, 0, len(t)) for j, t in enumerate(targets)]) == targets, steps
    assert live() == base
assert live() == start
print("ok", capacities[-1], log_sizes[-1], steps)
'''


def test_growth_replaces_a_buffer_and_adds_none_in_a_child_process(native):
    """NOLZSS_RLZ_COHORT_SAMPLES=1 and NOLZSS_RLZ_PILEUP_LOG_EVENTS=1 for a whole process: the planes double four times,
    the log grows with the batches, the archive's arrays are replaced three times; after every step each handle holds as
    many buffers as before it, everything reads back, and after the closes nothing is held"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, NOLZSS_RLZ_COHORT_SAMPLES="1", NOLZSS_RLZ_PILEUP_LOG_EVENTS="1")
    r = subprocess.run([sys.executable, "-c", CHILD], cwd=root, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("ok 16 "), r.stdout[-2000:] + r.stderr[-4000:]


# the cases no container file can hold: their target lengths do not sum to the decoded length of the header, which the
# writer and the reader of the container both refuse on the host
WRITER_REFUSES = {"a record behind the last target", "lengths sum to one more than the targets",
                  "targets sum to one more than the lengths"}
assert WRITER_REFUSES <= set(CASES)


@pytest.mark.parametrize("name", list(CASES))
def test_a_refused_packed_open_gives_its_arrays_back(native, rlz, name, tmp_path):
    """open_packed allocates the handle's three arrays and then checks the sections on the device: every corruption case of
    tests/test_gpu_rlz_archive_pack_refusals.py, at the handle and, but for WRITER_REFUSES, as a file through RlzArchive.load"""
    change, lengths = CASES[name][:2]
    sections = {**VALID, **change}
    with nothing_kept(native):
        with pytest.raises(ValueError):
            native.RlzArchiveHandle.open_packed(sections, lengths)
    path = tmp_path / "broken.rlz"
    if name in WRITER_REFUSES:
        with pytest.raises(ValueError, match="inconsistent sizes"):
            rlz.write_packed_archive(path, sections, lengths)
        return
    rlz.write_packed_archive(path, sections, lengths)
    with nothing_kept(native):
        with pytest.raises(ValueError):
            rlz.RlzArchive.load(path)


def test_the_valid_packed_archive_loads_and_closes(native, rlz, tmp_path):
    path = tmp_path / "valid.rlz"
    rlz.write_packed_archive(path, VALID, LENGTHS)
    with nothing_kept(native) as before:
        with rlz.RlzArchive.load(path) as arc:
            buffers, held = delta(native, before)
            assert buffers == 3 and arc.info["device_bytes"] <= held <= arc.info["device_bytes"] + 4
            assert len(arc.target(2)) == LENGTHS[2]


def test_refused_finder_opens_queries_and_appends_keep_nothing(native, rlz):
    with rlz.RlzIndex.build([REF]) as ix, rlz.RlzIndex.build([REF]) as twin, rlz.RlzArchive.from_index(ix) as arc:
        arc.append(TARGETS[:1])
        arc.append(TARGETS[1:])  # a grown archive
        with nothing_kept(native) as before:
            with pytest.raises(ValueError, match="bound to another index"):
                native.RlzFinderHandle.open(arc._live(), twin._live())
            with pytest.raises(ValueError, match="max_pattern_length"):
                arc.finder(max_pattern_length=0)
            with pytest.raises(ValueError, match="bound to another index"):
                arc._live().append_index(twin._live(), [REF[10:60]])
            with rlz.RlzArchive.build(REF, TARGETS) as host, pytest.raises(ValueError, match="opened by nolzss_rlz_archive_open_index"):
                host._live().append_index(ix._live(), [REF[10:60]])
            assert delta(native, before) == (0, 0)
        with arc.finder(max_pattern_length=12) as old:
            held = native.debug_device_buffers()
            arc.append([REF[300:380]])
            assert native.debug_device_buffers()[0] == held[0]
            with nothing_kept(native):
                with pytest.raises(ValueError, match="grown since the finder was opened"):
                    old.count([REF[50:60]])
        assert native.debug_device_buffers()[0] == held[0] - 3
        assert arc.extract([(3, 0, 80)]) == [REF[300:380]]


def test_an_index_closed_before_what_was_opened_over_it(native, rlz):
    with nothing_kept(native) as before:
        ix = rlz.RlzIndex.build([REF])
        pile, co, arc = ix.pileup(normalize_indels=True), ix.cohort(), rlz.RlzArchive.from_index(ix)
        pile.add(READS)
        co.add(pile)
        co.add_calls(CALLS[0])
        arc.append(TARGETS)
        finder = arc.finder(max_pattern_length=8)
        assert delta(native, before)[0] == 1 + 2 + 1 + 3 + 3
        ix.close()
        assert delta(native, before)[0] == 2 + 1 + 3 + 3
        with pytest.raises(ValueError, match="the index is closed"):
            pile.info
        for handle in (pile, co, finder, arc):
            handle.close()
