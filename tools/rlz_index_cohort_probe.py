#!/usr/bin/env python3
"""Relative-LZ index: what a cohort costs -- an add beside the consensus of the parent commit's library, distances()
beside the route a user takes without it, and the pair kernel's rate.

    python tools/rlz_index_cohort_probe.py [--parent nolzss_amd/libnolzss_hip.parent.so] [--lg 22] [--lgreads 16]
                                           [--samples 64,256,600] [--reps 5] [--host-seconds 50] [--sweep]
                                           [--out profiles/r18_rlz_index_cohort.txt]

One process, one device, medians of --reps after a warm-up of every arm.
  (a) one pileup of 2^lgreads reads of 150 bases over a reference of 2^lg bases (the parameters of
      tools/rlz_index_consensus_probe.py), in this library and, with the same reads, in the parent's: the wall time and
      the device span (profiler scopes) of RlzCohort.add of it, and of nolzss_rlz_pileup_consensus of the parent's
      library on its own pileup; the bytes either brings down.
  (b) per N of --samples: N samples made with add_calls from the reference mutated at 0.1 %, then distances(): wall time,
      the device span of the pair kernels and of the download.  The route without a cohort: one consensus download per
      sample (its time is that of (a)) and an all-pairs comparison of the byte strings in numpy, timed at the largest N
      of 16, 32, 64 ... whose predicted time stays below --host-seconds (predicted from 120 pairs); nothing is scaled here.
  (c) the pair kernel's word-pairs per second from (b): those of the tiles it computes and those a user asked for.
Runs on the GPU machine only.  --parent missing: the parent's columns are left out and the file says so.  No counter run.
"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
sys.path.insert(0, str(ROOT / "tools"))

import numpy as np  # noqa: E402

import gen  # noqa: E402
from nolzss_amd import _lib  # noqa: E402
from nolzss_amd import _noLZSS as native  # noqa: E402
from rlz_index_seeds_probe import cuts  # noqa: E402
from rlz_probe import mutated, timed  # noqa: E402

TILE, CHUNK, MAX_SLICE = 64, 8, 4096  # kCohortTile, kChunk, kCohortMaxSlice (rlz_cohort.hip)


class Parent:
    """the few entry points of another build of the library that the comparison needs, through ctypes"""

    def __init__(self, path):
        vp, sz = C.c_void_p, C.c_size_t
        seqs = [C.POINTER(C.c_char_p), C.POINTER(sz), sz]
        self.lib = lib = C.CDLL(str(path))
        lib.nolzss_rlz_index_open.argtypes = seqs + [C.c_int, C.c_uint32, C.c_int, C.POINTER(vp)]
        lib.nolzss_rlz_index_close.argtypes = [vp]
        lib.nolzss_rlz_pileup_open_flags.argtypes = [vp, C.POINTER(_lib.RlzAlignParams), C.c_uint32, C.POINTER(vp)]
        lib.nolzss_rlz_pileup_add.argtypes = [vp] + seqs + [C.c_int, C.POINTER(_lib.RlzPileupAddInfo)]
        lib.nolzss_rlz_pileup_consensus.argtypes = [vp, C.POINTER(_lib.RlzConsensusParams), C.c_int, C.POINTER(_lib.RlzConsensusResult)]
        lib.nolzss_free_rlz_consensus_result.argtypes = [C.POINTER(_lib.RlzConsensusResult)]
        lib.nolzss_free_rlz_consensus_result.restype = None
        lib.nolzss_rlz_pileup_close.argtypes = [vp]
        lib.nolzss_profile_enable.argtypes = [C.c_int, C.c_int]
        lib.nolzss_profile_reset.argtypes = [C.c_int]
        lib.nolzss_profile_report.argtypes = [C.c_int, C.c_char_p, sz]
        lib.nolzss_last_error.restype = C.c_char_p

    def check(self, rc):
        if rc:
            raise RuntimeError(f"parent library: status {rc}: {self.lib.nolzss_last_error().decode(errors='replace')}")

    def report(self):
        buf = C.create_string_buffer(1 << 16)
        self.check(self.lib.nolzss_profile_report(0, buf, len(buf)))
        return {name: (int(count), float(ms), float(nbytes))
                for name, count, ms, nbytes in (line.split() for line in buf.value.decode().splitlines())}


def profiled(fn, enable, reset, report):
    enable(True)
    try:
        reset()
        t, out = timed(fn)
        return t, out, report()
    finally:
        enable(False)
        reset()


LAUNCH_BLOCKS, MIN_SLICE = 2048, 64  # kLaunchBlocks, kMinSlice (rlz_cohort.hip)


def default_slice(row_tiles, words):
    """rlz_cohort_default_slice (rlz_cohort.hip), restated for the report: the slice of a launch over a row of tiles"""
    want = -(-LAUNCH_BLOCKS // row_tiles)
    return min(max(-(-(-(-words // want)) // CHUNK) * CHUNK, MIN_SLICE), MAX_SLICE)


def host_pairs(samples, pairs):
    """the comparison a user runs today over consensus strings, for the first `pairs` pairs: where both are called (not
    N), and where they differ there -> (seconds, differences summed)"""
    done, t0, total = 0, time.perf_counter(), 0
    for i in range(len(samples)):
        ok_i = samples[i] != ord("N")
        for j in range(i + 1, len(samples)):
            if done == pairs:
                return (time.perf_counter() - t0), total
            both = ok_i & (samples[j] != ord("N"))
            compared = int(np.count_nonzero(both))
            total += int(np.count_nonzero((samples[i] != samples[j]) & both)) if compared else 0
            done += 1
    return (time.perf_counter() - t0), total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=str(ROOT / "nolzss_amd" / "libnolzss_hip.parent.so"))
    ap.add_argument("--lg", type=int, default=22)
    ap.add_argument("--lgreads", type=int, default=16)
    ap.add_argument("--samples", default="64,256,600")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-seconds", type=float, default=50.0)
    ap.add_argument("--sweep", action="store_true", help="distances() under every slice length of the knob as well")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "r18_rlz_index_cohort.txt"))
    a = ap.parse_args()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    def flush():
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text("\n".join(lines) + "\n")

    lib = _lib.lib
    native.set_device(0)
    values = (20, 64, 5000, 31, 40, 16, 256)
    aparams = native._align_params(*values)
    ref_arr = gen.random_dna(1 << a.lg, 0x524C5A)
    ref = ref_arr.tobytes()
    B = len(ref)
    words = -(-B // 64)
    say(f"relative-LZ index cohort probe: reference 2^{a.lg} bases ({words} words per plane, {24 * words / 1e6:.2f} MB per sample), "
        f"reverse complement on; medians of {a.reps} after a warm-up")
    ix = native.RlzIndexHandle.open(ref, with_rc=True)
    parent = Parent(a.parent) if Path(a.parent).exists() else None
    p_ix = C.c_void_p()
    if parent:
        parent.check(parent.lib.nolzss_rlz_index_open(*native._seq_args([ref], "reference"), 1, 0, 0, C.byref(p_ix)))
        say(f"parent library: {Path(a.parent).name}, its own index and pileup handles on the same device")
    else:
        say(f"parent library {a.parent} not found: no comparison with the parent commit in this run")

    # ---- (a) an add beside a consensus ------------------------------------------------------------------------------
    k = 1 << a.lgreads
    reads = [row.tobytes() for row in cuts(ref_arr, k, 150, 0.01, 1)]
    args = native._seq_args(reads, "target")
    pile = native.RlzPileupHandle.open(ix, *values, normalize_indels=True)
    pile.add(reads)
    say()
    say(f"---- (a) one pileup of {k} reads of 150 bases, substitution rate 0.01, normalised; rule min_depth 1, 1/2")
    co = native.RlzCohortHandle.open(ix)
    first = co.add_pileup(pile, 1, (1, 2))  # warm-up (and the first allocation)
    say(f"the sample: called {first['called']}, low {first['low']}, deleted {first['deleted']}, differs {first['differs']}; "
        f"capacity {co.info['capacity']} samples, {co.info['device_bytes'] / 1e6:.1f} MB")
    walls, spans, packs = [], [], []
    for _ in range(a.reps):
        t, _, rep = profiled(lambda: co.add_pileup(pile, 1, (1, 2)), native.profile_enable, native.profile_reset, native.profile_report)
        walls.append(t)
        spans.append(rep.get("rlz_cohort_add_pileup", (0, 0.0, 0))[1])
        packs.append(rep.get("rlz_cohort_pack_counts", (0, 0.0, 0))[1])
    say(f"cohort add: wall median {statistics.median(walls):.3f} ms {['%.3f' % t for t in walls]}; device span of the call "
        f"{statistics.median(spans):.3f} ms, of rlz_cohort_pack_counts {statistics.median(packs):.3f} ms; 40 bytes of info down")
    t_cons = []
    for _ in range(a.reps + 1):
        t, cons, rep = profiled(lambda: pile.consensus(1, (1, 2), "reference", False), native.profile_enable, native.profile_reset,
                                native.profile_report)
        t_cons.append((t, rep.get("rlz_pileup_consensus_call", (0, 0.0, 0))[1]))
    t_cons = t_cons[1:]
    text_bytes = sum(len(r) for r in cons["records"])
    say(f"this library's consensus() of the same pileup: wall median {statistics.median(t for t, _ in t_cons):.3f} ms, device span of "
        f"the call {statistics.median(s for _, s in t_cons):.3f} ms; {text_bytes / 1e6:.2f} MB of text down")
    assert (first["called"], first["low"], first["deleted"], first["differs"]) == (
        cons["called"] - cons["deleted"], cons["low_positions"], cons["deleted"], cons["substitutions"])
    say("the four identities between the add's counts and that consensus hold")
    if parent:
        p_pile = C.c_void_p()
        parent.check(parent.lib.nolzss_rlz_pileup_open_flags(p_ix, C.byref(aparams), 1, C.byref(p_pile)))
        info = _lib.RlzPileupAddInfo()
        parent.check(parent.lib.nolzss_rlz_pileup_add(p_pile, *args, 1, C.byref(info)))
        params = _lib.RlzConsensusParams(1, 0, 1, 2)

        def parent_consensus():
            res = _lib.RlzConsensusResult()
            try:
                parent.check(parent.lib.nolzss_rlz_pileup_consensus(p_pile, C.byref(params), 0, C.byref(res)))
                return int(res.length)
            finally:
                parent.lib.nolzss_free_rlz_consensus_result(C.byref(res))

        rows = []
        for _ in range(a.reps + 1):
            t, length, rep = profiled(parent_consensus, lambda on: parent.check(parent.lib.nolzss_profile_enable(0, 1 if on else 0)),
                                      lambda: parent.check(parent.lib.nolzss_profile_reset(0)), parent.report)
            rows.append((t, rep.get("rlz_pileup_consensus_call", (0, 0.0, 0))[1], rep.get("rlz_consensus", (0, 0.0, 0))[1] +
                         rep.get("rlz_consensus_text", (0, 0.0, 0))[1]))
        rows = rows[1:]
        say(f"parent's consensus() of its own pileup of the same reads: wall median {statistics.median(r[0] for r in rows):.3f} ms "
            f"{['%.3f' % r[0] for r in rows]}; device span of the call {statistics.median(r[1] for r in rows):.3f} ms, of its kernels "
            f"(rlz_consensus + rlz_consensus_text) {statistics.median(r[2] for r in rows):.3f} ms; {length / 1e6:.2f} MB of text down")
        parent.check(parent.lib.nolzss_rlz_pileup_close(p_pile))
    co.close()
    pile.close()
    flush()

    # ---- (b), (c) distances -----------------------------------------------------------------------------------------
    sizes = [int(v) for v in a.samples.split(",")]
    samples = [mutated(ref_arr, 9000 + j) for j in range(max(sizes))]  # 0.1 % of the positions redrawn
    say()
    say(f"---- (b) distances(): samples are the reference with 0.1 % of its positions redrawn, added with add_calls")
    for n in sizes:
        co = native.RlzCohortHandle.open(ix)
        t_add = []
        for s in samples[:n]:
            t_add.append(timed(lambda: co.add_calls(s))[0])
        co.distances()  # warm-up
        walls, pair_ms, down_ms = [], [], []
        for _ in range(a.reps):
            t, (diff, comp), rep = profiled(co.distances, native.profile_enable, native.profile_reset, native.profile_report)
            walls.append(t)
            pair_ms.append(rep.get("rlz_cohort_pairs", (0, 0.0, 0))[1])
            down_ms.append(rep.get("cohort_distances_d2h", (0, 0.0, 0))[1])
        nt = -(-n // TILE)
        tiles = nt * (nt + 1) // 2
        rows = [(nt - ti, default_slice(nt - ti, words)) for ti in range(nt)]
        blocks = sum(t * -(-words // sl) for t, sl in rows)
        computed, asked = tiles * TILE * TILE * words, n * (n - 1) // 2 * words
        pm = statistics.median(pair_ms)
        say(f"N {n:4d}: add_calls median {statistics.median(t_add):.3f} ms each ({co.info['device_bytes'] / 1e6:.0f} MB of planes); "
            f"distances() wall median {statistics.median(walls):.3f} ms {['%.3f' % t for t in walls]}; device span of rlz_cohort_pairs "
            f"{pm:.3f} ms, of the download {statistics.median(down_ms):.3f} ms ({8 * n * n / 1e6:.2f} MB down)")
        say(f"        (c) {tiles} tiles in {nt} launches and the mirror, slices of {rows[0][1]} (first row) .. {rows[-1][1]} (last row) words, "
            f"{blocks} workgroups; {computed:.3e} word-pairs computed = {computed / (pm * 1e-3):.3e} per second of that span; "
            f"{asked:.3e} asked for (i < j) = {asked / (pm * 1e-3):.3e} per second")
        if a.sweep:
            cells = []
            for knob in (16, 32, 64, 128, 256, 512, 1024, 2048, 4096):
                os.environ["NOLZSS_RLZ_COHORT_SLICE"] = str(knob)  # read on every call: one slice length for every row
                co.distances()
                spans = []
                for _ in range(3):
                    _, (d2, c2), rep = profiled(co.distances, native.profile_enable, native.profile_reset, native.profile_report)
                    spans.append(rep.get("rlz_cohort_pairs", (0, 0.0, 0))[1])
                assert np.array_equal(d2, diff) and np.array_equal(c2, comp)
                cells.append(f"{knob}: {statistics.median(spans):.3f}")
            del os.environ["NOLZSS_RLZ_COHORT_SLICE"]
            say(f"        one slice length for every row (NOLZSS_RLZ_COHORT_SLICE), device span of rlz_cohort_pairs in ms, medians of 3: "
                + ", ".join(cells))
        assert int(diff[0, 0]) == 0 and int(comp[0, 0]) == B
        if n == sizes[0]:
            check = int(np.count_nonzero(samples[0] != samples[1]))
            assert int(diff[0, 1]) == check, (int(diff[0, 1]), check)
            say(f"        differences[0][1] = {check}, as numpy counts it")
        co.close()
        flush()
    say()
    say("---- (b) the route without a cohort: N consensus downloads (each as in (a)) and all pairs in numpy over byte strings")
    per_pair = host_pairs(samples[:16], 120)[0] / 120
    say(f"numpy: {per_pair * 1e3:.2f} ms per pair of {B} bytes (120 pairs of 16 samples)")
    n_host = 16
    while n_host * 2 <= max(sizes) and (2 * n_host) * (2 * n_host - 1) / 2 * per_pair <= a.host_seconds:
        n_host *= 2
    t_host, _ = host_pairs(samples[:n_host], n_host * (n_host - 1) // 2)
    say(f"numpy, all {n_host * (n_host - 1) // 2} pairs of N = {n_host} (the largest N predicted below {a.host_seconds:.0f} s): {t_host:.2f} s")
    if parent:
        parent.check(parent.lib.nolzss_rlz_index_close(p_ix))
    ix.close()
    say()
    say("no counter run was made")
    flush()


if __name__ == "__main__":
    main()
