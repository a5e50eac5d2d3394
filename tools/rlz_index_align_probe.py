#!/usr/bin/env python3
"""Relative-LZ index: base-level alignments of reads and contigs, measured beside the seed_chains call they start from.

    python tools/rlz_index_align_probe.py [--lg 24] [--lgreads 18] [--lgcontigs 12] [--reps 5]
                                          [--out profiles/r15_rlz_index_align.txt]

Input: the reference and the two target sets of tools/rlz_index_seed_chains_probe.py -- 2^lg random bases, reverse
complement on; 2^lgreads reads of 150 bases at 1 % substitutions, 2^lgcontigs contigs of 10 000 bases at 0.1 %.
Measured per set on arguments that are marshalled once, alternating, medians of `reps` after a warm-up of both:
  - align: the C ABI call nolzss_rlz_index_align (min_length 20, max_hits 64, bandwidth 31, band 16, max_flank 256, the
    other parameters at the defaults of RlzIndex.align), its result freed;
  - seed_chains: nolzss_rlz_index_seed_chains with the same first five parameters, its result freed -- the floor of the
    route a user takes without align: a dynamic programme between the anchors on the host comes on top of it.
Then the bytes either call brings down, the stage table (nolzss_profile_report) of one align call with the device time
of every align stage and the DP rows per second of the recurrence kernel, and a sample of 48 primary alignments whose
ops are replayed against the reference (tests/rlz_align_model.replay).  Runs on the GPU machine only.  No counter run is
made.
"""
import argparse
import ctypes as C
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
sys.path.insert(0, str(ROOT / "tools"))

import numpy as np  # noqa: E402

import gen  # noqa: E402
import rlz_align_model as am  # noqa: E402
from nolzss_amd import _lib  # noqa: E402
from nolzss_amd import _noLZSS as native  # noqa: E402
from rlz_index_seeds_probe import cuts  # noqa: E402
from rlz_probe import timed  # noqa: E402

ALIGN_STAGES = ("rlz_align_plan", "rlz_align_sizes", "rlz_align_offsets", "rlz_align_dp", "rlz_align_traceback",
                "rlz_align_heads", "rlz_align_ops", "rlz_align_records")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lg", type=int, default=24)
    ap.add_argument("--lgreads", type=int, default=18)
    ap.add_argument("--lgcontigs", type=int, default=12)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--min-length", type=int, default=20)
    ap.add_argument("--max-hits", type=int, default=64)
    ap.add_argument("--max-gap", type=int, default=5000)
    ap.add_argument("--bandwidth", type=int, default=31)
    ap.add_argument("--min-score", type=int, default=40)
    ap.add_argument("--band", type=int, default=16)
    ap.add_argument("--max-flank", type=int, default=256)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "r15_rlz_index_align.txt"))
    a = ap.parse_args()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    lib = _lib.lib
    native.set_device(0)
    ref_arr = gen.random_dna(1 << a.lg, 0x524C5A)
    ref = ref_arr.tobytes()
    say(f"relative-LZ index align probe: reference 2^{a.lg} bases, reverse complement on, min_length {a.min_length}, "
        f"max_hits {a.max_hits}, max_gap {a.max_gap}, bandwidth {a.bandwidth}, min_score {a.min_score}, band {a.band}, "
        f"max_flank {a.max_flank}")
    t_open, ix = timed(lambda: native.RlzIndexHandle.open(ref, with_rc=True))
    say(f"open: {t_open:.1f} ms, handle {ix.info['device_bytes'] / 2**20:.0f} MiB, P = {ix.info['prefix_syms']}")
    h = ix._handle()
    cparams = native._chain_params(a.min_length, a.max_hits, a.max_gap, a.bandwidth, a.min_score)
    aparams = native._align_params(a.min_length, a.max_hits, a.max_gap, a.bandwidth, a.min_score, a.band, a.max_flank)

    sets = (("reads", 1 << a.lgreads, 150, 0.01, 1), ("contigs", 1 << a.lgcontigs, 10_000, 0.001, 2))
    for label, k, length, rate, seed in sets:
        rows = cuts(ref_arr, k, length, rate, seed)
        targets = [row.tobytes() for row in rows]
        args = native._seq_args(targets, "target")  # marshalled once: both calls start from these arguments
        n = k * (length + 1)

        def align(keep=False):
            res = _lib.RlzAlignResult()
            try:
                _lib.check(lib.nolzss_rlz_index_align(h, *args, C.byref(aparams), C.byref(res)))
                counts = (res.num_alignments, res.num_ops, res.num_jobs, res.num_rows)
                if not keep:
                    return counts
                na, no = res.num_alignments, res.num_ops
                recs, ops = np.zeros(na, dtype=native.ALIGN_DTYPE), np.zeros(no, dtype=np.uint32)
                off = np.ctypeslib.as_array(C.cast(res.op_offsets, C.POINTER(C.c_uint64)), shape=(na + 1,)).copy()
                if na:
                    C.memmove(recs.ctypes.data, res.alignments, na * native.ALIGN_DTYPE.itemsize)
                if no:
                    C.memmove(ops.ctypes.data, res.ops, no * 4)
                return counts, recs, off, ops
            finally:
                lib.nolzss_free_rlz_align_result(C.byref(res))

        def chains():
            res = _lib.RlzSeedChainsResult()
            try:
                _lib.check(lib.nolzss_rlz_index_seed_chains(h, *args, C.byref(cparams), C.byref(res)))
                return res.num_chains, res.num_anchors
            finally:
                lib.nolzss_free_rlz_seed_chains_result(C.byref(res))

        say()
        say(f"---- {label}: {k} targets of {length} bases, substitution rate {rate} ({n} batch positions)")
        (na, no, nj, nr), recs, off, ops = align(keep=True)  # warm-up of both calls
        nc, nan = chains()
        assert nc == na, "one alignment per chain"
        prim = recs[recs["primary"] == 1]
        whole = int(((prim["t_start"] == 0) & (prim["t_end"] == length)).sum())
        say(f"chains {nc} with {nan} anchors; alignments {na}, jobs {nj}, DP rows {nr} ({nr / max(nj, 1):.2f} per job), ops {no} "
            f"({no / max(na, 1):.2f} per alignment)")
        say(f"primary alignments {len(prim)}: {whole} cover their target end to end, mean edit distance "
            f"{float(prim['edit_distance'].mean()) if len(prim) else 0:.2f}, mean columns {float(prim['columns'].mean()) if len(prim) else 0:.1f}")
        where = np.flatnonzero(recs["primary"] == 1)
        sample = where[np.unique(np.linspace(0, len(where) - 1, 48).astype(np.int64))] if len(where) else []
        for j in sample:
            r = recs[j]
            t = targets[int(r["target"])]
            rebuilt, cost = am.replay(ops[int(off[j]):int(off[j + 1])], t, ref, int(r["t_start"]), int(r["t_end"]),
                                      int(r["r_start"]), int(r["r_end"]), bool(r["is_rc"]))
            assert rebuilt == t[int(r["t_start"]):int(r["t_end"])] and cost == int(r["edit_distance"]), j
        say(f"a sample of {len(sample)} primary alignments: each replays to its stretch of the target at its edit distance")
        down_align = 80 * na + 8 * (na + 1) + 4 * no
        down_chains = 64 * nc + 8 * (nc + 1) + 24 * nan
        say(f"bytes down: align {down_align / 1e6:.2f} MB (records, offsets, ops), seed_chains {down_chains / 1e6:.2f} MB "
            f"(chains, offsets, anchors): {down_align / max(down_chains, 1):.3f} of it")
        t_align, t_chains = [], []
        for _ in range(a.reps):
            t_align.append(timed(align)[0])
            t_chains.append(timed(chains)[0])
        med_a, med_c = statistics.median(t_align), statistics.median(t_chains)
        say(f"align        median {med_a:9.1f} ms   {['%.1f' % t for t in t_align]}   {n / med_a / 1e3:.1f} M positions/s")
        say(f"seed_chains  median {med_c:9.1f} ms   {['%.1f' % t for t in t_chains]}")
        say(f"ratio: align takes {med_a / med_c:.3f} of the seed_chains call a user would align on the host")

        native.profile_enable(True)
        try:
            native.profile_reset()
            t, _ = timed(align)
            rep = native.profile_report()
        finally:
            native.profile_enable(False)
            native.profile_reset()
        say(f"stage table of one align call (wall {t:.1f} ms with the profiler on; nested scopes are listed too)")
        say(f"  {'stage':24s} {'launches':>8s} {'ms':>9s} {'GB/s':>8s}")
        for name, (launches, ms_, nbytes) in sorted(rep.items(), key=lambda kv: -kv[1][1]):
            gbs = f"{nbytes / (ms_ * 1e-3) / 1e9:8.0f}" if nbytes and ms_ else " " * 8
            say(f"  {name:24s} {launches:8d} {ms_:9.3f} {gbs}")
        stages = sum(rep[s][1] for s in ALIGN_STAGES if s in rep)
        span = rep.get("rlz_index_align", (0, 0.0, 0))[1]
        dp = rep.get("rlz_align_dp", (0, 0.0, 0))[1]
        say(f"the align stages together {stages:.3f} ms: {stages / max(span, 1e-9):.3f} of the call's device span ({span:.3f} ms); "
            f"the recurrence kernel {dp:.3f} ms for {nr} rows and {nj} jobs: {nr / max(dp, 1e-9) / 1e3:.1f} M DP rows/s")
    ix.close()
    say()
    say("no counter run was made")
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
