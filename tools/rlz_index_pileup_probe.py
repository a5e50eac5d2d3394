#!/usr/bin/env python3
"""Relative-LZ index: pileup counts of reads and contigs, measured beside the align call whose results a user would
otherwise pile up on the host.

    python tools/rlz_index_pileup_probe.py [--lg 24] [--lgreads 18] [--lgcontigs 12] [--reps 5]
                                           [--out profiles/r16_rlz_index_pileup.txt]

The reference and the two target sets are those of tools/rlz_index_align_probe.py, at the same parameters.  Per set, on
arguments marshalled once and with both calls alternating in one process, medians of --reps after a warm-up:
  - add: the C ABI call nolzss_rlz_pileup_add (primary_only) into one pileup that stays open;
  - align: the C ABI call nolzss_rlz_index_align, its result freed -- the floor of what a user pays today before a
    host-side pileup of the CIGARs.
Then the bytes either call brings down, one counts() of the whole block and one variants(2, 1, 2) with their times and
bytes, the stage table (nolzss_profile_report) of one add and of the two reads behind it with the device time of every
added stage and its share of the call's span, and the counters of a stretch of the block checked against
tests/rlz_pileup_model over the alignments align returns.  Runs on the GPU machine only.  No counter run is made.
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
import rlz_pileup_model as pm  # noqa: E402
from nolzss_amd import _lib  # noqa: E402
from nolzss_amd import _noLZSS as native  # noqa: E402
from rlz_index_seeds_probe import cuts  # noqa: E402
from rlz_probe import timed  # noqa: E402

ADD_STAGES = ("rlz_pileup_scans", "rlz_pileup_accumulate")
READ_STAGES = ("rlz_pileup_resolve", "rlz_pileup_counts", "rlz_pileup_variants", "rlz_pileup_variant_records")


def profiled(fn):
    native.profile_enable(True)
    try:
        native.profile_reset()
        t, out = timed(fn)
        return t, out, native.profile_report()
    finally:
        native.profile_enable(False)
        native.profile_reset()


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
    ap.add_argument("--out", default=str(ROOT / "profiles" / "r16_rlz_index_pileup.txt"))
    a = ap.parse_args()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    lib = _lib.lib
    native.set_device(0)
    ref_arr = gen.random_dna(1 << a.lg, 0x524C5A)
    ref = ref_arr.tobytes()
    B = len(ref)
    say(f"relative-LZ index pileup probe: reference 2^{a.lg} bases, reverse complement on, min_length {a.min_length}, "
        f"max_hits {a.max_hits}, max_gap {a.max_gap}, bandwidth {a.bandwidth}, min_score {a.min_score}, band {a.band}, "
        f"max_flank {a.max_flank}, primary_only")
    t_open, ix = timed(lambda: native.RlzIndexHandle.open(ref, with_rc=True))
    say(f"open: {t_open:.1f} ms, handle {ix.info['device_bytes'] / 2**20:.0f} MiB, P = {ix.info['prefix_syms']}")
    h = ix._handle()
    values = (a.min_length, a.max_hits, a.max_gap, a.bandwidth, a.min_score, a.band, a.max_flank)
    aparams = native._align_params(*values)

    sets = (("reads", 1 << a.lgreads, 150, 0.01, 1), ("contigs", 1 << a.lgcontigs, 10_000, 0.001, 2))
    for label, k, length, rate, seed in sets:
        rows = cuts(ref_arr, k, length, rate, seed)
        targets = [row.tobytes() for row in rows]
        args = native._seq_args(targets, "target")  # marshalled once: both calls start from these arguments
        n = k * (length + 1)
        t_popen, pile = timed(lambda: native.RlzPileupHandle.open(ix, *values))
        p = pile._handle()

        def add():
            info = _lib.RlzPileupAddInfo()
            _lib.check(lib.nolzss_rlz_pileup_add(p, *args, 1, C.byref(info)))
            return info.alignments, info.ops, info.columns, info.targets

        def align(keep=False):
            res = _lib.RlzAlignResult()
            try:
                _lib.check(lib.nolzss_rlz_index_align(h, *args, C.byref(aparams), C.byref(res)))
                na, no = res.num_alignments, res.num_ops
                if not keep:
                    return na, no
                recs, ops = np.zeros(na, dtype=native.ALIGN_DTYPE), np.zeros(no, dtype=np.uint32)
                off = np.ctypeslib.as_array(C.cast(res.op_offsets, C.POINTER(C.c_uint64)), shape=(na + 1,)).copy()
                if na:
                    C.memmove(recs.ctypes.data, res.alignments, na * native.ALIGN_DTYPE.itemsize)
                if no:
                    C.memmove(ops.ctypes.data, res.ops, no * 4)
                return recs, off, ops
            finally:
                lib.nolzss_free_rlz_align_result(C.byref(res))

        say()
        say(f"---- {label}: {k} targets of {length} bases, substitution rate {rate} ({n} batch positions)")
        say(f"pileup open: {t_popen:.1f} ms, {pile.info['device_bytes'] / 2**20:.0f} MiB of counters "
            f"({pile.info['device_bytes'] / B:.1f} bytes per block base)")
        kept, kops, kcols, _ = add()  # warm-up of both calls
        recs, off, ops = align(keep=True)
        na, no = len(recs), len(ops)
        prim = recs["primary"] == 1
        assert kept == int(prim.sum()) and kops == int(recs["num_ops"][prim].sum()) and kcols == int(recs["columns"][prim].sum())
        say(f"alignments {na} with {no} ops; kept (primary) {kept} with {kops} ops and {kcols} columns: "
            f"{kcols / max(kops, 1):.1f} columns per op")
        # a stretch of the block against the model over what align returned (the first add only: the table is still 1 x)
        lo, hi = B // 2, B // 2 + 4096
        counts = pile.counts(lo, hi)
        near = np.flatnonzero(prim & (recs["r_end"] > lo) & (recs["r_start"] < hi))
        alns = [{key: int(recs[key][c]) for key in ("target", "t_start", "t_end", "r_start", "r_end", "is_rc", "primary")}
                for c in near]
        sub_ops, sub_off = [], [0]
        for c in near:
            sub_ops += ops[int(off[c]):int(off[c + 1])].tolist()
            sub_off.append(len(sub_ops))
        first = min([al["r_start"] for al in alns] + [lo])
        last = max([al["r_end"] for al in alns] + [hi])
        for al in alns:
            al["r_start"] -= first
            al["r_end"] -= first
        exp = pm.pileup(last - first, alns, sub_ops, sub_off, targets, ref[first:last], True)[lo - first:hi - first]
        assert np.array_equal(counts, exp), "the counters of the stretch differ from the model"
        say(f"block positions [{lo}, {hi}): the counters equal the model over the {len(near)} primary alignments align "
            f"returned there (mean depth {float(counts[:, :5].sum(axis=1).mean()):.2f})")
        down_align = 80 * na + 8 * (na + 1) + 4 * no
        say(f"bytes down per batch: add 24 (three totals), align {down_align / 1e6:.2f} MB (records, offsets, ops)")
        t_add, t_align = [], []
        for _ in range(a.reps):
            t_add.append(timed(add)[0])
            t_align.append(timed(align)[0])
        med_p, med_a = statistics.median(t_add), statistics.median(t_align)
        say(f"add          median {med_p:9.1f} ms   {['%.1f' % t for t in t_add]}   {n / med_p / 1e3:.1f} M positions/s")
        say(f"align        median {med_a:9.1f} ms   {['%.1f' % t for t in t_align]}")
        say(f"ratio: add takes {med_p / med_a:.3f} of the align call a user would pile up on the host")

        t_counts, table = timed(lambda: pile.counts())  # (the first read after the adds: it resolves)
        t_again, _ = timed(lambda: pile.counts())
        t_var, found = timed(lambda: pile.variants(2, (1, 2)))
        depth = table[:, :5].sum(axis=1, dtype=np.uint64)
        say(f"counts() of the whole block: {t_counts:.1f} ms with the resolve, {t_again:.1f} ms without, {table.nbytes / 1e6:.1f} MB down; "
            f"mean depth {float(depth.mean()):.2f} after {pile.info['adds']} adds, REV share "
            f"{float(table[:, pm.REV].sum()) / max(float(depth.sum()), 1):.3f}")
        say(f"variants(2, 1, 2): {t_var:.1f} ms, {len(found)} records, {found.nbytes / 1e6:.3f} MB down")

        t, _, rep = profiled(add)
        say(f"stage table of one add (wall {t:.1f} ms with the profiler on; nested scopes are listed too)")
        say(f"  {'stage':28s} {'launches':>8s} {'ms':>9s} {'GB/s':>8s}")
        for name, (launches, ms_, nbytes) in sorted(rep.items(), key=lambda kv: -kv[1][1]):
            gbs = f"{nbytes / (ms_ * 1e-3) / 1e9:8.0f}" if nbytes and ms_ else " " * 8
            say(f"  {name:28s} {launches:8d} {ms_:9.3f} {gbs}")
        span = rep.get("rlz_pileup_add", (0, 0.0, 0))[1]
        for name in ADD_STAGES:
            ms_ = rep.get(name, (0, 0.0, 0))[1]
            say(f"added stage {name:24s} {ms_:9.3f} ms: {ms_ / max(span, 1e-9):.4f} of the add's device span ({span:.3f} ms)")
        _, _, rep_c = profiled(lambda: pile.counts())
        _, _, rep_v = profiled(lambda: pile.variants(2, (1, 2)))
        for rep_r, scope in ((rep_c, "rlz_pileup_counts_call"), (rep_v, "rlz_pileup_variants_call")):
            span_r = rep_r.get(scope, (0, 0.0, 0))[1]
            for name in READ_STAGES:
                if name in rep_r:
                    ms_ = rep_r[name][1]
                    say(f"read stage  {name:24s} {ms_:9.3f} ms: {ms_ / max(span_r, 1e-9):.4f} of {scope} ({span_r:.3f} ms)")
        pile.close()
    ix.close()
    say()
    say("no counter run was made")
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
