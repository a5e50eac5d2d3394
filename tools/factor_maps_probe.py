#!/usr/bin/env python3
"""Times the strand-bias grid and the space-scale histogram binned on the device (nolzss_factor_maps_text) on one GPU.

    python tools/factor_maps_probe.py [--reps 3] [--out profiles/factor_maps.txt] [--rc-log2n 28] [--plain-log2n 30]

For bench.py's two texts (tests/gen.py repeat_dna: 2^28 bases, seed 0x5EED0005, reverse-complement mode; 2^30 bases,
seed 0x5EED0003, plain mode), medians over --reps after one warm-up:
  (a) factor_maps from the host buffer: grid 50 x 50 and the space-scale request (base-2 ladder, the reference's
      position ladder) together, one pipeline run;
  (b) what a host-side binning needs first: factorize_dna_w_rc / factorize from the same host buffer to host records;
  (c) the same pipeline stopping at records in HBM (emit = 1) on a text already resident in device memory: the text
      upload is NOT inside this clock (it is inside (a) and (b));
  (d) the new kernels' own time from the stage profiler and their record bytes per second (24 bytes per factor read)
      beside the device-to-device copy rate of BENCH_r04.json (peak_measured).
"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import gen  # noqa: E402
from nolzss_amd import _noLZSS as native  # noqa: E402

LADDER = 2.0 ** np.linspace(0, 33, 133)


def timed(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), min(ts), max(ts)


def stages(fn):
    native.profile_enable(True)
    native.profile_reset()
    fn()
    rep = native.profile_report()
    native.profile_enable(False)
    return rep


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rc-log2n", type=int, default=28)
    ap.add_argument("--plain-log2n", type=int, default=30)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    peak = None
    try:
        bench = json.loads((ROOT / "BENCH_r04.json").read_text())
        peak = next(v["peak_measured"] for v in _walk(bench) if isinstance(v, dict) and "peak_measured" in v)
    except (OSError, StopIteration, ValueError):
        pass
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    for mode, lg, seed in (("rc", args.rc_log2n, 0x5EED0005), ("plain", args.plain_log2n, 0x5EED0003)):
        with_rc = mode == "rc"
        text = gen.repeat_dna(1 << lg, seed=seed)
        maps = lambda: native.factor_maps(text, with_rc=with_rc, grid=(50, 50), length_edges=LADDER)  # noqa: E731
        a = timed(maps, args.reps)
        b = timed(lambda: (native.factorize_dna_w_rc_array if with_rc else native.factorize_array)(text), args.reps)
        dev = torch.from_numpy(text).cuda()
        torch.cuda.synchronize()
        to_hbm = native.factorize_dna_w_rc_device if with_rc else native.factorize_device
        c = timed(lambda: to_hbm(dev.data_ptr(), dev.numel(), emit=1), args.reps)
        del dev
        m = maps()
        say(f"n=2^{lg} {mode}: z={m['z']} (forward {m['kept_forward']}, rc {m['kept_rc']})")
        say(f"  (a) factor_maps, host text -> grid 50x50 + space-scale histogram: {a[0]:.1f} ms ({a[1]:.1f}-{a[2]:.1f})")
        say(f"  (b) factorize, host text -> host records:                         {b[0]:.1f} ms ({b[1]:.1f}-{b[2]:.1f})")
        say(f"  (c) pipeline to records in HBM, text resident (no upload):        {c[0]:.1f} ms ({c[1]:.1f}-{c[2]:.1f})")
        say(f"  (a) <= (b): {'yes' if a[0] <= b[0] else 'NO'};  (a) - (c) = {a[0] - c[0]:.1f} ms = {100 * (a[0] - c[0]) / c[0]:.0f}% of (c)")
        rep = stages(maps)
        gb = 24.0 * m["z"] / 1e9
        for k in ("text_h2d", "factor_maps", "map_stats", "strand_grid", "length_position_hist"):
            if k in rep:
                ms = rep[k][1]
                rate = f", {gb / (ms / 1e3):.0f} GB/s of records" if k in ("map_stats", "strand_grid",
                                                                           "length_position_hist") and ms > 0 else ""
                say(f"  (d) {k}: {ms:.3f} ms{rate}")
        if peak:
            say(f"      device-to-device copy rate of BENCH_r04.json (peak_measured): {peak:.0f} GB/s")
        for forced in ("1",):
            import os
            os.environ["NOLZSS_FACTOR_MAPS_GLOBAL"] = forced
            rep = stages(maps)
            os.environ.pop("NOLZSS_FACTOR_MAPS_GLOBAL")
            say("      global-atomic form forced: " + ", ".join(
                f"{k} {rep[k][1]:.3f} ms" for k in ("strand_grid", "length_position_hist") if k in rep))
    if args.out:
        Path(args.out).write_text("\n".join(lines) + "\n")


def _walk(o):
    if isinstance(o, dict):
        yield o
        for v in o.values():
            yield from _walk(v)
    elif isinstance(o, list):
        for v in o:
            yield from _walk(v)


if __name__ == "__main__":
    sys.exit(main())
