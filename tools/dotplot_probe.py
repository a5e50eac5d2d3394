#!/usr/bin/env python3
"""Times the self dot plot (nolzss_dotplot_*) on one GPU.

    python tools/dotplot_probe.py [--reps 5] [--out profiles/dotplot.txt] [--rc-log2n 28] [--plain-log2n 30]

For bench.py's two texts (tests/gen.py repeat_dna: 2^28 bases, seed 0x5EED0005, reverse-complement mode; 2^30 bases,
seed 0x5EED0003, plain mode), medians over --reps after one warm-up:
  (a) open: DotPlot.from_text from the host buffer (upload, pipeline, the records copied into the handle, statistics),
      beside factor_maps (grid 50 x 50) from the same buffer -- (a) of tools/factor_maps_probe.py;
  (b) render of the full view at 800 x 800, max planes only / with counts and 800 hover bins: wall clock of the call
      (zeroing, kernels, download of the rasters) and the rasteriser kernel alone from the stage profiler;
  (c) the same for a 1 % zoom (the middle hundredth of x, all of y);
  (d) (b) and (c) with NOLZSS_DOTPLOT_GLOBAL=1, every pixel straight to global memory;
  (e) map_stats over the same records -- the rate of merely streaming them -- and the ratio of the rasteriser to it.
"""
import argparse
import os
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import gen  # noqa: E402
from nolzss_amd import _noLZSS as native  # noqa: E402


def timed(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), min(ts), max(ts)


def stage_ms(fn, name, reps):
    """median of the stage profiler's time of `name` over reps calls, after one warm-up"""
    fn()
    ts = []
    for _ in range(reps):
        native.profile_enable(True)
        native.profile_reset()
        fn()
        rep = native.profile_report()
        native.profile_enable(False)
        ts.append(rep[name][1] if name in rep else float("nan"))
    return statistics.median(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rc-log2n", type=int, default=28)
    ap.add_argument("--plain-log2n", type=int, default=30)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    for mode, lg, seed in (("rc", args.rc_log2n, 0x5EED0005), ("plain", args.plain_log2n, 0x5EED0003)):
        if lg <= 0:
            continue
        with_rc = mode == "rc"
        text = gen.repeat_dna(1 << lg, seed=seed)
        opened = []

        def open_close():
            dp = native.DotPlot.from_text(text, with_rc=with_rc)
            opened[:] = [dp.info]
            dp.close()

        a = timed(open_close, max(1, min(args.reps, 3)))
        m = timed(lambda: native.factor_maps(text, with_rc=with_rc, grid=(50, 50)), max(1, min(args.reps, 3)))
        info = opened[0]
        say(f"n=2^{lg} {mode}: z={info['z']} (forward {info['kept_forward']}, rc {info['kept_rc']}), "
            f"x_max={info['x_max']}, y_max={info['y_max']}, lengths {info['min_length']}..{info['max_length']}")
        say(f"  (a) open, host text -> resident records: {a[0]:.1f} ms ({a[1]:.1f}-{a[2]:.1f});  factor_maps (grid 50x50) "
            f"from the same text: {m[0]:.1f} ms ({m[1]:.1f}-{m[2]:.1f})")
        with native.DotPlot.from_text(text, with_rc=with_rc) as dp:
            extent = max(info["x_max"], info["y_max"])
            mid, hundredth = extent // 2, max(800, extent // 100)
            views = [("full view", (0, extent), (0, extent)),
                     ("1 % zoom", (mid - hundredth // 2, mid - hundredth // 2 + hundredth), (0, extent))]
            for form in ("strip", "global"):
                if form == "global":
                    os.environ["NOLZSS_DOTPLOT_GLOBAL"] = "1"
                for name, xr, yr in views:
                    for what, kw in (("max planes", {}), ("counts + 800 hover bins", dict(counts=True, hover_bins=800))):
                        call = lambda: dp.render(xr, yr, width=800, height=800, **kw)  # noqa: E731
                        wall = timed(call, args.reps)
                        kern = stage_ms(call, "dotplot_raster", args.reps)
                        r = call()
                        say(f"  ({'b' if name == 'full view' else 'c'}{', d' if form == 'global' else ''}) {form:6s} {name:9s} "
                            f"800x800 {what:24s}: call {wall[0]:8.2f} ms ({wall[1]:.2f}-{wall[2]:.2f}), rasteriser "
                            f"{kern:8.3f} ms = {24.0 * info['z'] / 1e9 / (kern / 1e3):7.0f} GB/s of records; visible "
                            f"{r['visible_forward']} + {r['visible_rc']}, lit pixels {int((r['max_forward'] > 0).sum())} + "
                            f"{int((r['max_rc'] > 0).sum())}")
                os.environ.pop("NOLZSS_DOTPLOT_GLOBAL", None)

            # map_stats over all records: the open of the text source runs it once
            native.profile_enable(True)
            native.profile_reset()
            native.DotPlot.from_text(text, with_rc=with_rc).close()
            rep = native.profile_report()
            native.profile_enable(False)
            stats_ms = rep["map_stats"][1] if "map_stats" in rep else float("nan")
            full = stage_ms(lambda: dp.render((0, extent), (0, extent), width=800, height=800), "dotplot_raster", args.reps)
            say(f"  (e) map_stats over the same records: {stats_ms:.3f} ms = {24.0 * info['z'] / 1e9 / (stats_ms / 1e3):.0f} GB/s; "
                f"rasteriser of the full view (max planes) / map_stats = {full / stats_ms:.1f}")
    if args.out:
        Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    sys.exit(main())
