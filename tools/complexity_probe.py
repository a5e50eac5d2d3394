#!/usr/bin/env python3
"""The complexity table's counting step: count_factors_batch_both (both counts of every record from ONE suffix sort
per pipeline run) against the two calls it replaces, on the same host-resident records and devices, in one process.

    python tools/complexity_probe.py [--shape a|b|c|all] [--reps 5] [--devices 0] [--stages]

Shapes (records on the host, as the table holds them):
  a  BASELINE config 4: 512 records x 4 Mi bases (tests/gen.py: fasta_records)
  b  4096 records x 16 Ki bases (merged runs only)
  c  one 2^28-base record with 40 % copied blocks (tests/gen.py: repeat_dna)
Two-call form: a, b -- factorize_batch(want_factors=False) + factorize_batch(with_rc=True, want_factors=False);
c -- count_factors + count_factors_dna_w_rc.  The two forms alternate, one warm-up each, then --reps timed
repeats each; median and spread (min - max) are printed, and the counts of both forms must agree.
--stages: the stage table (nolzss_profile_report) of one fused call at shape (c).
"""
import argparse
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import gen  # noqa: E402
from nolzss_amd import _noLZSS as native  # noqa: E402


def records(shape):
    if shape == "a":
        return [s.tobytes() for _, s in gen.fasta_records(512, 1 << 22)]
    if shape == "b":
        return [s.tobytes() for _, s in gen.fasta_records(4096, 1 << 14, seed0=0x9000)]
    return [gen.repeat_dna(1 << 28, seed=0x5EED0003).tobytes()]


def fused(recs, devices):
    return native.count_factors_batch_both(recs, devices=devices)


def two_calls(recs, devices):
    if len(recs) == 1:
        return [native.count_factors_dna_w_rc(recs[0])], [native.count_factors(recs[0])]
    no_rc, _ = native.factorize_batch(recs, devices=devices, want_factors=False)
    w_rc, _ = native.factorize_batch(recs, devices=devices, want_factors=False, with_rc=True)
    return w_rc, no_rc


def timed(fn, *args):
    t0 = time.perf_counter()
    out = fn(*args)
    return (time.perf_counter() - t0) * 1e3, out


def probe(shape, reps, devices):
    recs = records(shape)
    bases = sum(len(r) for r in recs)
    # (the single record of shape c goes to the current device, as count_factors does)
    devs = devices if shape != "c" else [devices[0]]
    native.set_device(devs[0])
    _, exp = timed(two_calls, recs, devs)
    _, got = timed(fused, recs, devs)
    assert got == exp, f"shape {shape}: the fused counts differ from the two calls"
    t_two, t_fused = [], []
    for _ in range(reps):
        t_two.append(timed(two_calls, recs, devs)[0])
        t_fused.append(timed(fused, recs, devs)[0])
    m2, mf = statistics.median(t_two), statistics.median(t_fused)
    print(f"shape {shape}: {len(recs)} records, {bases} bases, devices {devs}")
    print(f"  two calls  median {m2:9.1f} ms   spread {min(t_two):9.1f} - {max(t_two):9.1f} ms   {t_two}")
    print(f"  fused      median {mf:9.1f} ms   spread {min(t_fused):9.1f} - {max(t_fused):9.1f} ms   {t_fused}")
    print(f"  ratio two / fused (medians) {m2 / mf:.3f}   worst case (slowest fused vs fastest two) "
          f"{min(t_two) / max(t_fused):.3f}")
    print(f"  counts equal: {sum(got[0])} factors with RC, {sum(got[1])} without")
    sys.stdout.flush()
    return recs


def stages(recs):
    native.profile_enable(True)
    try:
        fused(recs, [0])  # (warm)
        native.profile_reset()
        t, _ = timed(fused, recs, [0])
        rep = native.profile_report()
    finally:
        native.profile_enable(False)
    print(f"stage table of one fused call at shape c ({len(recs[0])} bases, wall {t:.1f} ms with the profiler on)")
    print(f"  {'stage':24s} {'launches':>8s} {'ms':>9s}")
    for name, (count, ms, _) in sorted(rep.items(), key=lambda kv: -kv[1][1]):
        print(f"  {name:24s} {count:8d} {ms:9.3f}")
    print("  (plain_chain spans the chain_* / factor stages of the second chain: those appear in both lines)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="all", choices=["a", "b", "c", "all"])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--devices", default="0")
    ap.add_argument("--stages", action="store_true")
    a = ap.parse_args()
    devices = [int(d) for d in a.devices.split(",")]
    recs_c = None
    for shape in (["a", "b", "c"] if a.shape == "all" else [a.shape]):
        recs = probe(shape, a.reps, devices)
        if shape == "c":
            recs_c = recs
    if a.stages:
        stages(recs_c if recs_c is not None else records("c"))


if __name__ == "__main__":
    main()
