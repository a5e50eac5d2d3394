#!/usr/bin/env python3
"""Relative LZ of a collection against one reference: stage times, the rate of the candidate stage against the copy
ceiling of the same device, and the cost of the separate calls a user would make without it.

    python tools/rlz_probe.py [--lg 24] [--targets 15] [--reps 3] [--out profiles/r05_rlz.txt]

Input: one reference of 2^lg random bases and `targets` copies of it with 0.1 % substitutions (the generator of
tools/degenerate.py); every fourth target carries an inverted (reverse-complemented) segment of a tenth of its length,
so that the other strand is exercised.  Measured, with one warm-up each:
  - rlz_count_factors / rlz_factorize_arrays wall time (host bytes in, counts / records out);
  - the stage table (nolzss_profile_report) of one counts-only run, and the GB/s of rlz_candidates and
    rlz_text_order over their algorithmic bytes;
  - the copy ceiling: a device-to-device copy of 1 GiB (2 GiB moved), best of 6, HIP events -- what bench.py --full
    reports as peak_measured;
  - `targets` separate factorize_dna_w_reference_seq calls (binary-file form: no Python tuples).  Those calls have
    other semantics (a target also copies from itself) and other counts: the comparison is of cost only.
"""
import argparse
import os
import statistics
import sys
import tempfile
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import numpy as np  # noqa: E402

import gen  # noqa: E402
from nolzss_amd import _noLZSS as native  # noqa: E402

_COMP = np.zeros(256, dtype=np.uint8)
for _a, _b in zip(b"ACGT", b"TGCA"):
    _COMP[_a] = _b


def mutated(x, seed, rate=1000):
    y = x.copy()
    r = np.random.default_rng(seed)
    idx = r.integers(0, len(y), size=len(y) // rate)
    y[idx] = np.frombuffer(b"ACGT", dtype=np.uint8)[r.integers(0, 4, size=len(idx))]
    return y


def collection(lg, k):
    ref = gen.random_dna(1 << lg, 0x524C5A)
    targets = []
    for j in range(k):
        t = mutated(ref, 500 + j)
        if j % 4 == 0:
            a, n = (j + 1) * len(t) // (k + 2), len(t) // 10
            t[a:a + n] = _COMP[t[a:a + n]][::-1]
        targets.append(t.tobytes())
    return ref.tobytes(), targets


def copy_ceiling(nbytes=1 << 30, reps=6):
    import torch
    a = torch.empty(nbytes, dtype=torch.uint8, device="cuda:0")
    b = torch.empty(nbytes, dtype=torch.uint8, device="cuda:0")
    a.zero_()
    b.copy_(a)
    torch.cuda.synchronize()
    best = float("inf")
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        b.copy_(a)
        e1.record()
        e1.synchronize()
        best = min(best, e0.elapsed_time(e1))
    del a, b
    torch.cuda.empty_cache()
    return 2.0 * nbytes / (best * 1e-3) / 1e9


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lg", type=int, default=24)
    ap.add_argument("--targets", type=int, default=15)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "r05_rlz.txt"))
    a = ap.parse_args()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    native.set_device(0)
    ceiling = copy_ceiling()
    ref, targets = collection(a.lg, a.targets)
    total = len(ref) + sum(map(len, targets))
    say(f"relative LZ probe: reference 2^{a.lg} bases, {a.targets} targets 0.1 % apart (every fourth with an inverted "
        f"tenth), {total} bases in all, reverse complement on")
    say(f"copy ceiling (1 GiB device-to-device, 2 GiB moved, best of 6): {ceiling:.0f} GB/s")

    def counts():
        return native.rlz_factorize_arrays(ref, targets, with_rc=True, want_factors=False)["counts"]

    def records():
        return native.rlz_factorize_arrays(ref, targets, with_rc=True, want_factors=True)

    _, z = timed(counts)
    t_counts = [timed(counts)[0] for _ in range(a.reps)]
    _, full = timed(records)
    t_records = [timed(records)[0] for _ in range(a.reps)]
    assert full["counts"] == z
    rc_factors = sum(int((f["ref"] >> np.uint64(63)).sum()) for f in full["factors"])
    del full
    say(f"factors per target: {z}")
    say(f"factors in all {sum(z)}, reverse-complement factors {rc_factors}")
    say(f"rlz counts only   median {statistics.median(t_counts):9.1f} ms   {['%.1f' % t for t in t_counts]}")
    say(f"rlz with records  median {statistics.median(t_records):9.1f} ms   {['%.1f' % t for t in t_records]}")

    native.profile_enable(True)
    try:
        native.profile_reset()
        t, _ = timed(counts)
        rep = native.profile_report()
    finally:
        native.profile_enable(False)
    say(f"stage table of one counts-only run (wall {t:.1f} ms with the profiler on; nested scopes are listed too)")
    say(f"  {'stage':24s} {'launches':>8s} {'ms':>9s} {'GB/s':>8s}")
    for name, (count, ms, nbytes) in sorted(rep.items(), key=lambda kv: -kv[1][1]):
        rate = f"{nbytes / (ms * 1e-3) / 1e9:8.0f}" if nbytes and ms else " " * 8
        say(f"  {name:24s} {count:8d} {ms:9.3f} {rate}")
    for name in ("rlz_candidates", "rlz_text_order"):
        count, ms, nbytes = rep[name]
        gbs = nbytes / (ms * 1e-3) / 1e9
        say(f"{name}: {ms:.3f} ms over {nbytes:.0f} algorithmic bytes = {gbs:.0f} GB/s = {gbs / ceiling:.2f} of the copy "
            f"ceiling")

    out = os.path.join(tempfile.gettempdir(), f"nolzss_rlz_probe_{os.getpid()}.bin")
    rs = ref.decode()

    def separate():
        return [native.factorize_dna_w_reference_seq_file(rs, t.decode(), out) for t in targets]

    try:
        timed(lambda: native.factorize_dna_w_reference_seq_file(rs, targets[0].decode(), out))
        t_sep, z_sep = timed(separate)
    finally:
        if os.path.exists(out):
            os.remove(out)
    say(f"{a.targets} separate factorize_dna_w_reference_seq_file calls: {t_sep:.1f} ms in all, factors {sum(z_sep)} "
        f"(other semantics, other counts: cost only)")
    say(f"ratio separate calls / one relative-LZ run with records: {t_sep / statistics.median(t_records):.2f}")
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
