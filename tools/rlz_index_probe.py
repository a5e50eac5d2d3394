#!/usr/bin/env python3
"""Relative-LZ index: target batches matched against a resident reference, against the existing call that sorts
reference and targets together -- on the same inputs, in the same run.

    python tools/rlz_index_probe.py [--lg 24] [--targets 15] [--batches 8] [--reps 5] [--out profiles/r10_rlz_index.txt]

Input: the collection of tools/rlz_probe.py (a reference of 2^lg random bases, `targets` copies 0.1 % apart, every fourth
with an inverted tenth), `batches` such batches with mutations of their own.  Measured:
  - the open of the index (one suffix sort of the reference and its mirror, the copy into the handle);
  - batch 0 through the index and through nolzss_rlz_factorize, alternating, `reps` times after one warm-up each, with
    records and counts only: medians; the results are compared record for record on the way;
  - every batch once through the open index;
  - the stage table (nolzss_profile_report) of one batch through the index, with the shares of the search kernel, the
    chain and the records;
  - the copy ceiling of the run (1 GiB device-to-device, best of 6, HIP events).
Runs on the GPU machine only.
"""
import argparse
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
sys.path.insert(0, str(ROOT / "tools"))

import numpy as np  # noqa: E402

import gen  # noqa: E402
from nolzss_amd import _noLZSS as native  # noqa: E402
from rlz_probe import _COMP, copy_ceiling, mutated, timed  # noqa: E402


def batch_of(ref, k, b):
    targets = []
    for j in range(k):
        t = mutated(ref, 500 + 1000 * b + j)
        if j % 4 == 0:
            a, n = (j + 1) * len(t) // (k + 2), len(t) // 10
            t[a:a + n] = _COMP[t[a:a + n]][::-1]
        targets.append(t.tobytes())
    return targets


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lg", type=int, default=24)
    ap.add_argument("--targets", type=int, default=15)
    ap.add_argument("--batches", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "r10_rlz_index.txt"))
    a = ap.parse_args()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    native.set_device(0)
    ceiling = copy_ceiling()
    ref_arr = gen.random_dna(1 << a.lg, 0x524C5A)
    ref = ref_arr.tobytes()
    first = batch_of(ref_arr, a.targets, 0)
    say(f"relative-LZ index probe: reference 2^{a.lg} bases, batches of {a.targets} targets 0.1 % apart (every fourth with "
        f"an inverted tenth), {sum(map(len, first))} bases per batch, reverse complement on")
    say(f"copy ceiling (1 GiB device-to-device, 2 GiB moved, best of 6): {ceiling:.0f} GB/s")

    t_open, ix = timed(lambda: native.RlzIndexHandle.open(ref, with_rc=True))
    say(f"open: {t_open:.1f} ms (first call on the device: arena and code objects included), handle "
        f"{ix.info['device_bytes'] / 2**20:.0f} MiB = {ix.info['device_bytes'] / len(ref):.1f} bytes per reference base, "
        f"P = {ix.info['prefix_syms']}")
    ix.close()
    t_open, ix = timed(lambda: native.RlzIndexHandle.open(ref, with_rc=True))
    say(f"open again (warm): {t_open:.1f} ms")

    def joint(want):
        return native.rlz_factorize_arrays(ref, first, with_rc=True, want_factors=want)

    def index(want):
        return ix.factorize_arrays(first, want_factors=want)

    for want, label in ((True, "with records"), (False, "counts only")):
        old, new = joint(want), index(want)  # warm-up, and the comparison
        assert old["counts"] == new["counts"] and old["target_offsets"] == new["target_offsets"]
        if want:
            assert all(np.array_equal(x, y) for x, y in zip(old["factors"], new["factors"]))
            say(f"factors per batch {sum(new['counts'])}: the index equals nolzss_rlz_factorize record for record")
        del old, new
        t_new, t_old = [], []
        for _ in range(a.reps):  # alternating
            t_new.append(timed(lambda: index(want))[0])
            t_old.append(timed(lambda: joint(want))[0])
        m_new, m_old = statistics.median(t_new), statistics.median(t_old)
        say(f"{label:13s} index  median {m_new:9.1f} ms   {['%.1f' % t for t in t_new]}")
        say(f"{label:13s} joint  median {m_old:9.1f} ms   {['%.1f' % t for t in t_old]}")
        if m_old > m_new:
            say(f"{label:13s} a batch against the open index takes {m_new / m_old:.2f} of the joint call; the open "
                f"({t_open:.0f} ms) is paid back after {t_open / (m_old - m_new):.1f} batches")
        else:
            say(f"{label:13s} a batch against the open index takes {m_new / m_old:.2f} of the joint call: re-sorting is "
                f"the faster way here, the index never pays for its open")

    times = []
    for b in range(a.batches):
        targets = first if b == 0 else batch_of(ref_arr, a.targets, b)
        times.append(timed(lambda: ix.factorize_arrays(targets, want_factors=True))[0])
        del targets
    say(f"{a.batches} successive batches with records: {['%.1f' % t for t in times]} ms")

    native.profile_enable(True)
    try:
        native.profile_reset()
        t, _ = timed(lambda: index(True))
        rep = native.profile_report()
    finally:
        native.profile_enable(False)
    say(f"stage table of one batch with records (wall {t:.1f} ms with the profiler on; nested scopes are listed too)")
    say(f"  {'stage':24s} {'launches':>8s} {'ms':>9s} {'GB/s':>8s}")
    for name, (count, ms, nbytes) in sorted(rep.items(), key=lambda kv: -kv[1][1]):
        rate = f"{nbytes / (ms * 1e-3) / 1e9:8.0f}" if nbytes and ms else " " * 8
        say(f"  {name:24s} {count:8d} {ms:9.3f} {rate}")
    device_ms = sum(ms for name, (_, ms, _) in rep.items())
    chain = sum(ms for name, (_, ms, _) in rep.items() if name.startswith("chain_") or name == "factor_emit")
    for label, ms in (("search kernel", rep["rlz_index_search"][1]), ("chain", chain), ("records", rep["rlz_index_records"][1])):
        say(f"{label}: {ms:.3f} ms = {ms / device_ms:.2f} of the {device_ms:.1f} ms in profiled stages")
    ix.close()
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
