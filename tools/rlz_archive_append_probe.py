#!/usr/bin/env python3
"""Relative-LZ archive: a batch appended from the index on the device against the existing path through the host -- on
the same inputs, in the same run.

    python tools/rlz_archive_append_probe.py [--lg 24] [--targets 15] [--reps 5] [--out profiles/r11_rlz_archive_append.txt]

Two shapes: the collection of tools/rlz_index_probe.py (a reference of 2^lg random bases, `targets` copies 0.1 % apart,
every fourth with an inverted tenth), and the same with the copies 5 % apart (short records, many of them).  For each:
  - ix.archive(targets) -- records down, numpy, records up: the yardstick -- and ix.archive_on_device(targets),
    alternating, `reps` times after one warm-up each: medians and the spread; the exports are compared on the way;
  - the stage table (nolzss_profile_report) of one append.
The copy ceiling of the run (1 GiB device-to-device, best of 6, HIP events) is recorded.  Runs on the GPU machine only.
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
from nolzss_amd.genomics import rlz  # noqa: E402
from rlz_probe import _COMP, copy_ceiling, mutated, timed  # noqa: E402


def batch_of(ref, k, rate):
    targets = []
    for j in range(k):
        t = mutated(ref, 500 + j, rate)
        if j % 4 == 0:
            a, n = (j + 1) * len(t) // (k + 2), len(t) // 10
            t[a:a + n] = _COMP[t[a:a + n]][::-1]
        targets.append(t.tobytes())
    return targets


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lg", type=int, default=24)
    ap.add_argument("--targets", type=int, default=15)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "r11_rlz_archive_append.txt"))
    a = ap.parse_args()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    native.set_device(0)
    ceiling = copy_ceiling()
    ref_arr = gen.random_dna(1 << a.lg, 0x524C5A)
    ref = ref_arr.tobytes()
    say(f"relative-LZ archive append probe: reference 2^{a.lg} bases, one batch of {a.targets} targets (every fourth with "
        f"an inverted tenth), reverse complement on")
    say(f"copy ceiling (1 GiB device-to-device, 2 GiB moved, best of 6): {ceiling:.0f} GB/s")
    ix = rlz.RlzIndex.build(ref, with_rc=True)

    def host():
        with ix.archive(targets) as arc:
            return arc.info

    def device():
        with ix.archive_on_device(targets) as arc:
            return arc.info

    for rate, label in ((1000, "0.1 % apart"), (20, "5 % apart")):
        targets = batch_of(ref_arr, a.targets, rate)
        say()
        say(f"targets {label}: {sum(map(len, targets))} bases")
        with ix.archive(targets) as old, ix.archive_on_device(targets) as new:  # warm-up, and the comparison
            block, records, literals = new._live().export()
            assert block == old._arrays["block"].tobytes() and literals == old._arrays["literals"].tobytes()
            assert np.array_equal(records, old._arrays["records"]) and new.target_lengths == old.target_lengths
            info = new.info
            say(f"records {info['z']} ({info['n_literals']} literals), {info['total_length'] / max(info['z'], 1):.1f} bases per "
                f"record: the export of the appended archive equals the host path's arrays; handle "
                f"{info['device_bytes'] / 2**20:.0f} MiB")
            del block, records, literals
        t_new, t_old = [], []
        for _ in range(a.reps):  # alternating
            t_new.append(timed(device)[0])
            t_old.append(timed(host)[0])
        m_new, m_old = statistics.median(t_new), statistics.median(t_old)
        say(f"on device  median {m_new:9.1f} ms  min {min(t_new):9.1f}  max {max(t_new):9.1f}   {['%.1f' % t for t in t_new]}")
        say(f"via host   median {m_old:9.1f} ms  min {min(t_old):9.1f}  max {max(t_old):9.1f}   {['%.1f' % t for t in t_old]}")
        say(f"the append on the device takes {m_new / m_old:.2f} of the path through the host "
            f"({m_old - m_new:+.1f} ms per batch)")
        native.profile_enable(True)
        try:
            native.profile_reset()
            t, _ = timed(device)
            rep = native.profile_report()
        finally:
            native.profile_enable(False)
            native.profile_reset()
        say(f"stage table of one open_index + append (wall {t:.1f} ms with the profiler on; nested scopes are listed too)")
        say(f"  {'stage':28s} {'launches':>8s} {'ms':>9s} {'GB/s':>8s}")
        for name, (count, ms, nbytes) in sorted(rep.items(), key=lambda kv: -kv[1][1]):
            gbs = f"{nbytes / (ms * 1e-3) / 1e9:8.0f}" if nbytes and ms else " " * 8
            say(f"  {name:28s} {count:8d} {ms:9.3f} {gbs}")
        del targets
    ix.close()
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
