#!/usr/bin/env python3
"""Range extraction from a relative-LZ archive (nolzss_rlz_archive_extract_device) on one GPU: output rate beside the
copy ceiling of the same device and beside the decoder's stages on the same records.

    python tools/rlz_extract_probe.py [--lg 24] [--targets 15] [--reps 5] [--out profiles/r09_rlz_extract.txt]

Input: the collection of tools/rlz_probe.py -- one reference of 2^lg random bases and `targets` copies of it with 0.1 %
substitutions, every fourth with an inverted tenth.  The archive is built once (RlzArchive.build).  Three range sets, each
into a torch.uint8 tensor on the device, one warm-up and --reps repetitions:
  - every target whole;
  - 2^20 uniformly random 150-byte ranges;
  - 2^16 uniformly random 4096-byte ranges.
Per set: the call between two HIP events on the stream it runs on (the call plans the ranges on the host, uploads
8 bytes per range and waits for the kernel, so this is the caller's price), and, from repetitions of their own under the
library's stage profiler, the kernel alone (rlz_extract) and the upload of the ranges (ranges_h2d); output GB/s =
output bytes over the time, beside the copy ceiling (1 GiB device-to-device, 2 GiB moved, best of 6).  Then
nolzss_decode of the same records with the block as prefix, for its stage times (check, expand, emit; these records
need no jump round) beside the whole-target extraction.
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

from decode_probe import copy_ceiling, profiled  # noqa: E402
from rlz_probe import collection  # noqa: E402
from nolzss_amd import _noLZSS as native  # noqa: E402
from nolzss_amd.genomics import rlz  # noqa: E402

DECODE_STAGES = ("decode_check", "decode_expand", "decode_jump", "decode_emit")


def random_ranges(lengths, count, size, seed):
    rng = np.random.default_rng(seed)
    lengths = np.asarray(lengths, dtype=np.int64)
    target = rng.integers(0, len(lengths), size=count)
    lo = (rng.random(count) * (lengths[target] - size + 1)).astype(np.int64)
    return np.stack([target, lo, lo + size], axis=1).astype(np.uint64)


def spread(ts):
    return f"median {statistics.median(ts):8.3f} ms  min {min(ts):8.3f}  max {max(ts):8.3f}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lg", type=int, default=24)
    ap.add_argument("--targets", type=int, default=15)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "r09_rlz_extract.txt"))
    a = ap.parse_args()
    import torch
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    native.set_device(0)
    ceiling = copy_ceiling(torch)
    ref, targets = collection(a.lg, a.targets)
    factors = rlz.rlz_factorize(ref, targets, with_rc=True)
    literals = rlz.rlz_literals(targets, factors)
    archive = rlz.RlzArchive.from_factors(ref, factors, literals)
    info = archive.info
    lengths = archive.target_lengths
    kinds = archive._arrays["records"]["ref"] >> np.uint64(63)
    say(f"relative-LZ extract probe: reference 2^{a.lg} bases, {a.targets} targets 0.1 % apart (every fourth with an "
        f"inverted tenth); {info['z']} records ({int(kinds.sum())} reverse-complement, {info['n_literals']} literals) over "
        f"{info['total_length']} target bases; the handle holds {info['device_bytes']} bytes of device memory")
    say(f"copy ceiling (1 GiB device-to-device, 2 GiB moved, best of 6): {ceiling:.0f} GB/s")

    sets = [("every target whole", np.array([(j, 0, n) for j, n in enumerate(lengths)], dtype=np.uint64)),
            ("2^20 random 150-byte ranges", random_ranges(lengths, 1 << 20, 150, 1)),
            ("2^16 random 4096-byte ranges", random_ranges(lengths, 1 << 16, 4096, 2))]
    capacity = max(int((r[:, 2] - r[:, 1]).sum()) for _, r in sets)
    out = torch.empty(capacity, dtype=torch.uint8, device="cuda:0")
    stream = torch.cuda.Stream(device="cuda:0")
    torch.cuda.synchronize()
    rates = {}
    for name, ranges in sets:
        total = int((ranges[:, 2] - ranges[:, 1]).sum())

        def call():
            return archive.extract_device(ranges, out.data_ptr(), capacity, stream=stream.cuda_stream)

        assert call() == total  # warm-up
        if name == "every target whole":  # what came out is what went in
            at = 0
            for t in targets[:2]:
                assert out[at:at + len(t)].cpu().numpy().tobytes() == t
                at += len(t)
        calls, kernels, uploads = [], [], []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            call()
            e1.record(stream)
            e1.synchronize()
            calls.append(e0.elapsed_time(e1))
        for _ in range(a.reps):
            _, rep = profiled(call)
            kernels.append(rep["rlz_extract"][1])
            uploads.append(rep["ranges_h2d"][1])
        k, c = statistics.median(kernels), statistics.median(calls)
        rates[name] = total / (k * 1e-3) / 1e9
        say()
        say(f"== {name}: {len(ranges)} ranges, {total} output bytes ==")
        say(f"  call (HIP events around it)  {spread(calls)}   {total / (c * 1e-3) / 1e9:8.1f} GB/s of output")
        say(f"  kernel rlz_extract           {spread(kernels)}   {rates[name]:8.1f} GB/s of output = "
            f"{rates[name] / ceiling:.3f} of the copy ceiling")
        say(f"  upload of the ranges         {spread(uploads)}")
    whole, short = rates["every target whole"], rates["2^20 random 150-byte ranges"]
    say()
    say(f"kernel rate, whole targets over 150-byte ranges: {whole / short:.2f} (the price of the per-range lookups)")

    block, records = archive._arrays["block"], archive._arrays["records"]
    lit = archive._arrays["literals"]
    native.decode_array(records, lit, prefix=block)  # warm-up
    per_stage = {s: [] for s in DECODE_STAGES}
    for _ in range(a.reps):
        (text, dinfo), rep = profiled(lambda: native.decode_array(records, lit, prefix=block))
        for s in DECODE_STAGES:
            per_stage[s].append(rep[s][1] if s in rep else 0.0)
    assert text[len(block):len(block) + len(targets[0])].tobytes() == targets[0] and dinfo["rounds"] == 0
    say()
    say(f"== nolzss_decode of the same records (prefix = the block, {dinfo['rounds']} jump rounds), stage times ==")
    for s in DECODE_STAGES:
        say(f"  {s:14s} {spread(per_stage[s])}")
    stages = sum(statistics.median(per_stage[s]) for s in DECODE_STAGES)
    total = info["total_length"]
    k_whole = total / whole / 1e9 * 1e3
    say(f"decoder stages in all {stages:.3f} ms ({total / (stages * 1e-3) / 1e9:.1f} GB/s of output) against "
        f"{k_whole:.3f} ms of rlz_extract for every target whole: ratio {stages / k_whole:.2f}")
    archive.close()
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
