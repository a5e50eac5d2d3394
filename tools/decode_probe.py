#!/usr/bin/env python3
"""The decoder (nolzss_decode / nolzss_roundtrip_device) on one GPU: how far its stages are from the copy ceiling and
how the decode time compares with the factorization time of the same text.

    python tools/decode_probe.py [--plain-log2n 26 28] [--rc-log2n 26] [--reps 3] [--out profiles/r07_decode.txt]

Texts: tests/gen.py repeat_dna with bench.py's seeds (0x5EED0003 plain, 0x5EED0005 reverse complement), resident in
device memory.  Per text, medians over --reps after one warm-up:
  - wall time of the factorization alone (records built in HBM and left there) and of the device-resident round trip
    (factorize, gather the literals, decode, compare): the difference is what decoding and checking add;
  - the stage table of one round trip (nolzss_profile_report): decode_check, decode_expand, every jump round with the
    unresolved positions entering it, decode_emit, literal_gather, mismatch -- GB/s over their algorithmic bytes
    (expand: 24 B per record + 8 B per position; a round: 24 B per unresolved position; emit: 9 B per position)
    beside the copy ceiling (1 GiB device-to-device, 2 GiB moved, best of 6) measured on the same device;
  - the jump rounds with the tiles that hold no unresolved position skipped (the default) and not
    (NOLZSS_DECODE_TILE_SKIP=0), alternating.
On the first plain text also: nolzss_decode from host records (PCIe both ways) and the per-factor slice decoder of
tests/decode_model.py on the same records.
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

import decode_model  # noqa: E402
import gen  # noqa: E402
from nolzss_amd import _noLZSS as native  # noqa: E402

DECODE_STAGES = ("decode_check", "decode_expand", "decode_jump", "decode_emit")


def copy_ceiling(torch, nbytes=1 << 30, reps=6):
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


def walls(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), ts


def profiled(fn):
    native.profile_enable(True)
    try:
        native.profile_reset()
        out = fn()
        return out, native.profile_report()
    finally:
        native.profile_enable(False)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--plain-log2n", type=int, nargs="*", default=[26, 28])
    ap.add_argument("--rc-log2n", type=int, nargs="*", default=[26])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "r07_decode.txt"))
    a = ap.parse_args()
    import torch
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    native.set_device(0)
    ceiling = copy_ceiling(torch)
    say(f"decode probe; copy ceiling (1 GiB device-to-device, 2 GiB moved, best of 6): {ceiling:.0f} GB/s")
    host_case = None
    for with_rc, lg in [(False, x) for x in a.plain_log2n] + [(True, x) for x in a.rc_log2n]:
        n = 1 << lg
        text = gen.repeat_dna(n, seed=0x5EED0005 if with_rc else 0x5EED0003)
        if host_case is None and not with_rc:
            host_case = (lg, text)
        d = torch.from_numpy(text).to("cuda:0")
        torch.cuda.synchronize()
        ptr = d.data_ptr()
        mode = "reverse complement" if with_rc else "plain"
        say()
        say(f"== 2^{lg} bases, {mode} mode (text resident in device memory) ==")

        def factorize():
            if with_rc:
                return native.factorize_dna_w_rc_device(ptr, n, emit=1)[0]
            return native.factorize_device(ptr, n, emit=1)[0]

        def roundtrip():
            return native.roundtrip_device(ptr, n, with_rc=with_rc)

        t_fact, all_fact = walls(factorize, a.reps)
        t_rt, all_rt = walls(roundtrip, a.reps)
        res, rep = profiled(roundtrip)
        assert res["mismatches"] == 0 and res["n"] == n, res
        say(f"factors {res['z']}, literals {res['n_literals']}, resolved at expand {res['resolved_at_expand']}, "
            f"unresolved entering round 1 {res['max_active']}, rounds {res['rounds']}, mismatches {res['mismatches']}")
        say(f"factorization alone (records left in HBM)  median {t_fact:9.2f} ms   {['%.2f' % t for t in all_fact]}")
        say(f"round trip (factorize, gather, decode, compare) median {t_rt:9.2f} ms   {['%.2f' % t for t in all_rt]}")
        decode_ms = sum(rep[s][1] for s in DECODE_STAGES if s in rep)
        say(f"decode stages (check + expand + rounds + emit, HIP events): {decode_ms:.3f} ms = "
            f"{decode_ms / t_fact:.3f} of the factorization time; round trip minus factorization (wall): "
            f"{t_rt - t_fact:.2f} ms")
        say(f"  {'stage':18s} {'launches':>8s} {'ms':>9s} {'alg. GB':>9s} {'GB/s':>8s} {'of ceiling':>10s} {'unresolved in':>14s}")
        names = ["decode_check", "decode_expand"] + sorted(k for k in rep if k.startswith("decode_jump_")) + \
                ["decode_jump", "decode_emit", "literal_gather", "mismatch"]
        for name in names:
            if name not in rep:
                continue
            count, ms, nbytes = rep[name]
            gbs = nbytes / (ms * 1e-3) / 1e9 if ms else 0.0
            active = f"{int(round(nbytes / 24)):14d}" if name.startswith("decode_jump_") else ""
            say(f"  {name:18s} {count:8d} {ms:9.3f} {nbytes / 1e9:9.3f} {gbs:8.0f} {gbs / ceiling:10.2f} {active}")

        skip_on, skip_off = [], []
        for _ in range(a.reps):
            for flag, acc in (("1", skip_on), ("0", skip_off)):
                os.environ["NOLZSS_DECODE_TILE_SKIP"] = flag
                acc.append(profiled(roundtrip)[1]["decode_jump"][1])
        os.environ.pop("NOLZSS_DECODE_TILE_SKIP", None)
        say(f"jump rounds, resolved tiles skipped: median {statistics.median(skip_on):.3f} ms {['%.3f' % t for t in skip_on]}; "
            f"every tile launched: median {statistics.median(skip_off):.3f} ms {['%.3f' % t for t in skip_off]}")
        del d
        torch.cuda.empty_cache()

    if host_case is not None:
        lg, text = host_case
        data = text.tobytes()
        f = native.factorize_array(data)
        lit = native.literal_symbols(data, f)
        say()
        say(f"== host records of the 2^{lg}-base plain text: {len(f)} records, {len(lit)} literals ==")
        t_dev, all_dev = walls(lambda: native.decode_array(f, lit), a.reps)
        got, info = native.decode_array(f, lit)
        assert got.tobytes() == data
        say(f"nolzss_decode (24-byte records up, text down)   median {t_dev:9.2f} ms   {['%.2f' % t for t in all_dev]}")
        t0 = time.perf_counter()
        rows = decode_model.as_rows(f)
        t_rows = (time.perf_counter() - t0) * 1e3
        t0 = time.perf_counter()
        out = decode_model.decode_slices(rows, lit)
        t_slices = (time.perf_counter() - t0) * 1e3
        assert out == data
        say(f"per-factor slice decoder (tests/decode_model.py, one CPU thread): {t_slices:.0f} ms "
            f"(+ {t_rows:.0f} ms turning the array into rows) = {t_slices / t_dev:.0f} x nolzss_decode")
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
