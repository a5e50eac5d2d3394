#!/usr/bin/env python3
"""Factor records: what the compact container costs and saves beside the 24-byte records and the v2 file.

    python tools/packed_factors_probe.py [--lg 30] [--lg-random 28] [--lg-collection 28] [--genomes 24] [--reps 5]
                                         [--dir DIR] [--out profiles/packed_factors.txt]

One process, one device, three inputs: the benchmark text (bench.py's dna1g at 2^lg bases), a random text and a
collection of similar genomes (tools/degenerate.py's generator: one random genome and copies 0.1 % apart).  Per input,
medians of --reps after a warm-up of every arm, with ranges:
  (a) the packed path, factorize_packed + write_packed_factors, beside the parent commit's path, which this commit
      leaves as it was: factorize to host records (factorize_array), then the v2 writer (nolzss_write_factor_file).
      Wall times of the call and of the file, the bytes that cross PCIe downwards, the file sizes.
  (b) the device time of the stages of the packed call from nolzss_profile_report.
  (c) bytes per record by nibble class.
  (d) once per input: unpack_factors equals the factorizer's records, decode_packed equals the text.
Runs on the GPU machine only.  No figure is asserted: the byte-exact model tests pin the sizes.  No counter run.
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
from nolzss_amd import _lib, utils  # noqa: E402
from nolzss_amd import _noLZSS as native  # noqa: E402

SCOPES = ("factorize_packed_all", "text_h2d", "literal_gather", "factors_pack_plan", "factors_pack_write",
          "factors_pack_literals", "factors_packed_d2h")
LENGTH_BYTES, CODE_BYTES = (0, 1, 2, 4), (0, 2, 4, 5)


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def mutated(x, seed, rate=1000):  # (tools/degenerate.py)
    y = x.copy()
    r = np.random.default_rng(seed)
    idx = r.integers(0, len(y), size=len(y) // rate)
    y[idx] = np.frombuffer(b"ACGT", dtype=np.uint8)[r.integers(0, 4, size=len(idx))]
    return y


def collection(n, copies):
    base = gen.random_dna(n // copies, 40 + copies)
    return np.concatenate([base] + [mutated(base, 100 * copies + k) for k in range(copies - 1)])


def write_v2(path, f, n):
    _lib.check(_lib.lib.nolzss_write_factor_file(os.fsencode(str(path)), f.ctypes.data if len(f) else None, len(f), 0, 0, n,
                                                 None, 0))


def spread(ts):
    return f"{statistics.median(ts):.1f} ms ({min(ts):.1f}-{max(ts):.1f})"


def one_input(say, name, text, reps, tmp):
    n = len(text)
    packed_path, v2_path = Path(tmp) / "f.nolzfac", Path(tmp) / "f.v2"
    say(f"==== {name}: {n} symbols")
    rows = {k: [] for k in ("packed call", "packed file", "v2 call", "v2 file")}
    reports = []
    s = f = None
    for rep in range(reps + 1):  # the first round of both arms is the warm-up; the arms alternate
        native.profile_enable(True)
        native.profile_reset()
        t_call, s = timed(lambda: native.factorize_packed(text))
        report = native.profile_report()
        native.profile_enable(False)
        native.profile_reset()
        t_file, _ = timed(lambda: utils.write_packed_factors(packed_path, s))
        f = None  # (the block of the round before goes first: two of them are 2.5 GB at 2^30)
        t_call2, f = timed(lambda: native.factorize_array(text))
        t_file2, _ = timed(lambda: write_v2(v2_path, f, n))
        if rep:
            for k, t in zip(rows, (t_call, t_file, t_call2, t_file2)):
                rows[k].append(t)
            reports.append(report)
    z = s["z"]
    sections = sum(len(s[k]) for k in ("control", "data", "literals"))
    size, size2 = os.path.getsize(packed_path), os.path.getsize(v2_path)
    say(f"z = {z} factors ({n / z:.1f} symbols each), {s['n_literals']} literals, literal_mode {s['literal_mode']}")
    say(f"packed path: factorize_packed {spread(rows['packed call'])}, write_packed_factors {spread(rows['packed file'])}")
    say(f"v2 path (parent, unchanged): factorize to host records {spread(rows['v2 call'])}, v2 writer {spread(rows['v2 file'])}")
    both = [a + b for a, b in zip(rows["packed call"], rows["packed file"])]
    both2 = [a + b for a, b in zip(rows["v2 call"], rows["v2 file"])]
    say(f"call + file: packed {spread(both)}, v2 {spread(both2)}; ratio of the medians v2 / packed "
        f"{statistics.median(both2) / statistics.median(both):.2f} (calls alone {statistics.median(rows['v2 call']) / statistics.median(rows['packed call']):.2f})")
    say(f"bytes across PCIe, downwards: packed {sections} (control {len(s['control'])}, data {len(s['data'])}, literals "
        f"{len(s['literals'])}), v2 path {24 * z}: {24 * z / max(sections, 1):.2f} x")
    say(f"file bytes: packed {size}, v2 {size2}: {size2 / size:.2f} x; the text at 2 bits per symbol {n // 4} ({size / (n / 4):.2f} of it)")
    cells = [f"{k} {statistics.median(r.get(k, (0, 0.0, 0))[1] for r in reports):.3f}" for k in SCOPES]
    say("device spans of factorize_packed (ms, medians; a stage and the scopes inside it are separate): " + ", ".join(cells))
    nib = np.frombuffer(s["control"], dtype=np.uint8)
    nib = np.stack([nib & 15, nib >> 4], axis=1).reshape(-1)[:z]
    share = np.bincount(nib, minlength=16) / max(z, 1)
    say(f"bytes per record: {(len(s['control']) + len(s['data'])) / max(z, 1):.3f} of control and data, "
        f"{len(s['literals']) / max(z, 1):.4f} of literals; by class (a: bytes of L, b: bytes of v):")
    for code in range(16):
        if share[code]:
            what = "literal" if code == 0 else f"L in {LENGTH_BYTES[code & 3]}, v in {CODE_BYTES[code >> 2]}"
            cost = 0.5 + LENGTH_BYTES[code & 3] + CODE_BYTES[code >> 2]
            say(f"    a = {code & 3}, b = {code >> 2} ({what}; {cost} bytes): {100 * share[code]:.2f} %")
    # (d) the way back, once
    back = utils.read_packed_factors(packed_path)
    assert back == s
    t_unpack, (records, literals) = timed(lambda: native.unpack_factors(back))
    same = all(np.array_equal(records[k], f[k]) for k in ("start", "length", "ref"))
    del records
    t_decode, (out, _) = timed(lambda: native.decode_packed_array(back))
    equal = out.size == n and np.array_equal(out, np.frombuffer(text, dtype=np.uint8))
    say(f"unpack_factors of the file {t_unpack:.1f} ms: records equal the factorizer's: {same}; decode_packed {t_decode:.1f} ms: "
        f"equals the text: {equal}")
    assert same and equal
    say()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lg", type=int, default=30)
    ap.add_argument("--lg-random", type=int, default=28)
    ap.add_argument("--lg-collection", type=int, default=28)
    ap.add_argument("--genomes", type=int, default=24)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--dir", default="/dev/shm" if os.path.isdir("/dev/shm") else None,
                    help="where the files go (default: a temporary directory in memory, so that no disk is timed)")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "packed_factors.txt"))
    a = ap.parse_args()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text("\n".join(lines) + "\n")

    native.set_device(0)
    say(f"packed factors probe: factorize_packed + write_packed_factors beside factorize to host records + the v2 writer; "
        f"one process, the arms alternating, medians of {a.reps} after a warm-up of both, ranges in brackets")
    say()
    inputs = [(f"the benchmark text (bench.py dna1g, 2^{a.lg})", lambda: gen.repeat_dna(1 << a.lg, seed=0x5EED0003)),
              (f"random DNA, 2^{a.lg_random}", lambda: gen.random_dna(1 << a.lg_random, seed=0x6E6F4C5A)),
              (f"{a.genomes} genomes 0.1 % apart, 2^{a.lg_collection} in all", lambda: collection(1 << a.lg_collection, a.genomes))]
    with tempfile.TemporaryDirectory(dir=a.dir) as tmp:
        for name, make in inputs:
            text = np.ascontiguousarray(make()).tobytes()
            one_input(say, name, text, a.reps, tmp)
    say("no counter run was made")


if __name__ == "__main__":
    main()
