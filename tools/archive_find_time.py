#!/usr/bin/env python3
"""Relative-LZ archive: locate through the parse, timed against the only route without it.

    python tools/archive_find_time.py [--lg 28] [--genomes 96] [--patterns 10000] [--reps 5] [--out profiles/r05_archive_find.txt]

Collection: `genomes` genomes of 2^lg bases in all, 0.1 % apart, as in tools/degenerate.py: a random base genome and
its mutated copies.  The base genome is the reference of an RlzIndex (reverse complement on); all genomes are appended
to an archive opened over it.  Patterns: 32 bases drawn from the targets at seeded positions, every second one
reverse-complemented.
Timed: the finder's open; count and locate (max_hits 0) through the C ABI on arguments marshalled once, medians of `reps`
runs after a warm-up; and the route without a finder -- extract of every target to the host, then a host scan (numpy:
the 2-bit code of every 32-mer of a target against the sorted codes of the patterns and of their reverse complements).
The counts of both routes are compared.  The stage table of one locate gives the share of the two walks.
Runs on the GPU machine only.  No counter run is made.
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
from nolzss_amd import _lib  # noqa: E402
from nolzss_amd import _noLZSS as native  # noqa: E402
from nolzss_amd.genomics import rlz  # noqa: E402
from rlz_probe import _COMP, mutated, timed  # noqa: E402

M = 32
_CODE = np.zeros(256, dtype=np.uint64)
for _i, _c in enumerate(b"ACGT"):
    _CODE[_c] = _i


def kmer_codes(arr):
    """the 2-bit code of every 32-mer of a byte array of bases (uint64), by doubling"""
    c = _CODE[arr]
    width = 1
    while width < M:  # c[i] holds `width` bases: append the next `width`
        c = (c[:-width] << np.uint64(2 * width)) | c[width:]
        width *= 2
    return c


def host_scan(texts, patterns):
    """occurrences of every 32-base pattern on both strands in the byte arrays `texts`, by 32-mer codes"""
    q = len(patterns)
    fw = kmer_codes(np.frombuffer(b"".join(patterns), dtype=np.uint8))[::M]
    rc = kmer_codes(np.frombuffer(b"".join(_COMP[np.frombuffer(p, dtype=np.uint8)][::-1].tobytes() for p in patterns),
                                  dtype=np.uint8))[::M]
    both = np.concatenate([fw, rc])  # entry j and entry q + j belong to pattern j
    order = np.argsort(both, kind="stable")
    keys = both[order]
    first = np.zeros(len(keys), dtype=np.int64)  # occurrences, at the first entry of each run of equal keys
    for text in texts:
        codes = kmer_codes(text)
        lo = np.searchsorted(keys, codes, side="left")
        hit = keys[np.minimum(lo, len(keys) - 1)] == codes
        first += np.bincount(lo[hit], minlength=len(keys))
    # entries that share a code (equal patterns, a pattern that is its own reverse complement) all get the occurrences
    run = np.cumsum(np.concatenate([[True], keys[1:] != keys[:-1]])) - 1
    per_entry = np.bincount(run, weights=first)[run]
    return np.bincount(order % q, weights=per_entry, minlength=q).astype(np.uint64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lg", type=int, default=28)
    ap.add_argument("--genomes", type=int, default=96)
    ap.add_argument("--patterns", type=int, default=10000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "r05_archive_find.txt"))
    a = ap.parse_args()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    lib = _lib.lib
    native.set_device(0)
    n, k, q = 1 << a.lg, a.genomes, a.patterns
    base = gen.random_dna(n // k, 40 + k)
    genomes = [base] + [mutated(base, 100 * k + j) for j in range(k - 1)]
    rng = np.random.default_rng(7)
    patterns = []
    for j in range(q):
        g = genomes[int(rng.integers(0, k))]
        at = int(rng.integers(0, len(g) - M))
        p = g[at:at + M]
        patterns.append((_COMP[p][::-1] if j % 2 else p).tobytes())
    say(f"relative-LZ archive find: {k} genomes of {len(base)} bases ({k * len(base)} in all), 0.1 % apart; reference = the base "
        f"genome, reverse complement on; {q} patterns of {M} bases drawn from the targets, every second one reverse-complemented")

    ix = rlz.RlzIndex.build(base.tobytes(), with_rc=True)
    t_append, arc = timed(lambda: ix.archive_on_device([g.tobytes() for g in genomes]))
    info = arc.info
    say(f"archive: {info['num_targets']} targets, z = {info['z']} records ({info['n_literals']} literals), "
        f"{info['device_bytes'] / 2**20:.0f} MiB resident; appended in {t_append:.0f} ms")
    t_open, finder = timed(lambda: arc.finder(max_pattern_length=M))
    fi = finder.info
    say(f"finder open: {t_open:.1f} ms; |K| = {fi['kernel_length']} bytes in {fi['intervals']} intervals, "
        f"{fi['device_bytes'] / 2**20:.0f} MiB resident")
    t_open2, f2 = timed(lambda: arc.finder(max_pattern_length=M))
    f2.close()
    say(f"finder open, second time (arena and code warm): {t_open2:.1f} ms")

    h = finder._live()._handle()
    args = native._seq_args(patterns, "pattern")  # marshalled once: the calls below are the library's time
    counts, offsets = np.zeros(q, dtype=np.uint64), np.zeros(q + 1, dtype=np.uint64)

    def count():
        _lib.check(lib.nolzss_rlz_finder_count(h, *args, counts.ctypes.data))

    def locate():
        out, z = C.c_void_p(), C.c_size_t()
        _lib.check(lib.nolzss_rlz_finder_locate(h, *args, 0, counts.ctypes.data, offsets.ctypes.data, C.byref(out), C.byref(z)))
        lib.nolzss_free(out)
        return z.value

    count()
    T = locate()  # warm-up
    say(f"occurrences {int(counts.sum())} ({counts.sum() / q:.1f} per pattern, largest {int(counts.max())}), hits reported {T}")
    for label, fn in (("count", count), ("locate", locate)):
        ts = [timed(fn)[0] for _ in range(a.reps)]
        say(f"{label:7s} median {statistics.median(ts):8.1f} ms   {['%.1f' % t for t in ts]}")
    found = counts.copy()

    native.profile_enable(True)
    try:
        native.profile_reset()
        t, _ = timed(locate)
        rep = native.profile_report()
    finally:
        native.profile_enable(False)
        native.profile_reset()
    say(f"stage table of one locate (wall {t:.1f} ms with the profiler on; nested scopes are listed too)")
    say(f"  {'stage':24s} {'launches':>8s} {'ms':>9s}")
    for name, (launches, ms, _) in sorted(rep.items(), key=lambda kv: -kv[1][1]):
        say(f"  {name:24s} {launches:8d} {ms:9.3f}")
    whole = rep["rlz_finder_locate"][1]
    walks = sum(rep[s][1] for s in ("rlz_find_walk_count", "rlz_find_walk_emit") if s in rep)
    say(f"the two walks (count and emit): {walks:.3f} ms of {whole:.3f} ms on the stream = {100 * walks / whole:.1f} %")

    # the route without a finder: every target to the host, then a host scan
    def extract_all():
        return [arc.extract_array(np.array([[j, 0, len(genomes[j])]], dtype=np.uint64))[0] for j in range(k)]

    t_extract, texts = timed(extract_all)
    t_scan, host = timed(lambda: host_scan(texts, patterns))
    assert np.array_equal(host, found), "the host scan and the finder disagree"
    say(f"without a finder: extract of every target {t_extract:.0f} ms ({k * len(base) / t_extract / 1e6:.2f} GB/s to the host), "
        f"host scan {t_scan:.0f} ms (numpy, one thread); the counts of all {q} patterns equal the finder's")
    finder.close()
    arc.close()
    ix.close()
    say()
    say("no counter run was made")
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
