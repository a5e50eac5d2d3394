#!/usr/bin/env python3
"""Relative-LZ index: pattern count and locate queries, measured on the reference of tools/rlz_index_probe.py.

    python tools/rlz_index_locate_probe.py [--lg 24] [--lgq 20] [--reps 5] [--out profiles/r12_rlz_index_locate.txt]

Input: the reference of 2^lg random bases of tools/rlz_index_probe.py, reverse complement on.  Two pattern sets of 2^lgq
patterns each, half cut from the reference or its reverse complement and half of those cuts with one substitution:
  - 32 bases: a seed look-up, about one hit per present pattern;
  - 12 bases: many hits each, so that the expansion and the sort show.
Measured per set: the C ABI calls nolzss_rlz_index_count and nolzss_rlz_index_locate (max_hits = 64) on arguments that
are marshalled once -- medians of `reps` after a warm-up --, the stage table (nolzss_profile_report) of one locate, the
pattern kernel's lanes per second next to the positions per second of rlz_index_search on the same batch (the batch
through nolzss_rlz_index_codes, which searches every position of it), and the copy ceiling of the run (1 GiB
device-to-device, best of 6, HIP events).  A sample of the answers is compared with bytes.find on the way.
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
from rlz_probe import _COMP, copy_ceiling, timed  # noqa: E402


def pattern_set(ref_arr, q, m, seed):
    """q patterns of m bases: cuts of the reference, every second cut reverse-complemented, and one substitution in the
    second half of the set"""
    r = np.random.default_rng(seed)
    at = r.integers(0, len(ref_arr) - m, size=q)
    rows = ref_arr[at[:, None] + np.arange(m)[None, :]]
    rows[1::2] = _COMP[rows[1::2]][:, ::-1]
    where = r.integers(0, m, size=q // 2)
    half = rows[q // 2:]
    half[np.arange(q // 2), where] = np.frombuffer(b"ACGT", dtype=np.uint8)[
        (np.searchsorted(np.frombuffer(b"ACGT", dtype=np.uint8), half[np.arange(q // 2), where]) + r.integers(1, 4, size=q // 2)) % 4]
    return [row.tobytes() for row in np.ascontiguousarray(rows)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lg", type=int, default=24)
    ap.add_argument("--lgq", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--max-hits", type=int, default=64)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "r12_rlz_index_locate.txt"))
    a = ap.parse_args()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    lib = _lib.lib
    native.set_device(0)
    ceiling = copy_ceiling()
    ref_arr = gen.random_dna(1 << a.lg, 0x524C5A)
    ref = ref_arr.tobytes()
    rc_ref = _COMP[ref_arr][::-1].tobytes()
    q = 1 << a.lgq
    say(f"relative-LZ index locate probe: reference 2^{a.lg} bases, reverse complement on, 2^{a.lgq} patterns per set (half cut "
        f"from the reference or its reverse complement, half with one substitution), max_hits {a.max_hits}")
    say(f"copy ceiling (1 GiB device-to-device, 2 GiB moved, best of 6): {ceiling:.0f} GB/s")
    t_open, ix = timed(lambda: native.RlzIndexHandle.open(ref, with_rc=True))
    say(f"open: {t_open:.1f} ms, handle {ix.info['device_bytes'] / 2**20:.0f} MiB, P = {ix.info['prefix_syms']}")
    h = ix._handle()

    for m, seed in ((32, 1), (12, 2)):
        patterns = pattern_set(ref_arr, q, m, seed)
        args = native._seq_args(patterns, "pattern")  # marshalled once: the calls below are the library's time
        n = q * (m + 1)
        counts, offsets = np.zeros(q, dtype=np.uint64), np.zeros(q + 1, dtype=np.uint64)

        def count():
            _lib.check(lib.nolzss_rlz_index_count(h, *args, counts.ctypes.data))

        def locate(keep=False):
            out, z = C.c_void_p(), C.c_size_t()
            _lib.check(lib.nolzss_rlz_index_locate(h, *args, a.max_hits, counts.ctypes.data, offsets.ctypes.data,
                                                   C.byref(out), C.byref(z)))
            hits = np.ctypeslib.as_array(C.cast(out, C.POINTER(C.c_uint64)), shape=(2 * z.value,)).copy() if keep and z.value else None
            lib.nolzss_free(out)
            return z.value, hits

        say()
        say(f"---- {q} patterns of {m} bases ({n} batch positions)")
        count()
        T, hits = locate(keep=True)  # warm-up, and the comparison of a sample with bytes.find
        hits = hits.view(native.HIT_DTYPE)
        for j in list(range(0, q, q // 64)) + [q - 1]:
            p = patterns[j]
            exp = sorted([(x, 0) for x in _find_all(ref, p)] +
                         [(len(ref) - x - m, 1) for x in _find_all(rc_ref, p)])
            assert int(counts[j]) == len(exp), (j, counts[j], len(exp))
            if len(exp) <= a.max_hits:
                mine = hits[int(offsets[j]):int(offsets[j + 1])]
                assert [(int(x["position"]), int(x["is_rc"])) for x in mine] == exp, j
        present = int((counts > 0).sum())
        say(f"patterns with a hit {present} ({present / q:.2f}), occurrences {int(counts.sum())}, largest count {int(counts.max())}, "
            f"hits reported {T} ({T / q:.2f} per pattern); a sample of {len(range(0, q, q // 64)) + 1} patterns equals bytes.find")
        del hits
        for label, fn in (("count", count), ("locate", locate)):
            ts = [timed(fn)[0] for _ in range(a.reps)]
            med = statistics.median(ts)
            say(f"{label:7s} median {med:8.1f} ms   {['%.1f' % t for t in ts]}   {q / med / 1e3:.1f} M patterns/s")

        native.profile_enable(True)
        try:
            native.profile_reset()
            t, _ = timed(locate)
            rep = native.profile_report()
            native.profile_reset()
            code = np.zeros(n, dtype=np.uint32)
            _lib.check(lib.nolzss_rlz_index_codes(h, *args, code.ctypes.data))
            search = native.profile_report()["rlz_index_search"]
        finally:
            native.profile_enable(False)
            native.profile_reset()
        say(f"stage table of one locate (wall {t:.1f} ms with the profiler on; nested scopes are listed too)")
        say(f"  {'stage':24s} {'launches':>8s} {'ms':>9s} {'GB/s':>8s}")
        for name, (launches, ms, nbytes) in sorted(rep.items(), key=lambda kv: -kv[1][1]):
            rate = f"{nbytes / (ms * 1e-3) / 1e9:8.0f}" if nbytes and ms else " " * 8
            say(f"  {name:24s} {launches:8d} {ms:9.3f} {rate}")
        pat_ms = rep["rlz_index_pattern"][1]
        say(f"pattern kernel: {pat_ms:.3f} ms = {q / pat_ms / 1e6:.2f} G lanes/s (one lane per pattern)")
        say(f"rlz_index_search on the same batch: {search[1]:.3f} ms = {n / search[1] / 1e6:.2f} G positions/s (one lane per "
            f"position, {m + 1} positions per pattern)")
        if T:
            exp_ms = rep["rlz_index_hits"][1] + rep["rlz_locate_sort"][1] + rep["rlz_index_hit_records"][1]
            say(f"expansion, sort and unpacking: {exp_ms:.3f} ms for {T} hits = {T / exp_ms / 1e6:.2f} G hits/s")
    ix.close()
    say()
    say("no counter run was made")
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text("\n".join(lines) + "\n")


def _find_all(text, p):
    out, at = [], text.find(p)
    while at >= 0:
        out.append(at)
        at = text.find(p, at + 1)
    return out


if __name__ == "__main__":
    main()
