#!/usr/bin/env python3
"""Relative-LZ index: the maximal repeats of the reference, measured on the reference of tools/rlz_index_locate_probe.py
with copies planted into it.

    python tools/rlz_index_repeats_probe.py [--lg 24] [--copies 2048] [--reps 5] [--out profiles/rlz_index_repeats.txt]

Input: the reference of 2^lg random bases of tools/rlz_index_probe.py, reverse complement on, in which `copies` stretches
of 64 .. 2048 bases are overwritten by a copy of another stretch, every second one inverted (reverse-complemented), each
with 1 % substitutions -- so that records exist beyond the chance repeats of random bases.
Measured for min_length 20 and 12 (min_count 2, max_hits 64): the C ABI calls nolzss_rlz_index_repeat_count and
nolzss_rlz_index_repeats -- medians of `reps` after a warm-up --, the stage table (nolzss_profile_report) of one repeats
call, the flags stage next to the open of the index on the same reference, and the copy ceiling of the run (1 GiB
device-to-device, best of 6, HIP events).  A sample of the records is compared with bytes.find on the way: the count and
the hits of the record's string on both strands, and that it extends neither way.
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


def planted(ref_arr, copies, seed):
    r = np.random.default_rng(seed)
    out = ref_arr.copy()
    letters = np.frombuffer(b"ACGT", dtype=np.uint8)
    for j in range(copies):
        n = int(r.integers(64, 2049))
        src, dst = int(r.integers(0, len(out) - n)), int(r.integers(0, len(out) - n))
        piece = out[src:src + n].copy()
        if j & 1:
            piece = _COMP[piece][::-1].copy()
        where = r.integers(0, n, size=max(n // 100, 1))
        piece[where] = letters[r.integers(0, 4, size=len(where))]
        out[dst:dst + n] = piece
    return out


def _find_all(text, p):
    out, at = [], text.find(p)
    while at >= 0:
        out.append(at)
        at = text.find(p, at + 1)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lg", type=int, default=24)
    ap.add_argument("--copies", type=int, default=2048)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--max-hits", type=int, default=64)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "rlz_index_repeats.txt"))
    a = ap.parse_args()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    lib = _lib.lib
    native.set_device(0)
    ceiling = copy_ceiling()
    ref_arr = planted(gen.random_dna(1 << a.lg, 0x524C5A), a.copies, 7)
    ref = ref_arr.tobytes()
    rc_ref = _COMP[ref_arr][::-1].tobytes()
    B = len(ref)
    say(f"relative-LZ index repeats probe: reference 2^{a.lg} bases with {a.copies} planted copies of 64 .. 2048 bases (every "
        f"second one inverted, 1 % substitutions), reverse complement on, min_count 2, max_hits {a.max_hits}")
    say(f"copy ceiling (1 GiB device-to-device, 2 GiB moved, best of 6): {ceiling:.0f} GB/s")
    native.RlzIndexHandle.open(ref, with_rc=True).close()  # warm-up of the open
    opens = []
    for _ in range(a.reps):
        t_open, ix = timed(lambda: native.RlzIndexHandle.open(ref, with_rc=True))
        opens.append(t_open)
        if len(opens) < a.reps:
            ix.close()
    t_open = statistics.median(opens)
    say(f"open: median {t_open:.1f} ms {['%.1f' % t for t in opens]}, handle {ix.info['device_bytes'] / 2**20:.0f} MiB, "
        f"{ix.info['index_length']} ranks, P = {ix.info['prefix_syms']}")
    h = ix._handle()

    for min_length in (20, 12):
        def count():
            out = C.c_uint64()
            _lib.check(lib.nolzss_rlz_index_repeat_count(h, min_length, 2, C.byref(out)))
            return out.value

        def repeats(keep=False):
            res = _lib.RlzRepeatsResult()
            try:
                _lib.check(lib.nolzss_rlz_index_repeats(h, min_length, 2, a.max_hits, C.byref(res)))
                S, T = res.num_repeats, res.num_hits
                if not keep:
                    return S, T, None, None, None
                recs = np.zeros(S, dtype=native.REPEAT_DTYPE)
                hits = np.zeros(T, dtype=native.HIT_DTYPE)
                offsets = np.ctypeslib.as_array(C.cast(res.hit_offsets, C.POINTER(C.c_uint64)), shape=(S + 1,)).copy()
                if S:
                    C.memmove(recs.ctypes.data, res.repeats, S * recs.itemsize)
                if T:
                    C.memmove(hits.ctypes.data, res.hits, T * hits.itemsize)
                return S, T, recs, offsets, hits
            finally:
                lib.nolzss_free_rlz_repeats_result(C.byref(res))

        say()
        say(f"---- min_length {min_length}")
        S, T, recs, offsets, hits = repeats(keep=True)  # warm-up, and the comparison of a sample with bytes.find
        assert count() == S
        assert np.all(np.diff((recs["position"] << np.uint64(32)) | recs["length"]) > 0)  # ascending, the key unique
        sample = list(range(0, S, max(S // 48, 1)))
        for j in sample:
            p, L = int(recs["position"][j]), int(recs["length"][j])
            w = ref[p:p + L]
            exp = sorted([(x, 0) for x in _find_all(ref, w)] + [(B - x - L, 1) for x in _find_all(rc_ref, w)])
            assert int(recs["count"][j]) == len(exp) and exp[0] == (p, 0), (j, recs[j], exp[:4])
            if len(exp) <= a.max_hits:
                mine = hits[int(offsets[j]):int(offsets[j + 1])]
                assert [(int(x["position"]), int(x["is_rc"])) for x in mine] == exp, j
            # neither extension is shared by every occurrence (the block is one record: its ends are the end marks)
            right, left = set(), set()
            for x, s in exp:
                after = ref[x + L] if x + L < B else None
                before = ref[x - 1] if x > 0 else None
                if s:  # the reverse strand swaps the sides and complements
                    after, before = (None if before is None else int(_COMP[before])), (None if after is None else int(_COMP[after]))
                right.add((x, s, "end") if after is None else after)
                left.add((x, s, "end") if before is None else before)
            assert len(right) > 1 and len(left) > 1, (j, recs[j])
        say(f"records {S}, longest {int(recs['length'].max()) if S else 0} bases, largest count {int(recs['count'].max()) if S else 0}, "
            f"palindromes {int(recs['palindrome'].sum())}, hits reported {T} ({T / max(S, 1):.2f} per record); a sample of "
            f"{len(sample)} records equals bytes.find and extends neither way")
        del recs, hits, offsets
        for label, fn in (("repeat_count", count), ("repeats", repeats)):
            ts = [timed(fn)[0] for _ in range(a.reps)]
            med = statistics.median(ts)
            say(f"{label:13s} median {med:8.1f} ms   {['%.1f' % t for t in ts]}")

        native.profile_enable(True)
        try:
            native.profile_reset()
            t, _ = timed(repeats)
            rep = native.profile_report()
        finally:
            native.profile_enable(False)
            native.profile_reset()
        say(f"stage table of one repeats call (wall {t:.1f} ms with the profiler on; nested scopes are listed too)")
        say(f"  {'stage':24s} {'launches':>8s} {'ms':>9s} {'GB/s':>8s}")
        for name, (launches, ms, nbytes) in sorted(rep.items(), key=lambda kv: -kv[1][1]):
            rate = f"{nbytes / (ms * 1e-3) / 1e9:8.0f}" if nbytes and ms else " " * 8
            say(f"  {name:24s} {launches:8d} {ms:9.3f} {rate}")
        n = ix.info["index_length"]
        flags = rep["rlz_repeat_left"][1] + rep["rlz_repeat_flags"][1] + rep["rlz_repeat_scans"][1]
        say(f"flags stage (left context, both scans, interval flags): {flags:.3f} ms = {n / flags / 1e6:.2f} G ranks/s; "
            f"{flags / t_open:.3f} of the open of the same reference ({t_open:.1f} ms)")
    ix.close()
    say()
    say("no counter run was made")
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
