#!/usr/bin/env python3
"""Relative-LZ index: maximal match seeds of reads and contigs, measured on the reference of tools/rlz_index_probe.py.

    python tools/rlz_index_seeds_probe.py [--lg 24] [--lgreads 18] [--lgcontigs 12] [--reps 5]
                                          [--out profiles/r13_rlz_index_seeds.txt]

Input: the reference of 2^lg random bases of tools/rlz_index_probe.py, reverse complement on.  Two target sets:
  - 2^lgreads reads of 150 bases cut from either strand, 1 % substitutions;
  - 2^lgcontigs contigs of 10 000 bases cut from either strand, 0.1 % substitutions.
Measured per set, alternating, medians of `reps` after a warm-up of both:
  - seeds: the C ABI call nolzss_rlz_index_seeds (min_length 20, max_hits 64) on arguments that are marshalled once, its
    result freed;
  - the route a user had to take before it: nolzss_rlz_index_codes on the same arguments, the selection of the
    left-maximal positions of at least min_length in numpy, the substrings cut out and marshalled, and
    nolzss_rlz_index_locate of them with the same cap.  Its four steps are timed separately.
Then the stage table (nolzss_profile_report) of one seeds call, and a sample of seeds compared with bytes.find: the
count and the hits of the seed's bytes on both strands, and that neither extension by one base occurs.  The two routes'
seeds, counts and hits are compared in full on the way.  Runs on the GPU machine only.  No counter run is made.
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
from rlz_index_locate_probe import _find_all  # noqa: E402
from rlz_probe import _COMP, timed  # noqa: E402

ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


def cuts(ref_arr, count, length, rate, seed):
    """count cuts of `length` bases, every second one reverse-complemented, each base substituted with probability rate"""
    r = np.random.default_rng(seed)
    at = r.integers(0, len(ref_arr) - length, size=count)
    rows = ref_arr[at[:, None] + np.arange(length)[None, :]]
    rows[1::2] = _COMP[rows[1::2]][:, ::-1]
    where = r.random(rows.shape) < rate
    rows[where] = ACGT[(np.searchsorted(ACGT, rows[where]) + r.integers(1, 4, size=int(where.sum()))) % 4]
    return np.ascontiguousarray(rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lg", type=int, default=24)
    ap.add_argument("--lgreads", type=int, default=18)
    ap.add_argument("--lgcontigs", type=int, default=12)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--min-length", type=int, default=20)
    ap.add_argument("--max-hits", type=int, default=64)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "r13_rlz_index_seeds.txt"))
    a = ap.parse_args()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    lib = _lib.lib
    native.set_device(0)
    ref_arr = gen.random_dna(1 << a.lg, 0x524C5A)
    ref = ref_arr.tobytes()
    rc_ref = _COMP[ref_arr][::-1].tobytes()
    say(f"relative-LZ index seeds probe: reference 2^{a.lg} bases, reverse complement on, min_length {a.min_length}, "
        f"max_hits {a.max_hits}")
    t_open, ix = timed(lambda: native.RlzIndexHandle.open(ref, with_rc=True))
    say(f"open: {t_open:.1f} ms, handle {ix.info['device_bytes'] / 2**20:.0f} MiB, P = {ix.info['prefix_syms']}")
    h = ix._handle()

    sets = (("reads", 1 << a.lgreads, 150, 0.01, 1), ("contigs", 1 << a.lgcontigs, 10_000, 0.001, 2))
    for label, k, length, rate, seed in sets:
        rows = cuts(ref_arr, k, length, rate, seed)
        targets = [row.tobytes() for row in rows]
        args = native._seq_args(targets, "target")  # marshalled once: both routes start from these arguments
        n = k * (length + 1)
        flat = np.concatenate([rows, np.ones((k, 1), dtype=np.uint8)], axis=1).reshape(-1)  # Tcat, as the library lays it out
        first = (np.arange(n) % (length + 1)) == 0

        def seeds(keep=False):
            res = _lib.RlzSeedsResult()
            try:
                _lib.check(lib.nolzss_rlz_index_seeds(h, *args, a.min_length, a.max_hits, C.byref(res)))
                if not keep:
                    return res.num_seeds, res.num_hits
                S, T = res.num_seeds, res.num_hits
                s = np.ctypeslib.as_array(C.cast(res.seeds, C.POINTER(C.c_uint64)), shape=(4 * S,)).copy().view(native.SEED_DTYPE)
                o = np.ctypeslib.as_array(C.cast(res.hit_offsets, C.POINTER(C.c_uint64)), shape=(S + 1,)).copy()
                f = np.ctypeslib.as_array(C.cast(res.hits, C.POINTER(C.c_uint64)), shape=(2 * T,)).copy().view(native.HIT_DTYPE)
                return s, o, f
            finally:
                lib.nolzss_free_rlz_seeds_result(C.byref(res))

        def today(keep=False):
            """-> the four step times, and with keep the route's answer"""
            code = np.zeros(n, dtype=np.uint32)
            t_codes, _ = timed(lambda: _lib.check(lib.nolzss_rlz_index_codes(h, *args, code.ctypes.data)))

            def select():
                ms = code & np.uint32(0x7fffffff)
                ms[length::length + 1] = 0  # (the separators: only target positions are specified)
                left = np.concatenate([np.zeros(1, dtype=np.uint32), ms[:-1]])
                return np.flatnonzero((ms >= max(a.min_length, 1)) & (first | (left <= ms))), ms
            t_select, (at, ms) = timed(select)

            def cut():
                raw = flat.tobytes()
                return native._seq_args([raw[p:p + L] for p, L in zip(at.tolist(), ms[at].tolist())], "pattern")
            t_cut, pargs = timed(cut)
            q = len(at)
            counts, offsets = np.zeros(q, dtype=np.uint64), np.zeros(q + 1, dtype=np.uint64)

            def locate():
                out, z = C.c_void_p(), C.c_size_t()
                _lib.check(lib.nolzss_rlz_index_locate(h, *pargs, a.max_hits, counts.ctypes.data, offsets.ctypes.data,
                                                       C.byref(out), C.byref(z)))
                hits = None
                if keep and z.value:
                    hits = np.ctypeslib.as_array(C.cast(out, C.POINTER(C.c_uint64)), shape=(2 * z.value,)).copy().view(native.HIT_DTYPE)
                lib.nolzss_free(out)
                return hits
            t_locate, hits = timed(locate)
            times = (t_codes, t_select, t_cut, t_locate)
            return (times, at, ms[at], counts, offsets, hits) if keep else times

        say()
        say(f"---- {label}: {k} targets of {length} bases, substitution rate {rate} ({n} batch positions)")
        s, o, f = seeds(keep=True)  # warm-up of both routes, and their answers compared in full
        _, at, lens, counts, offsets, hits = today(keep=True)
        assert np.array_equal(s["target"] * np.uint64(length + 1) + s["start"], at.astype(np.uint64)), "seed positions"
        assert np.array_equal(s["length"], lens.astype(np.uint64)) and np.array_equal(s["count"], counts), "lengths, counts"
        assert np.array_equal(o, offsets) and (len(f) == 0 or np.array_equal(f, hits)), "hits"
        S, T = len(s), len(f)
        sample = np.unique(np.linspace(0, S - 1, 48).astype(np.int64)) if S else []
        for j in sample:
            t, p, L = targets[int(s["target"][j])], int(s["start"][j]), int(s["length"][j])
            piece = t[p:p + L]
            exp = sorted([(x, 0) for x in _find_all(ref, piece)] + [(len(ref) - x - L, 1) for x in _find_all(rc_ref, piece)])
            assert int(s["count"][j]) == len(exp) >= 1, (j, s[j], len(exp))
            if len(exp) <= a.max_hits:
                mine = f[int(o[j]):int(o[j + 1])]
                assert [(int(x["position"]), int(x["is_rc"])) for x in mine] == exp, j
            for longer in ([t[p - 1:p + L]] if p else []) + ([t[p:p + L + 1]] if p + L < len(t) else []):
                assert ref.find(longer) < 0 and rc_ref.find(longer) < 0, (j, "extends")
        say(f"seeds {S} ({S / k:.2f} per target), mean length {float(s['length'].mean()) if S else 0:.1f}, largest count "
            f"{int(s['count'].max()) if S else 0}, hits reported {T}; both routes agree on every seed, count and hit; a sample of "
            f"{len(sample)} seeds equals bytes.find and extends neither way")
        t_seeds, t_today = [], []
        for _ in range(a.reps):
            t_seeds.append(timed(seeds)[0])
            t_today.append(today())
        med_seeds = statistics.median(t_seeds)
        steps = [statistics.median(x[i] for x in t_today) for i in range(4)]
        med_today = statistics.median(sum(x) for x in t_today)
        say(f"seeds            median {med_seeds:9.1f} ms   {['%.1f' % t for t in t_seeds]}   {n / med_seeds / 1e3:.1f} M positions/s")
        say(f"codes -> locate  median {med_today:9.1f} ms   {['%.1f' % sum(x) for x in t_today]}")
        say(f"  its steps (medians): codes {steps[0]:.1f} ms, selection in numpy {steps[1]:.1f} ms, substrings cut and marshalled "
            f"{steps[2]:.1f} ms, locate {steps[3]:.1f} ms; the two library calls alone {steps[0] + steps[3]:.1f} ms")
        say(f"ratio: seeds takes {med_seeds / med_today:.3f} of the three-step route, {med_seeds / (steps[0] + steps[3]):.3f} of its "
            f"two library calls alone")

        native.profile_enable(True)
        try:
            native.profile_reset()
            t, _ = timed(seeds)
            rep = native.profile_report()
        finally:
            native.profile_enable(False)
            native.profile_reset()
        say(f"stage table of one seeds call (wall {t:.1f} ms with the profiler on; nested scopes are listed too)")
        say(f"  {'stage':24s} {'launches':>8s} {'ms':>9s} {'GB/s':>8s}")
        for name, (launches, ms_, nbytes) in sorted(rep.items(), key=lambda kv: -kv[1][1]):
            gbs = f"{nbytes / (ms_ * 1e-3) / 1e9:8.0f}" if nbytes and ms_ else " " * 8
            say(f"  {name:24s} {launches:8d} {ms_:9.3f} {gbs}")
    ix.close()
    say()
    say("no counter run was made")
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
