#!/usr/bin/env python3
"""Relative-LZ index: colinear seed chains of reads and contigs, measured beside the seeds call they start from.

    python tools/rlz_index_seed_chains_probe.py [--lg 24] [--lgreads 18] [--lgcontigs 12] [--reps 5]
                                                [--out profiles/r14_rlz_index_seed_chains.txt]

Input: the reference and the two target sets of tools/rlz_index_seeds_probe.py -- 2^lg random bases, reverse complement
on; 2^lgreads reads of 150 bases at 1 % substitutions, 2^lgcontigs contigs of 10 000 bases at 0.1 %.
Measured per set on arguments that are marshalled once, alternating, medians of `reps` after a warm-up of both:
  - seed_chains: the C ABI call nolzss_rlz_index_seed_chains (min_length 20, max_hits 64, the other parameters at the
    defaults of RlzIndex.seed_chains), its result freed;
  - seeds: nolzss_rlz_index_seeds with the same min_length and max_hits, its result freed -- the floor of the route a
    user takes without seed_chains: grouping, sorting and chaining the hits on the host comes on top of it.
Then the bytes either call brings down, the stage table (nolzss_profile_report) of one seed_chains call with the share
of the chain stages, the sizes of the reported chains, and a sample of 48 primary chains whose every anchor is compared
with bytes.find on its strand.  Runs on the GPU machine only.  No counter run is made.
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
from rlz_index_seeds_probe import cuts  # noqa: E402
from rlz_probe import _COMP, timed  # noqa: E402

CHAIN_STAGES = ("rlz_chain_hit_total", "rlz_chain_keys", "rlz_chain_sort", "rlz_chain_gather", "rlz_chain_heads",
                "rlz_chain_recurrence", "rlz_chain_offsets", "rlz_chain_backtrack", "rlz_chain_primary")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lg", type=int, default=24)
    ap.add_argument("--lgreads", type=int, default=18)
    ap.add_argument("--lgcontigs", type=int, default=12)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--min-length", type=int, default=20)
    ap.add_argument("--max-hits", type=int, default=64)
    ap.add_argument("--max-gap", type=int, default=5000)
    ap.add_argument("--bandwidth", type=int, default=500)
    ap.add_argument("--min-score", type=int, default=40)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "r14_rlz_index_seed_chains.txt"))
    a = ap.parse_args()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    lib = _lib.lib
    native.set_device(0)
    ref_arr = gen.random_dna(1 << a.lg, 0x524C5A)
    ref = ref_arr.tobytes()
    comp = bytes.maketrans(b"ACGT", b"TGCA")
    say(f"relative-LZ index seed chains probe: reference 2^{a.lg} bases, reverse complement on, min_length {a.min_length}, "
        f"max_hits {a.max_hits}, max_gap {a.max_gap}, bandwidth {a.bandwidth}, min_score {a.min_score}")
    t_open, ix = timed(lambda: native.RlzIndexHandle.open(ref, with_rc=True))
    say(f"open: {t_open:.1f} ms, handle {ix.info['device_bytes'] / 2**20:.0f} MiB, P = {ix.info['prefix_syms']}")
    h = ix._handle()
    params = native._chain_params(a.min_length, a.max_hits, a.max_gap, a.bandwidth, a.min_score)

    sets = (("reads", 1 << a.lgreads, 150, 0.01, 1), ("contigs", 1 << a.lgcontigs, 10_000, 0.001, 2))
    for label, k, length, rate, seed in sets:
        rows = cuts(ref_arr, k, length, rate, seed)
        targets = [row.tobytes() for row in rows]
        args = native._seq_args(targets, "target")  # marshalled once: both calls start from these arguments
        n = k * (length + 1)

        def chains(keep=False):
            res = _lib.RlzSeedChainsResult()
            try:
                _lib.check(lib.nolzss_rlz_index_seed_chains(h, *args, C.byref(params), C.byref(res)))
                counts = (res.num_chains, res.num_anchors, res.num_seeds, res.num_seed_hits)
                return (counts,) + native._unpack_seed_chains(res) if keep else counts
            finally:
                lib.nolzss_free_rlz_seed_chains_result(C.byref(res))

        def seeds():
            res = _lib.RlzSeedsResult()
            try:
                _lib.check(lib.nolzss_rlz_index_seeds(h, *args, a.min_length, a.max_hits, C.byref(res)))
                return res.num_seeds, res.num_hits
            finally:
                lib.nolzss_free_rlz_seeds_result(C.byref(res))

        say()
        say(f"---- {label}: {k} targets of {length} bases, substitution rate {rate} ({n} batch positions)")
        (nc, na, ns, nh), c, o, an = chains(keep=True)  # warm-up of both calls
        S, T = seeds()
        assert (S, T) == (ns, nh), "the two calls see the same seeds and hits"
        prim = c[c["primary"] == 1]
        placed = len(np.unique(c["target"]))
        say(f"seeds {S}, hits expanded {T}; chains {nc} ({nc / k:.2f} per target) with {na} anchors, targets with a chain "
            f"{placed} of {k}, primary chains {len(prim)}, mean primary score {float(prim['score'].mean()) if len(prim) else 0:.1f}")
        small = int((c["num_anchors"] < 8).sum())
        say(f"chains of fewer than 8 anchors: {small} of {nc} ({100.0 * small / max(nc, 1):.1f} %); largest chain "
            f"{int(c['num_anchors'].max()) if nc else 0} anchors (the profiler's scopes time whole kernels: the wavefront time "
            f"of small groups cannot be split off)")
        where = np.flatnonzero(c["primary"] == 1)
        sample = where[np.unique(np.linspace(0, len(where) - 1, 48).astype(np.int64))] if len(where) else []
        checked = 0
        for j in sample:
            t = targets[int(c["target"][j])]
            for q, x, L in an[int(o[j]):int(o[j + 1])].tolist():
                piece = t[q:q + L]
                needle = piece.translate(comp)[::-1] if c["is_rc"][j] else piece
                assert len(piece) == L and x in _find_all(ref, needle), (j, q, x, L)
                checked += 1
        say(f"a sample of {len(sample)} primary chains: each of their {checked} anchors is where bytes.find finds its bases")
        down_chains = 64 * nc + 8 * (nc + 1) + 24 * na
        down_seeds = 32 * S + 8 * (S + 1) + 16 * T
        say(f"bytes down: seed_chains {down_chains / 1e6:.2f} MB (chains, offsets, anchors), seeds {down_seeds / 1e6:.2f} MB "
            f"(records, offsets, hits): {down_chains / max(down_seeds, 1):.3f} of it")
        t_chains, t_seeds = [], []
        for _ in range(a.reps):
            t_chains.append(timed(chains)[0])
            t_seeds.append(timed(seeds)[0])
        med_c, med_s = statistics.median(t_chains), statistics.median(t_seeds)
        say(f"seed_chains  median {med_c:9.1f} ms   {['%.1f' % t for t in t_chains]}   {n / med_c / 1e3:.1f} M positions/s")
        say(f"seeds        median {med_s:9.1f} ms   {['%.1f' % t for t in t_seeds]}")
        say(f"ratio: seed_chains takes {med_c / med_s:.3f} of the seeds call a user would chain on the host")

        native.profile_enable(True)
        try:
            native.profile_reset()
            t, _ = timed(chains)
            rep = native.profile_report()
        finally:
            native.profile_enable(False)
            native.profile_reset()
        say(f"stage table of one seed_chains call (wall {t:.1f} ms with the profiler on; nested scopes are listed too)")
        say(f"  {'stage':24s} {'launches':>8s} {'ms':>9s} {'GB/s':>8s}")
        for name, (launches, ms_, nbytes) in sorted(rep.items(), key=lambda kv: -kv[1][1]):
            gbs = f"{nbytes / (ms_ * 1e-3) / 1e9:8.0f}" if nbytes and ms_ else " " * 8
            say(f"  {name:24s} {launches:8d} {ms_:9.3f} {gbs}")
        stages = sum(rep[s][1] for s in CHAIN_STAGES if s in rep)
        search = rep.get("rlz_index_search", (0, 0.0, 0))[1]
        whole = rep.get("rlz_index_seed_chains", (0, 0.0, 0))[1]
        say(f"the chain stages together {stages:.3f} ms: {stages / max(search, 1e-9):.3f} of rlz_index_search ({search:.3f} ms), "
            f"{stages / max(whole, 1e-9):.3f} of the call's device span ({whole:.3f} ms)")
    ix.close()
    say()
    say("no counter run was made")
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
