#!/usr/bin/env python3
"""Times the shuffled-control significance path (nolzss_amd.genomics.significance) on one GPU.

    python tools/significance_probe.py [--log2n 24 30] [--reps 3] [--composed]

For every size (BASELINE's generator: tests/gen.py repeat_dna, seed 0x5EED0003) and mode (plain, rc): wall time of
the real call (histogram + lengths in factor order, one pipeline run), of the shuffled call (keyed shuffle +
histogram), and of shuffled_control_significance end to end (both calls + the statistics); medians over --reps after
one warm-up.  Then one profiled run of each call: the stage table (nolzss_profile_report), which names the shuffle,
the histogram kernel (length_hist) and the lengths emit (length_emit).
--composed (2^24 only): the path without these calls -- factorize into tuples for the text and its shuffle, lengths
from the tuples, and the reference's O(U N) loops for S0 / S0_upper -- for comparison.
"""
import argparse
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import gen  # noqa: E402
from nolzss_amd import _noLZSS as native  # noqa: E402
from nolzss_amd.genomics import significance as sig  # noqa: E402


def timed(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), min(ts), max(ts)


def stages(fn):
    native.profile_enable(True)
    native.profile_reset()
    t0 = time.perf_counter()
    fn()
    wall = (time.perf_counter() - t0) * 1e3
    rep = native.profile_report()
    native.profile_enable(False)
    return rep, wall


def composed(text, seed, with_rc):
    """the path the reference's functions take: tuples for both texts, then O(U N) statistics"""
    shuf = native.shuffle_dna(text, seed)
    t0 = time.perf_counter()
    fz = native.factorize_dna_w_rc if with_rc else native.factorize
    real_f, shuf_f = fz(text), fz(shuf)
    t1 = time.perf_counter()
    real_l, shuf_l = sig.extract_factor_lengths(real_f), sig.extract_factor_lengths(shuf_f)
    uniq = np.unique(shuf_l)
    n = len(shuf_l)
    S0 = np.array([np.sum(shuf_l >= L) / n for L in uniq])
    S0U = np.array([sig.clopper_pearson_upper(int(np.sum(shuf_l >= L)), n) for L in uniq])
    np.interp(real_l, uniq, S0, left=1.0, right=0.0)
    t2 = time.perf_counter()
    return (t1 - t0) * 1e3, (t2 - t1) * 1e3, len(uniq), S0U


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, nargs="+", default=[24, 30])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--composed", action="store_true")
    args = ap.parse_args()
    seed = 0x51515151
    for lg in args.log2n:
        text = gen.repeat_dna(1 << lg, seed=0x5EED0003).tobytes()
        for with_rc in (False, True):
            mode = "rc" if with_rc else "plain"
            real = timed(lambda: native.factor_length_histogram_with_lengths(text, with_rc=with_rc), args.reps)
            shuf = timed(lambda: native.factor_length_histogram(text, with_rc=with_rc, shuffle_seed=seed), args.reps)
            e2e = timed(lambda: sig.shuffled_control_significance(text, with_rc=with_rc, seed=seed), args.reps)
            r = sig.shuffled_control_significance(text, with_rc=with_rc, seed=seed)
            print(f"n=2^{lg} {mode}: real call {real[0]:.1f} ms ({real[1]:.1f}-{real[2]:.1f}), shuffled call "
                  f"{shuf[0]:.1f} ms ({shuf[1]:.1f}-{shuf[2]:.1f}), end to end {e2e[0]:.1f} ms "
                  f"({e2e[1]:.1f}-{e2e[2]:.1f}); N_real={r['N_real']} N_shuf={r['N_shuf']} L_star={r['L_star']} "
                  f"unique shuffled lengths={len(r['uniq_L'])}", flush=True)
            for name, fn in (("real", lambda: native.factor_length_histogram_with_lengths(text, with_rc=with_rc)),
                             ("shuffled", lambda: native.factor_length_histogram(text, with_rc=with_rc,
                                                                                 shuffle_seed=seed))):
                rep, wall = stages(fn)
                keys = [k for k in ("text_h2d", "shuffle", "length_pipeline", "length_hist", "length_emit",
                                    "lengths_d2h") if k in rep]
                top = sorted(rep.items(), key=lambda kv: -kv[1][1])[:12]
                # stream time of the upload, the shuffle, the pipeline and the downloads; the rest of the call's wall
                # time is host work outside those scopes (argument buffers, result structs, numpy views)
                timed_ms = sum(rep[k][1] for k in ("text_h2d", "shuffle", "length_pipeline", "lengths_d2h") if k in rep)
                print(f"  stages ({name} call, wall {wall:.1f} ms, outside the scopes {wall - timed_ms:.1f} ms): "
                      + ", ".join(f"{k} {rep[k][1]:.2f} ms" for k in keys), flush=True)
                print("    " + "; ".join(f"{k} {v[1]:.1f}" for k, v in top), flush=True)
            rh = native.factor_length_histogram_with_lengths(text, with_rc=with_rc)
            sh = native.factor_length_histogram(text, with_rc=with_rc, shuffle_seed=seed)
            st = timed(lambda: sig._from_hists(rh, sh, seed, with_rc, 1.0, 0.05), args.reps)
            print(f"  statistics on the host (both histograms given): {st[0]:.1f} ms ({st[1]:.1f}-{st[2]:.1f})",
                  flush=True)
            if args.composed and lg <= 24:
                fac_ms, stat_ms, U, _ = composed(text, seed, with_rc)
                print(f"  composed path: factorize to tuples x2 {fac_ms:.1f} ms, lengths + O(U N) statistics "
                      f"{stat_ms:.1f} ms (U={U})", flush=True)


if __name__ == "__main__":
    sys.exit(main())
