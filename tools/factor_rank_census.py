#!/usr/bin/env python3
"""Census of the factor intervals on the benchmark generator (CPU, true SA / LCP from the oracle): per factor that is
no literal, the interval width hi - lo + 1 and the number of aligned 16-rank blocks that hold [lo, hi + 1] -- what a
look-up over rank blocks (nolzss_amd/csrc/rank_blocks.hpp) has to read.  Usage: tools/factor_rank_census.py [log2 n ...]"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
import gen  # noqa: E402
import oracle_lib as oracle  # noqa: E402
import rank_block_cases as rb  # noqa: E402


def main():
    for lg in [int(a) for a in sys.argv[1:]] or [18, 20]:
        t = rb.as_bytes(gen.repeat_dna(2 ** lg, seed=0x5EED0003))
        f = oracle.factors_array(t)
        widths, blocks, lines, covered = rb.census(t, f)
        z = len(widths)
        print(f"repeat_dna(2^{lg}): {len(f)} factors, {z} with a reference; mean length {len(t) / len(f):.1f}")
        edges = [1, 2, 3, 4, 5, 9, 17, 33, 49, 129, 1 << 62]
        print("  width      " + "  ".join(f"{a}" if b == a + 1 else (f"{a}-{b - 1}" if b < 1 << 62 else f">={a}")
                                          for a, b in zip(edges, edges[1:])))
        print("  share %    " + "  ".join(f"{100.0 * np.count_nonzero((widths >= a) & (widths < b)) / z:.1f}"
                                          for a, b in zip(edges, edges[1:])))
        for k in (1, 2, 3):
            print(f"  interval inside {k} block(s): {100.0 * np.count_nonzero(blocks <= k) / z:.1f} %")
        print(f"  look-up: {lines.mean():.2f} block lines per factor; {100.0 * covered.mean():.1f} % of the factors need no pyramid")


if __name__ == "__main__":
    main()
