"""Texts and CPU-side references for tests/test_gpu_factor_blocks.py (the factor look-ups over rank blocks,
nolzss_amd/csrc/rank_blocks.hpp), and the interval census of tools/factor_rank_census.py.  No GPU here."""
import numpy as np

import gen
import oracle_lib as oracle

BLOCK = 16           # ranks per block
LDS_TILE = 1024      # ranks per workgroup of the candidate kernel (nearest_lds.hpp: kLdsTile)
FIELDS = ("start", "length", "ref")
PLANT = "ACGTTGCATGCA"                    # the planted 12-mer
PLANT_COUNTS = (3, 14, 18, 40, 100)


def as_bytes(a) -> bytes:
    return np.ascontiguousarray(a).tobytes()


def true_arrays(t: bytes):
    """sa (n), isa (n), lcp (n + 1: lcp[0] = lcp[n] = 0, lcp[r] = lcp of the suffixes of rank r - 1 and r) as int64"""
    n = len(t)
    sa = oracle.suffix_array(t).astype(np.int64)
    lcp = np.zeros(n + 1, dtype=np.int64)
    lcp[:n] = oracle.lcp_array(t, sa)
    lcp[0] = 0
    isa = np.empty(n, dtype=np.int64)
    isa[sa] = np.arange(n)
    return sa, isa, lcp


def interval(lcp, r, L):
    """[lo, hi]: the ranks around r whose suffixes share L symbols, as factor_kernel's scans find them"""
    lo, hi = r, r + 1
    while lcp[lo] >= L:
        lo -= 1
    while lcp[hi] >= L:
        hi += 1
    return lo, hi - 1


def blocks_touched(lo, hi):
    """aligned 16-rank blocks that hold the entries lo .. hi + 1 (both stops included)"""
    return ((hi + 1) // BLOCK) - (lo // BLOCK) + 1


def census(t: bytes, factors):
    """(interval widths, blocks touched, block lines the look-up reads, 1 if it needs no pyramid) of the factors that
    are no literals; the look-up reads the block of the rank and the neighbour on each side that the interval leaves
    it, and needs a pyramid when the interval leaves a neighbour too"""
    sa, isa, lcp = true_arrays(t)
    widths, blocks, lines, covered = [], [], [], []
    for s, L, ref in zip(factors["start"].tolist(), factors["length"].tolist(), factors["ref"].tolist()):
        if L == 1 and ref == s:
            continue
        lo, hi = interval(lcp, int(isa[s]), L)
        widths.append(hi - lo + 1)
        blocks.append(blocks_touched(lo, hi))
        b = int(isa[s]) // BLOCK
        lines.append(1 + (lo // BLOCK < b) + ((hi + 1) // BLOCK > b))
        covered.append(int(lo // BLOCK >= b - 1 and (hi + 1) // BLOCK <= b + 1))
    return tuple(np.array(x, dtype=np.int64) for x in (widths, blocks, lines, covered))


def expected_positions(t: bytes, positions=None):
    """the record of every position (or of `positions`): length from the oracle's L*, ref = the leftmost occurrence by
    brute force, a literal as (i, 1, i) -- the rule of tests/test_gpu_chain_outputs.py / factor_kernel"""
    ln, _ = oracle.lpnf_all(t)
    idx = np.arange(len(t)) if positions is None else np.asarray(positions)
    out = np.zeros(len(idx), dtype=[(f, "<u8") for f in FIELDS])
    for k, i in enumerate(idx.tolist()):
        L = int(ln[i])
        out[k] = (i, 1, i) if L == 0 else (i, L, t.find(t[i:i + L]))
    return out


def planted_text(count: int) -> bytes:
    """8192 random bases with the 12-mer written `count` times at distinct, non-overlapping places"""
    rng = np.random.default_rng(0xB10C + count)
    t = bytearray(as_bytes(gen.random_dna(8192, seed=0xB10C00 + count)))
    slots = rng.choice(8192 // 16 - 1, size=count, replace=False)
    for s in sorted(slots.tolist()):
        t[16 * s + 2:16 * s + 2 + len(PLANT)] = PLANT.encode()
    return bytes(t)


def two_copies(p_sub: float) -> bytes:
    a = gen.random_dna(4096, seed=0x2C0B)
    b = a.copy()
    if p_sub > 0:
        rng = np.random.default_rng(0x2C0C)
        at = np.flatnonzero(rng.random(4096) < p_sub)
        b[at] = gen.ACGT[(np.searchsorted(gen.ACGT, b[at]) + rng.integers(1, 4, size=len(at))) % 4]
    return as_bytes(np.concatenate([a, b]))


def make_texts():
    texts = {}
    for n in (1, 15, 16, 17, 31, 32, 33, 47, 48, 49, 255, 256, 257, LDS_TILE - 1, LDS_TILE, LDS_TILE + 1):
        texts[f"random{n}"] = as_bytes(gen.random_dna(n, seed=0xF00 + n))
    texts["run300"] = b"A" * 300
    texts["run5000"] = b"A" * 5000
    texts["period2"] = b"AC" * 2048
    texts["period5"] = b"ACGTT" * 819 + b"A"
    for c in PLANT_COUNTS:
        texts[f"plant{c}"] = planted_text(c)
    texts["copies_exact"] = two_copies(0.0)
    texts["copies_1pct"] = two_copies(0.01)
    return texts


BIG = "repeat65536"


def big_text() -> bytes:
    return as_bytes(gen.repeat_dna(2 ** 16, seed=0x5EED0003))


def big_sample(n: int):
    """a fixed-seed sample of 4096 positions plus the first and the last 64"""
    rng = np.random.default_rng(0x5A3B1E)
    return np.unique(np.concatenate([np.arange(64), np.arange(n - 64, n), rng.choice(n, size=4096, replace=False)]))
