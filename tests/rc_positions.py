"""Reverse-complement mode checked at EVERY position of the original strand -- TEST INFRASTRUCTURE ONLY (a plain helper
module: the GPU tests of test_gpu_rc_positions.py import it in process, their child processes run its main(), and
test_rc_positions_inputs.py checks on the CPU that the inputs below hold what those tests claim to cover).

rc_tile_kernel, rc_far_kernel, rc_fallback_kernel and factor_kernel<true, ..> write a code / can write a record for
every position i < N of a prepared string; a factorization only ever reads the ones on its greedy chain.  The checker
takes all of them through the debug hook (nolzss_debug_rc_arrays) and compares them with the oracle's answer at
every position (oracle_lpnf_all_rc), together with the suffix array, LCP array and inverse suffix array of S.
"""
import functools
import json
import random
import sys
from pathlib import Path

import numpy as np

import gen
import oracle_lib as oracle

KATS = json.loads((Path(__file__).parent / "golden" / "kats.json").read_text())
LEN_MASK = 0x7FFFFFFF
NUCLEOTIDES = (65, 67, 71, 84)


# ---- inputs ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def family_300():
    """300 copies of one 300-mer, each with one position set to 'A'"""
    a = gen.random_dna(5000, 1)[:300]
    rng = np.random.default_rng(3)
    out = []
    for _ in range(300):
        b = a.copy()
        b[rng.integers(0, 300, 1)] = ord("A")
        out.append(b.tobytes())
    return out


def _mixed_50k():
    rng = random.Random(77)  # (the text test_gpu_rc.py calls mixed_50k: second draw of that generator)
    gen.mixed_dna(rng, 2000)
    return gen.mixed_dna(rng, 50_000, maxlen=300).encode()


def _self_complementary_unit(half, seed):
    """V rc(V) for a random V of `half` bases: a repeat unit that is its own reverse complement"""
    v = gen.random_dna(half, seed).tobytes()
    return v + v[::-1].translate(bytes.maketrans(b"ACGT", b"TGCA"))


@functools.lru_cache(maxsize=None)
def cases_single():
    """4(a): one sequence each; name -> [sequence]"""
    return {
        "AT_x3000": [b"AT" * 3000],
        "A_x6000": [b"A" * 6000],
        "CT_x10000": [b"CT" * 10000],
        "copies_40_of_1500": [gen.random_dna(1500, 1).tobytes() * 40],
        "family_300_joined": [b"".join(family_300())],
        "period_300_x40": [np.tile(gen.random_dna(5000, 1)[:300], 40).tobytes()],
        "repeat_200k": [gen.repeat_dna(200_000, 22, lo=16, hi=4096).tobytes()],
        "far_copy_150k": [gen.far_copy(150_000, 10)],
        "ACAG_tandem": [(b"ACAG" * 300 + b"AGAGAT") * 3],
        "palindromic": [b"ACGT" * 700 + b"TTAA" * 200],
        "CCCT_G_CCCT": [b"CCCT" * 5000 + b"G" + b"CCCT" * 5000],
        "mixed_50k": [_mixed_50k()],
        "GC_x5000": [b"GC" * 5000],
        "ACGT_x2500": [b"ACGT" * 2500],
        "selfrc_500_x40": [_self_complementary_unit(250, 9) * 40],
        "selfrc_300_x60": [_self_complementary_unit(150, 9) * 60],
    }


# nearly every position takes the exact forward search ...
PERIODIC = ("A_x6000", "CT_x10000", "CCCT_G_CCCT", "AT_x3000", "GC_x5000", "ACGT_x2500")
# ... and is queued for it by rc_tile_kernel itself.  The texts above reach the exact search through rc_far_kernel:
# where no reverse-complement suffix qualifies (A, CT, CCCT) more than kListCap ranks of a wavefront are still
# searching after four steps (overflowing_wavefronts) and a rank that finds its list full restarts from global memory;
# where a short period is its own reverse complement (AT, GC, ACGT) all suffixes of one phase share one long run of
# ranks, and the qualifying reverse-complement suffix of a position in the first half of the text lies further than
# the tile's reach of 256 ranks up that run.  A long unit V rc(V) repeated k times keeps both away: the 2 k suffixes of
# one phase (both strands, interleaved by length) fit the reach, and no work list overflows.
PERIODIC_IN_TILES = ("selfrc_500_x40", "selfrc_300_x60")


@functools.lru_cache(maxsize=None)
def cases_multi():
    """4(b): several sequences in one prepared string"""
    return {
        "family_120_sequences": family_300()[:120],  # 240 sentinels: the device's order is not the byte order
        "family_9_sequences": family_300()[:9],
        "tiny_sequences_x4": [b"A", b"A", b"AA", b"AAA", b"C", b"CA", b"AAAA"] * 4,
    }


TILE_SIZES = (1, 2, 3, 6, 7, 8, 127, 128, 255, 256, 383, 510, 511, 512, 639, 1022, 1023, 1024, 1535, 2047, 2048, 4095,
              4096, 32767, 32768)
RUN_SIZES = (511, 512, 1023, 1024)


@functools.lru_cache(maxsize=None)
def cases_sizes():
    """4(c): around the tile geometry (1024 ranks per tile, 256 per wavefront, reach 256, pyramid blocks of 16,
    m = 2 N + 2)"""
    c = {f"repeat_{n}": [gen.repeat_dna(n, 40 + n % 7, lo=8, hi=512).tobytes()] for n in TILE_SIZES}
    c.update({f"A_x{n}": [b"A" * n] for n in RUN_SIZES})
    return c


@functools.lru_cache(maxsize=None)
def cases_kats():
    """4(d): the known answers of the reference, and the example its documentation gets wrong"""
    c = {"kat_" + v["input"]: [v["input"].encode()] for v in KATS["dna_w_rc"] + KATS["derived_dna_w_rc"]}
    c["kat_doc_example"] = [KATS["reference_doc_example_contradicted_by_the_code"][0]["input"].encode()]
    return c


def all_cases(kats=True):
    c = {}
    for part in (cases_single(), cases_multi(), cases_sizes()) + ((cases_kats(),) if kats else ()):
        c.update(part)
    return c


# ---- the oracle's side, computed once per input ---------------------------------------------------------------------
class Expected:
    def __init__(self, seqs):
        self.S, self.orig, self.sent = oracle.prepare_multiple_dna_w_rc(list(seqs))
        S = self.S
        self.m = len(S)
        self.N = self.m // 2 - 1
        self.bytes = np.frombuffer(S, dtype=np.uint8)
        self.sa = oracle.suffix_array(S).astype(np.int64)
        self.lcp = oracle.lcp_array(S, self.sa).astype(np.int64)
        self.ln, self.rf = oracle.lpnf_all_rc(S)
        self.plain_ln, self.plain_rf = (a[:self.N] for a in oracle.lpnf_all(S))
        sentinels = self.bytes[~np.isin(self.bytes, NUCLEOTIDES)]
        # every sentinel below 'A': byte order is the device's order (text.hpp: a terminator is smaller than every
        # nucleotide, and of two terminators the one with the lower index; the sentinel bytes 1, 2, .. rise with the
        # index up to the 64th, the first to land above 'A')
        self.byte_order = bool((sentinels < ord("A")).all())
        for a in (self.sa, self.lcp, self.ln, self.rf, self.plain_ln, self.plain_rf, self.bytes):
            a.setflags(write=False)

    @functools.cached_property
    def isa(self):
        isa = np.empty(self.m, dtype=np.int64)
        isa[self.sa] = np.arange(self.m)
        return isa

    def chain(self, start=0):
        """positions the greedy cursor visits from `start`"""
        out, p = [], start
        ln = self.ln
        while p < self.N:
            out.append(p)
            p += int(ln[p])
        return np.array(out, dtype=np.int64)


@functools.lru_cache(maxsize=None)
def expected(name):
    return Expected(all_cases()[name])


# ---- the checker -----------------------------------------------------------------------------------------------------
def _same(what, got, exp, isa, counters):
    """integer equality of two arrays indexed by text position; the first mismatch, its rank and the counters if not"""
    got, exp = np.asarray(got), np.asarray(exp)
    assert got.shape == exp.shape, (what, got.shape, exp.shape)
    bad = np.flatnonzero(got != exp)
    if bad.size:
        i = int(bad[0])
        rank = int(isa[i]) if isa is not None and i < len(isa) else None
        raise AssertionError(f"{what}: {bad.size} mismatches, first at position {i} (rank {rank}): device {got[i]!r}, "
                             f"expected {exp[i]!r}; counters {counters}")


def _lcp_of_pairs(text, is_term, a, b):
    """common prefix of the suffixes a[k] and b[k], cut at the nearer sentinel"""
    m = len(text)
    l = np.zeros(len(a), dtype=np.int64)
    live = np.arange(len(a))
    while live.size:
        x, y = a[live] + l[live], b[live] + l[live]
        ok = (x < m) & (y < m)
        xs, ys = np.minimum(x, m - 1), np.minimum(y, m - 1)
        ok &= ~is_term[xs] & ~is_term[ys] & (text[xs] == text[ys])
        live = live[ok]
        l[live] += 1
    return l


def _check_suffix_order_by_rule(e, sa, lcp, counters):
    """more than 64 sentinels: the device sorts every terminator in front of the nucleotides and terminators by
    index, the byte values do not -- the arrays are checked against that rule itself"""
    m, text = e.m, e.bytes
    assert np.array_equal(np.sort(sa), np.arange(m)), f"suffix array is no permutation; counters {counters}"
    is_term = ~np.isin(text, NUCLEOTIDES)
    a, b = sa[:-1], sa[1:]
    l = _lcp_of_pairs(text, is_term, a, b)
    _same("LCP (suffix pairs compared in the text)", lcp[1:m], l, None, counters)
    assert lcp[0] == 0
    # the order itself: behind the common prefix the upper suffix has its terminator (the lower index of two),
    # or the smaller nucleotide
    x, y = a + l, b + l
    assert (x < m).all() and (y < m).all()
    tx, ty = is_term[x], is_term[y]
    good = np.where(tx, ~ty | (x < y), ~ty & (text[x] < text[y]))
    bad = np.flatnonzero(~good)
    assert bad.size == 0, f"suffix order: ranks {int(bad[0])}, {int(bad[0]) + 1} are out of order; counters {counters}"


def check_every_position(native, seqs, want_plain, e=None):
    """Every array of the reverse-complement pipeline over the prepared string of `seqs` against the oracle, with
    integer equality.  Returns (N, counters of the run)."""
    seqs = list(seqs)
    if e is None:
        e = Expected(seqs)
    S, N, m = e.S, e.N, e.m
    S_dev, orig_dev, sent_dev = native.prepare_multiple_dna_sequences_w_rc_bytes(seqs)
    assert (bytes(S_dev), orig_dev, list(sent_dev)) == (S, e.orig, list(e.sent)), "prepared string"

    d = native.debug_rc_arrays(S, want_plain=want_plain)
    counters = d["counters"]
    sa, lcp, isa = d["sa"].astype(np.int64), d["lcp"].astype(np.int64), d["isa"].astype(np.int64)
    assert len(sa) == m and len(lcp) == m + 1 and len(isa) == N and len(d["code"]) == N and len(d["records"]) == N

    # suffix array, LCP, inverse suffix array
    if e.byte_order:
        _same("suffix array", sa, e.sa, None, counters)
        _same("LCP", lcp[:m], e.lcp, None, counters)
    else:
        _check_suffix_order_by_rule(e, sa, lcp, counters)
    assert lcp[m] == 0, f"LCP[m] = {lcp[m]}; counters {counters}"
    inv = np.empty(m, dtype=np.int64)
    inv[sa] = np.arange(m)
    _same("inverse suffix array", isa, inv[:N], None, counters)

    # codes
    code = d["code"].astype(np.int64)
    length = code & LEN_MASK
    is_lit = (e.rf == np.arange(N, dtype=np.uint64)) & (e.ln == 1)  # (no flag: the flag bit would make ref != i)
    _same("code: length", np.where(length == 0, 1, length), e.ln.astype(np.int64), isa, counters)
    _same("code: reverse-complement flag", code >> 31, (e.rf >> np.uint64(63)).astype(np.int64), isa, counters)
    _same("code: literal", length == 0, is_lit, isa, counters)

    # records
    rec = d["records"]
    _same("record: start", rec["start"], np.arange(N, dtype=np.uint64), isa, counters)
    _same("record: length", rec["length"], e.ln.astype(np.uint64), isa, counters)
    _same("record: ref", rec["ref"], e.rf, isa, counters)

    # the plain-mode by-product, and the codes of the run that makes it
    if want_plain:
        plain = d["plain"].astype(np.int64)
        _same("plain by-product", np.where(plain == 0, 1, plain), e.plain_ln.astype(np.int64), isa, counters)
        _same("plain by-product: literal", plain == 0,
              (e.plain_rf.astype(np.int64) == np.arange(N)) & (e.plain_ln == 1), isa, counters)
        d0 = native.debug_rc_arrays(S, want_plain=False)
        _same("codes with and without the plain by-product", d["code"], d0["code"], isa, counters)
        assert d0["counters"] == counters, (d0["counters"], counters)

    # the chain over the records is what the product path emits
    for sp in sorted({0, N // 3, N - 1 - N // 7}):
        got = native.factorize_multiple_dna_w_rc_array(S, start_pos=sp)
        walk, p = [], sp
        while p < N:
            walk.append(p)
            p += int(rec["length"][p])
        exp = rec[np.array(walk, dtype=np.int64)]
        assert len(got) == len(exp), f"chain from {sp}: {len(got)} factors, records give {len(exp)}; counters {counters}"
        for k in ("start", "length", "ref"):
            _same(f"chain from {sp}: {k}", got[k], exp[k], None, counters)
    return N, counters


# ---- input conditions, from the oracle alone (test_rc_positions_inputs.py) -------------------------------------------
def _range_min_table(v):
    t = [np.asarray(v, dtype=np.int64)]
    k = 1
    while 2 * k <= len(v):
        p = t[-1]
        t.append(np.minimum(p[:-k], p[k:]))
        k *= 2
    return t


def _range_min(t, lo, hi):
    """min v[lo..hi] (inclusive, lo <= hi), vectorised"""
    k = np.floor(np.log2(hi - lo + 1)).astype(np.int64)
    out = np.empty(len(lo), dtype=np.int64)
    for level in np.unique(k):
        sel = k == level
        out[sel] = np.minimum(t[level][lo[sel]], t[level][hi[sel] - (1 << level) + 1])
    return out


def _nearest_smaller(sa):
    """rank of the nearest suffix above / below every rank that starts earlier in the text (-1 / m: none)"""
    m = len(sa)
    up, down = np.full(m, -1, dtype=np.int64), np.full(m, m, dtype=np.int64)
    v = sa.tolist()
    stack = []
    for r in range(m):
        while stack and v[stack[-1]] > v[r]:
            down[stack.pop()] = r
        if stack:
            up[r] = stack[-1]
        stack.append(r)
    return up, down


def exact_search_positions(e):
    """positions i < N whose forward match rc_decide reports as not final (fwd_final false): the longer of the two
    nearest earlier suffixes overlaps position i"""
    m, N, sa = e.m, e.N, e.sa
    lcpx = np.append(e.lcp, 0)  # lcp[m] = 0
    t = _range_min_table(lcpx)
    up, down = _nearest_smaller(sa)
    r = np.flatnonzero(sa < N)
    i = sa[r]
    has_up, has_down = up[r] >= 0, down[r] < m
    lp = np.where(has_up, _range_min(t, np.where(has_up, up[r] + 1, r), r), 0)
    ls = np.where(has_down, _range_min(t, r + 1, np.where(has_down, down[r], r + 1)), 0)
    jp = sa[np.maximum(up[r], 0)]
    js = sa[np.minimum(down[r], m - 1)]
    M = np.maximum(lp, ls)
    final = (M == 0) | ((lp == M) & (i - jp >= M)) | ((ls == M) & (i - js >= M))
    return np.sort(i[~final])


def quirk_positions(e):
    """positions where the emitted forward factor is shorter than the plain-mode L* over S: the explicit-node rule of
    the reference (d_u in rc_fallback_kernel).  Positions where the reverse complement wins do not show their forward
    candidate in the oracle's answer and are not counted: a lower bound."""
    fwd = (e.rf >> np.uint64(63)) == 0
    return np.flatnonzero(fwd & (e.ln < e.plain_ln))


def quirk_at(e, i):
    """the same for one position, whichever strand wins there (tests/array_model.py restates the rule)"""
    import array_model as am
    Lf = am.lstar_plain(e.sa, e.isa, np.append(e.lcp, 0), e.m, i)
    if Lf == 0:
        return False
    lcp = np.append(e.lcp, 0)
    a, b = am._interval(lcp, e.m, e.isa[i], Lf + 1)
    d_u = max(lcp[a], lcp[b + 1] if b + 1 < e.m else 0)
    a, b = am._interval(lcp, e.m, e.isa[i], d_u)
    j = int(e.sa[a:b + 1].min())
    return min(am._range_lcp(lcp, e.isa, i, j), i - j) < Lf


def rc_chosen_positions(e):
    return np.flatnonzero((e.rf >> np.uint64(63)) == 1)


def overflowing_wavefronts(e, steps=4, group=256, cap=128):
    """Model of the work lists of rc_tile_kernel (kListCap = 128 entries per wavefront and kind of search): per
    aligned group of 256 ranks and per search (forward up / down, reverse complement up / down), the ranks of the
    original strand that have neither found a qualifying suffix nor driven their LCP minimum to 0 after four steps.
    Returns the number of (group, search) lists that hold more than 128."""
    m, N, sa = e.m, e.N, e.sa
    lcpx = np.append(e.lcp, 0)
    r = np.flatnonzero(sa < N)
    i = sa[r]
    over = 0
    for rc in (False, True):
        for step in (-1, 1):
            live = np.ones(len(r), dtype=bool)
            run = np.full(len(r), np.iinfo(np.int64).max)
            for k in range(1, steps + 1):
                q = r + step * k
                inside = (q >= 0) & (q < m)
                qc = np.clip(q, 0, m - 1)
                # the LCP entry crossed by this step: lcp[q + 1] going up, lcp[q] going down
                edge = np.where(inside, lcpx[np.clip(qc + 1 if step < 0 else qc, 0, m)], 0)
                run = np.minimum(run, edge)
                hit = (sa[qc] > 2 * N - i) if rc else (sa[qc] < i)
                live &= (run > 0) & ~(inside & hit)
            counts = np.bincount(r[live] // group, minlength=(m + group - 1) // group)
            over += int((counts > cap).sum())
    return over


# ---- child processes of test_every_position_paths ---------------------------------------------------------------------
def main():
    sys.path.insert(0, str(Path(__file__).resolve().parent.parent))  # (run as a script: the package sits beside tests/)
    from nolzss_amd import _noLZSS as native
    assert native.device_count() >= 1, "no MI355X visible"
    report = {}
    for name, seqs in all_cases(kats=False).items():
        N, counters = check_every_position(native, seqs, True, expected(name))
        report[name] = dict(counters, N=N)
    total = {k: sum(c[k] for c in report.values()) for k in native.RC_COUNTERS}
    print("COUNTERS " + json.dumps(report))
    print("TOTAL " + json.dumps(total))
    print("ok")


if __name__ == "__main__":
    sys.exit(main())
