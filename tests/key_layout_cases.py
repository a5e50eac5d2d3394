"""Inputs built around the constants of every round-0 key layout (plan_keys, suffix_array.hip; table in DESIGN section 5)
-- TEST INFRASTRUCTURE ONLY.  A plain helper module: test_key_layout_inputs.py proves on the CPU that every input holds the
boundary it is named for, test_gpu_key_layouts.py sends the inputs through the device, and its child processes run main().

A layout is (bits per symbol, k_syms, window W of the first direct round, cap of that round).  Around each of them:
pairs of suffixes whose longest common prefix is exactly L, texts that end L symbols into a copy of an earlier block, texts
that end in runs of the padding symbol, and the same with a sentinel in place of the end of the text.

tied_after_key_sort() is the model of what the key sort must leave tied: with lim(i) the distance from i to its next
terminator (or to the end of the text), a suffix with lim(i) < k_syms carries its own length in the key (and on segmented
keys its terminator index) or is made a group of its own by the regroup kernel; the others tie exactly when their first
k_syms symbols are equal (and, in a batch, they lie in the same record).
"""
import functools
import os
import pickle
import re
import sys
from collections import namedtuple
from pathlib import Path

import numpy as np

NUCLEOTIDES = (65, 67, 71, 84)
ACGT = b"ACGT"
REFINE_WINDOW_WORDS = 4  # kRefineWords: 64-bit words of text per round of the direct round

Layout = namedtuple("Layout", "name bits k_syms window cap")

# name of the plan's choice -> (bits per symbol, symbols in the key)
KEY_TABLE = {
    "general8": (8, 7), "general4": (4, 15), "general2": (2, 17), "dna_fast": (2, 17), "key16": (2, 16), "fused": (2, 16),
    "segmented": (2, 17), "independent": (2, 12), "independent_mirrored": (2, 12), "rec_fast": (2, 14),
}


def layout(name, refine_words=32):
    bits, k = KEY_TABLE[name]
    return Layout(name, bits, k, REFINE_WINDOW_WORDS * 64 // bits, k + refine_words * 64 // bits)


def plan_k_syms(plan, bits):
    """symbols in the key of a plan as the trace names it ("general" has one width per symbol size)"""
    return {2: 17, 4: 15, 8: 7}[bits] if plan == "general" else KEY_TABLE[plan][1]


def boundary_lengths(lay, refine_words=32):
    """the LCPs at which a layout can go wrong: around the key width, around the first window edge, the second window edge,
    around the cap of the direct round"""
    k, w = lay.k_syms, lay.window
    cap = k + refine_words * 64 // lay.bits
    return sorted({k - 1, k, k + 1, k + w - 1, k + w, k + w + 1, k + 2 * w, cap - 1, cap, cap + 1})


def short_lengths(lay):
    k, w = lay.k_syms, lay.window
    return [k - 1, k, k + 1, k + w - 1, k + w, k + w + 1]


def naive_lcp(t, p, q):
    t = np.frombuffer(t, dtype=np.uint8) if isinstance(t, (bytes, bytearray)) else t
    m = min(len(t) - p, len(t) - q)
    d = np.nonzero(t[p:p + m] != t[q:q + m])[0]
    return int(d[0]) if len(d) else m


# ---- what the device makes of a text (text_pack.hip) ---------------------------------------------------------------------
def classify(t):
    """-> (sigma, bits, segmented) as pack_text decides them"""
    a = np.frombuffer(t, dtype=np.uint8)
    counts = np.bincount(a, minlength=256)
    sigma = int((counts > 0).sum())
    bits = 2 if sigma <= 4 else (4 if sigma <= 16 else 8)
    other = np.ones(256, dtype=bool)
    other[list(NUCLEOTIDES)] = False
    others = int(((counts > 0) & other).sum())
    nucleotides = int((counts[list(NUCLEOTIDES)] > 0).sum())
    segmented = 1 <= others <= 250 and nucleotides >= 1 and int(counts[other].sum()) == others
    return (4, 2, True) if segmented else (sigma, bits, False)


def dense_codes(t):
    """the rank of every byte among the byte values present: the device's order-preserving symbol codes"""
    a = np.frombuffer(t, dtype=np.uint8)
    present = np.bincount(a, minlength=256) > 0
    return (np.cumsum(present) - 1)[a].astype(np.int64)


def text_view(t):
    """-> (codes, lim) of a single text: segmented texts code their nucleotides 0 .. 3 and stop at every other byte"""
    a = np.frombuffer(t, dtype=np.uint8)
    n = len(a)
    if classify(t)[2]:
        code = np.zeros(256, dtype=np.int64)
        for k, c in enumerate(NUCLEOTIDES):
            code[c] = k
        is_term = ~np.isin(a, NUCLEOTIDES)
        codes = np.where(is_term, 0, code[a])
    else:
        is_term = np.zeros(n, dtype=bool)
        codes = dense_codes(t)
    return codes, limits(is_term)


def limits(is_term):
    """distance from every position to its next terminator or to the end of the text"""
    n = len(is_term)
    nxt = np.where(is_term, np.arange(n), n)
    nxt = np.minimum.accumulate(nxt[::-1])[::-1] if n else nxt
    return nxt - np.arange(n)


def tied_after_key_sort(codes, lim, bits, k_syms, record=None):
    """the model (module docstring): suffixes with lim >= k_syms whose first k_syms symbols equal another such suffix's"""
    n = len(codes)
    assert k_syms * bits <= 62
    padded = np.concatenate([codes, np.zeros(k_syms, dtype=np.int64)])
    key = np.zeros(n, dtype=np.int64)
    for j in range(k_syms):
        key = (key << bits) | padded[j:j + n]
    full = lim >= k_syms
    key = key[full]
    if record is not None:
        key = np.stack([record[full], key], axis=1)
        _, inv, counts = np.unique(key, axis=0, return_inverse=True, return_counts=True)
    else:
        _, inv, counts = np.unique(key, return_inverse=True, return_counts=True)
    return int((counts[inv.reshape(-1)] > 1).sum())


def tied_at_depth(lcp, depth):
    """suffixes that agree with a neighbour in suffix order on at least `depth` symbols (lcp: n entries, lcp[0] = 0)"""
    l = np.asarray(lcp, dtype=np.int64)
    nxt = np.append(l[1:], 0)
    return int((np.maximum(l, nxt) >= depth).sum())


# ---- builders --------------------------------------------------------------------------------------------------------------
def _alphabet(alphabet):
    alpha = np.array(sorted(set(alphabet)), dtype=np.uint8)
    assert len(alpha) == len(alphabet)
    return alpha


def planted_pairs_text(alphabet, lay, lengths, seed):
    """Random text over `alphabet` (written once in front, so every symbol is present) with, for every L of `lengths`, two
    pairs of copies of a random block of L symbols: behind one pair the symbols differ only in the LOWEST bit of their
    dense code, behind the other only in the HIGHEST bit of the symbol width (where the alphabet has no code with that bit:
    in the highest bit it has, kind "high_avail").  Returns (text, [(p, q, L, kind)])."""
    alpha = _alphabet(alphabet)
    sigma = len(alpha)
    rng = np.random.default_rng(seed)
    top = 1 << (lay.bits - 1)
    high, high_kind = (top, "high") if sigma > top else (1 << ((sigma - 1).bit_length() - 1), "high_avail")
    spots, at = [], sigma + 9
    for L in lengths:
        for bit, kind in ((1, "low"), (high, high_kind)):
            p, q = at, at + L + 8
            spots.append((p, q, L, bit, kind))
            at = q + L + 8
    n = at + 16
    t = alpha[rng.integers(0, sigma, size=n)]
    t[:sigma] = alpha
    plants = []
    for p, q, L, bit, kind in spots:
        block = alpha[rng.integers(0, sigma, size=L)]
        t[p:p + L] = block
        t[q:q + L] = block
        ok = [c for c in range(sigma) if (c ^ bit) < sigma]
        c = ok[int(rng.integers(0, len(ok)))]
        t[p + L], t[q + L] = alpha[c], alpha[c ^ bit]
        plants.append((p, q, L, kind))
    text = t.tobytes()
    # the bit patterns, from the codes the device computes: ranks among the byte values present
    codes = dense_codes(text)
    assert codes.max() == sigma - 1
    for p, q, L, kind in plants:
        x = int(codes[p + L] ^ codes[q + L])
        assert x == (1 if kind == "low" else high), (p, q, L, kind, x)
        assert kind != "high" or x == 1 << (lay.bits - 1)
    return text, plants


def end_in_copy_text(alphabet, L, seed):
    """the text ends L symbols into a copy of an earlier block: the suffix n - L is a prefix of the suffix p and sorts
    in front of it.  Returns (text, [(p, n - L, L, "end")])."""
    alpha = _alphabet(alphabet)
    sigma = len(alpha)
    rng = np.random.default_rng(seed)
    block = alpha[rng.integers(0, sigma, size=L + 5)]
    fill = lambda m: alpha[rng.integers(0, sigma, size=m)]  # noqa: E731
    t = np.concatenate([alpha, fill(9), block, fill(11), block[:L]])
    return t.tobytes(), [(sigma + 9, len(t) - L, L, "end")]


def padding_run_texts(alphabet, lay, seed):
    """texts ending in a run of k copies of the smallest byte value present (dense code 0: the zero padding behind the end
    of the text), k around k_syms and around the window, n around 32 / 64 and around 4097, with a longer run of that byte
    in the middle where there is room: the zero-padded keys and windows of the short suffixes collide with real runs"""
    alpha = _alphabet(alphabet)
    sigma = len(alpha)
    k0, w = lay.k_syms, lay.window
    out = []
    for n in (32, 33, 64, 65, 4097):
        for k in sorted({0, 1, k0 - 1, k0, k0 + 1, w - 1, w, w + 1}):
            body = n - k
            if body < sigma + 4:
                continue
            rng = np.random.default_rng(seed + 1000 * n + k)
            t = alpha[rng.integers(0, sigma, size=body)]
            t[:sigma] = alpha
            if int(t[-1]) == int(alpha[0]) and sigma > 1:
                t[-1] = alpha[1]  # the run at the end has exactly k members
            long_run = k + w + 3
            if body - sigma - 2 > long_run:
                mid = sigma + (body - sigma - long_run) // 2
                t[mid:mid + long_run] = alpha[0]
            out.append(t.tobytes() + bytes([int(alpha[0])]) * k)
    return out


def sentinel_byte(index):
    """the k-th of 1, 2, 3, .. without the nucleotides: the sentinels of the prepared strings"""
    s, count = 1, 0
    while True:
        if s not in NUCLEOTIDES:
            if count == index:
                return s
            count += 1
        s += 1


def prepare_no_rc(seqs, trailing):
    """T1 s1 T2 s2 .. Tk [sk]: the no-RC counterpart of the prepared reverse-complement string"""
    out = bytearray()
    for j, s in enumerate(seqs):
        out += bytes(s)
        if trailing or j + 1 < len(seqs):
            out.append(sentinel_byte(j))
    assert len(seqs) <= 251
    return bytes(out)


def prepare_rc(seqs):
    """T1 s0 .. Tk s(k-1) rc(Tk) sk .. rc(T1) s(2k-1): the prepared reverse-complement string (restated here so that the
    model needs no library; test_key_layout_inputs.py compares it with the oracle's)"""
    comp = bytes.maketrans(b"ACGT", b"TGCA")
    parts = [bytes(s) for s in seqs] + [bytes(s)[::-1].translate(comp) for s in reversed(seqs)]
    return b"".join(p + bytes([sentinel_byte(j)]) for j, p in enumerate(parts))


def shared_suffix_pair(L, seed):
    """two sequences that end in the same L bases behind different ones: their last L + 1 suffixes (the terminator's
    included) tie on every symbol and are ordered by the terminators"""
    rng = np.random.default_rng(seed)
    tail = np.frombuffer(ACGT, dtype=np.uint8)[rng.integers(0, 4, size=L)].tobytes()
    a = np.frombuffer(ACGT, dtype=np.uint8)[rng.integers(0, 4, size=20)].tobytes()
    b = np.frombuffer(ACGT, dtype=np.uint8)[rng.integers(0, 4, size=23)].tobytes()
    return a + b"A" + tail, b + b"C" + tail


def _dna(n, seed):
    return np.frombuffer(ACGT, dtype=np.uint8)[np.random.default_rng(seed).integers(0, 4, size=n)].tobytes()


def sequence_sets(lay):
    """name -> (sequences, trailing sentinel in the no-RC form): the planted pairs and ends of `lay` as sequences, pairs with
    a shared suffix around k_syms, sequences of 15, 16 and 17 bases (the edge of key16_applicable), in sets of 1 .. 5, 32,
    33, 64 and 65 sequences"""
    k = lay.k_syms
    big, _ = planted_pairs_text(ACGT, lay, boundary_lengths(lay), 500 + k)
    ends = [end_in_copy_text(ACGT, L, 600 + L)[0] for L in short_lengths(lay)]
    runs = [t for t in padding_run_texts(ACGT, lay, 700) if len(t) in (64, 65)][:6]
    shared = [s for L in (k - 1, k, k + 1) for s in shared_suffix_pair(L, 800 + L)]
    edge = [_dna(15, 1), _dna(16, 2), _dna(17, 3)]
    many = shared + edge + ends + runs
    while len(many) < 65:
        many.append(_dna(18 + len(many) % 29, 900 + len(many)))
    return {
        "one_planted": ([big], True),
        "one_end_in_copy": ([ends[1]], True),
        "one_of_31": ([_dna(31, 4)], True),  # (2 x 31 + 2 = 64 symbols: the smallest reverse-complement string of key16)
        "one_of_30": ([_dna(30, 5)], True),
        "two_planted_shared": ([big, shared[2]], False),
        "two_shared": ([_dna(40, 6) + shared[2][-k:], shared[3]], False),
        "three_edges_16_17": ([_dna(40, 7), edge[1], edge[2]], False),
        "three_edge_15": ([_dna(40, 8), edge[0], edge[2]], False),
        "four_shared": (shared[:4], False),
        "four_ends": (ends[:4], False),
        "five": ([big] + shared[:2] + ends[:2], True),
        "thirty_two": (many[:32], True),
        "thirty_three": (many[:33], True),
        "sixty_four": (many[:64], True),
        "sixty_five": (many[:65], True),
        # 70 short suffixes with one key, for every length up to 10: a run of equal keys longer than a wavefront, so that one
        # of them is the last lane of its wavefront in the regroup kernel whatever else the text holds
        "seventy_shared_tails": ([_dna(20 + j % 7, 1000 + j) + ACGT[j % 4:j % 4 + 1] + b"GATTACAGAT" for j in range(70)], True),
    }


def key16_applicable(t):
    """radix_sort.hip: one segment of at least 32 bases, or 2 .. 4 terminators (the end of the text included) around
    segments of at least 16 bases in a text of at least 64 symbols, whose last segment may be empty"""
    sigma, bits, segmented = classify(t)
    if bits != 2:
        return False
    if not segmented:
        return len(t) >= 32
    a = np.frombuffer(t, dtype=np.uint8)
    terms = np.flatnonzero(~np.isin(a, NUCLEOTIDES)).tolist() + [len(t)]
    if not 2 <= len(terms) <= 4 or len(t) < 64:
        return False
    start = 0
    for j, p in enumerate(terms):
        if not (p - start >= 16 or (j + 1 == len(terms) and p == start)):
            return False
        start = p + 1
    return True


# ---- the rows of the plan table --------------------------------------------------------------------------------------------
# row -> (environment that forces it on small texts, does the tied count have a model to be compared with)
ROWS = {
    "general8": ({}, True),
    "general4": ({}, True),
    "general2": ({}, True),
    "dna_fast": ({"NOLZSS_DNA_FAST_MIN": "1", "NOLZSS_NO_KEY16": "1"}, True),
    "key16": ({"NOLZSS_DNA_FAST_MIN": "1", "NOLZSS_NO_KEY35": "1"}, True),
    "key16_local": ({"NOLZSS_DNA_FAST_MIN": "1", "NOLZSS_NO_KEY35": "1", "NOLZSS_LOCAL_SORT_MIN": "1"}, True),
    "fused": ({"NOLZSS_DNA_FAST_MIN": "1", "NOLZSS_NO_KEY35": "1", "NOLZSS_FUSED_SORT": "1"}, False),
    "segmented": ({}, True),
    "independent": ({}, False),
    "independent_mirrored": ({}, False),
    "rec_fast": ({"NOLZSS_DNA_FAST_MIN": "1", "NOLZSS_REC_BUCKET_MIN": "1"}, False),
    # the cap of the direct round on the first window edge
    "general8_cap_at_window": ({"NOLZSS_REFINE_WORDS": "4"}, True),
    "general4_cap_at_window": ({"NOLZSS_REFINE_WORDS": "4"}, True),
    "key16_cap_at_window": ({"NOLZSS_DNA_FAST_MIN": "1", "NOLZSS_NO_KEY35": "1", "NOLZSS_REFINE_WORDS": "4"}, True),
    "segmented_cap_at_window": ({"NOLZSS_REFINE_WORDS": "4"}, True),
}

ALPHABETS = {
    "general8": [bytes(range(100, 117)), bytes(range(256))],
    "general4": [b"abcde", b"abcdefghijklmnop"],
    "general2": [ACGT, bytes([0, 7, 200, 255])],
}

Case = namedtuple("Case", "name kind data plan lay plants")
# kind: "text" (data = bytes), "prepared_rc" (data = sequences), "batch" / "batch_rc" (data = records)


def _single_text_cases(name, alphabets, lay, plan):
    cases = []
    for a, alphabet in enumerate(alphabets):
        t, plants = planted_pairs_text(alphabet, lay, boundary_lengths(lay), 10 * lay.k_syms + a)
        cases.append(Case(f"{name}_planted_sigma{len(alphabet)}", "text", t, plan, lay, plants))
        for L in boundary_lengths(lay):
            t, plants = end_in_copy_text(alphabet, L, 100 * lay.k_syms + L)
            cases.append(Case(f"{name}_end_in_copy_{L}_sigma{len(alphabet)}", "text", t, plan, lay, plants))
    for j, t in enumerate(padding_run_texts(alphabets[0], lay, 40)):
        cases.append(Case(f"{name}_padding_run_{j}_n{len(t)}", "text", t, plan, lay, []))
    return cases


def _prepared_cases(name, lay, plan_of):
    cases = []
    for set_name, (seqs, trailing) in sequence_sets(lay).items():
        S = prepare_no_rc(seqs, trailing)
        cases.append(Case(f"{name}_no_rc_{set_name}", "text", S, plan_of(S), lay, []))
        if len(seqs) <= 33:
            cases.append(Case(f"{name}_rc_{set_name}", "prepared_rc", [bytes(s) for s in seqs], plan_of(prepare_rc(seqs)), lay, []))
    return cases


def _batch_records(lay):
    """records with planted pairs inside one record, one block in two different records (it must not tie), records that
    end L symbols into a copy"""
    k = lay.k_syms
    big, plants = planted_pairs_text(ACGT, lay, boundary_lengths(lay), 300 + k)
    recs = [big]
    for L in short_lengths(lay):
        recs.append(end_in_copy_text(ACGT, L, 310 + L)[0])
    for L in (k - 1, k, k + 1, k + lay.window):
        block = _dna(L, 320 + L)
        recs += [_dna(30, 330 + L) + block + b"A" + _dna(9, 340 + L), _dna(25, 350 + L) + block + b"C" + _dna(14, 360 + L)]
    recs += [_dna(k - 1, 370), _dna(k, 371), _dna(k + 1, 372), b"A", b"A" * (k + 3), _dna(5000, 373)]
    return recs, plants


@functools.lru_cache(maxsize=None)
def cases_of(row):
    """every input of one row of the table, with the plan it must take"""
    base = row.replace("_cap_at_window", "").replace("_local", "")
    refine_words = 4 if row.endswith("_cap_at_window") else 32
    lay = layout(base, refine_words)
    if base in ALPHABETS:
        return _single_text_cases(base, ALPHABETS[base], lay, "general")
    if base == "fused":
        return [c for c in _single_text_cases(base, [ACGT], lay, "fused") if len(c.data) >= 32]
    if base == "dna_fast":
        cases = _single_text_cases(base, [ACGT], lay, "dna_fast")
        sets = sequence_sets(lay)
        for set_name in ("five", "sixty_four", "sixty_five", "seventy_shared_tails"):
            S = prepare_no_rc(sets[set_name][0], True)
            cases.append(Case(f"dna_fast_no_rc_{set_name}", "text", S, "dna_fast", lay, []))
        cases.append(Case("dna_fast_rc_five", "prepared_rc", [bytes(s) for s in sets["five"][0]], "dna_fast", lay, []))
        return cases
    if base == "key16":
        # (texts the 16-base key does not take -- shorter than 32 bases, a segment shorter than 16 -- sort on the 17-base key)
        plan_of = lambda S: "key16" if key16_applicable(S) else "dna_fast"  # noqa: E731
        cases = [c._replace(plan=plan_of(c.data)) for c in _single_text_cases(base, [ACGT], lay, None)]
        return cases + [c for c in _prepared_cases(base, lay, plan_of)
                        if c.name.split("_rc_")[-1].startswith(("one", "two", "three", "four"))]
    if base == "segmented":
        return _prepared_cases(base, lay, lambda S: "segmented")
    if base in ("independent", "independent_mirrored", "rec_fast"):
        recs, plants = _batch_records(lay)
        return [Case(base, "batch_rc" if base == "independent_mirrored" else "batch", recs, base, lay, plants)]
    raise KeyError(row)


def batch_model(recs, lay):
    """tied count of a batch: records side by side, ties only inside one record"""
    codes, lim, rec = [], [], []
    for j, r in enumerate(recs):
        c = dense_codes(ACGT + bytes(r))[4:]
        codes.append(np.append(c, 0))
        lim.append(np.append(np.arange(len(r), 0, -1), 0))
        rec.append(np.full(len(r) + 1, j))
    return tied_after_key_sort(np.concatenate(codes), np.concatenate(lim), 2, lay.k_syms, np.concatenate(rec))


# ---- the oracle's side -------------------------------------------------------------------------------------------------------
def expected_of(case):
    import oracle_lib as oracle
    import rc_positions
    if case.kind == "text":
        t = case.data
        sa = oracle.suffix_array(t)
        exp = oracle.factors_array(t)
        return {"sa": sa, "lcp": oracle.lcp_array(t, sa), "ln": oracle.lpnf_all(t)[0],
                "factors": {k: np.asarray(exp[k]) for k in ("start", "length", "ref")}}
    if case.kind == "prepared_rc":
        return rc_positions.Expected(case.data)
    if case.kind == "batch":
        return [oracle.factors_array(r) for r in case.data]
    return [oracle.factors_array_multiple_dna_w_rc(oracle.prepare_multiple_dna_w_rc([bytes(r)])[0]) for r in case.data]


def check_order_by_rule(t, sa, lcp):
    """Suffix array and LCP of a segmented text against the ordering rule of text.hpp, in the text itself: a comparison runs
    to the nearer terminator, the suffix that reaches its terminator first is the smaller one, and of two terminators the one
    with the lower index -- the end of the text is the LAST terminator, where the byte order has it in front of every byte."""
    import rc_positions
    a = np.frombuffer(t, dtype=np.uint8)
    m = len(a)
    assert np.array_equal(np.sort(sa), np.arange(m)), "suffix array is no permutation"
    is_term = ~np.isin(a, NUCLEOTIDES)
    p, q = sa[:-1], sa[1:]
    l = rc_positions._lcp_of_pairs(a, is_term, p, q)
    assert lcp[0] == 0 and np.array_equal(lcp[1:m], l), "LCP (suffix pairs compared in the text)"
    x, y = p + l, q + l
    xs, ys = np.minimum(x, m - 1), np.minimum(y, m - 1)
    tx, ty = (x == m) | is_term[xs], (y == m) | is_term[ys]
    good = np.where(tx, ~ty | (x < y), ~ty & (a[xs] < a[ys]))
    bad = np.flatnonzero(~good)
    assert bad.size == 0, f"suffix order: ranks {int(bad[0])}, {int(bad[0]) + 1} are out of order"


def check_case(native, case, exp):
    """one input through the device, every array against the oracle with integer equality"""
    import rc_positions
    if case.kind == "text":
        t = case.data
        n = len(t)
        d = native.debug_arrays(t)
        sa, lcp = d["sa"].astype(np.int64), d["lcp"].astype(np.int64)
        a = np.frombuffer(t, dtype=np.uint8)
        sentinels = a[~np.isin(a, NUCLEOTIDES)].astype(np.int64)
        if classify(t)[2]:
            check_order_by_rule(t, sa, lcp)
        # (the bytes order like the device's terminators only where every sentinel lies below 'A', they rise along the text --
        # up to 64 sentinels of a prepared string -- and the text ends in one: the end of the text is the last terminator)
        if not classify(t)[2] or (bool((sentinels < ord("A")).all()) and bool((np.diff(sentinels) > 0).all())
                                  and not a[-1] in NUCLEOTIDES):
            assert np.array_equal(sa, exp["sa"].astype(np.int64)), (case.name, "suffix array")
            assert np.array_equal(lcp[:n], exp["lcp"].astype(np.int64)), (case.name, "LCP")
        assert lcp[n] == 0
        inv = np.empty(n, dtype=np.int64)
        inv[sa] = np.arange(n)
        assert np.array_equal(d["isa"].astype(np.int64), inv), (case.name, "inverse suffix array")
        got = d["lstar"].astype(np.int64)
        assert np.array_equal(np.where(got == 0, 1, got), exp["ln"].astype(np.int64)), (case.name, "L*")
        f = native.factorize_array(t)
        assert len(f) == len(exp["factors"]["start"]), (case.name, "factor count")
        for k in ("start", "length", "ref"):
            assert np.array_equal(np.asarray(f[k]).astype(np.uint64), exp["factors"][k].astype(np.uint64)), (case.name, k)
    elif case.kind == "prepared_rc":
        rc_positions.check_every_position(native, case.data, True, exp)
    else:
        recs = [np.frombuffer(bytes(r), dtype=np.uint8) for r in case.data]
        m0, s0 = native.debug_batch_counters()
        counts, arrays = native.factorize_batch(recs, want_factors=True, with_rc=case.kind == "batch_rc")
        m1, s1 = native.debug_batch_counters()
        assert (m1 - m0, s1 - s0) == (len(recs), 0), (case.name, "records merged / taken one by one", m1 - m0, s1 - s0)
        for j, e in enumerate(exp):
            assert counts[j] == len(e), (case.name, j)
            for k in ("start", "length", "ref"):
                assert np.array_equal(arrays[j][k], e[k]), (case.name, j, k)


TRACE_KEY = re.compile(r"n=(\d+): (\d+) suffixes tied after the (\d+)-symbol key sort \(plan: (\w+)\)")
TRACE_DIRECT = re.compile(r"direct round \(cap (\d+) symbols\): (\d+) still tied")


def split_trace(stderr):
    """the trace of a child process, cut at the CASE markers -> {case index: text}"""
    parts = re.split(r"^CASE (\d+)\n", stderr, flags=re.M)
    return {int(parts[k]): parts[k + 1] for k in range(1, len(parts), 2)}


def run_child(cases, expected_path):
    """body of a child process: every case through the device against the pickled expectations of the parent; a CASE marker
    goes to stderr in front of every input so that the trace lines behind it can be told apart"""
    sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
    from nolzss_amd import _noLZSS as native
    assert native.device_count() >= 1, "no MI355X visible"
    with open(expected_path, "rb") as f:
        expected = pickle.load(f)
    assert len(cases) == len(expected)
    for i, (case, exp) in enumerate(zip(cases, expected)):
        os.write(2, f"CASE {i}\n".encode())
        check_case(native, case, exp)
    print("ok", len(cases))


def main():
    """child process of test_gpu_key_layouts.py: main(row, file of pickled expectations)"""
    run_child(cases_of(sys.argv[1]), sys.argv[2])


if __name__ == "__main__":
    sys.exit(main())
