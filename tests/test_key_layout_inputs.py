"""(no GPU) The inputs of key_layout_cases.py hold what test_gpu_key_layouts.py sends them through the device for: every
planted longest common prefix is exact (naive comparison), the alphabet has the intended size and symbol width, the padding
byte is the smallest present, every (L, bit kind) combination is there, and the tied count the key layout must leave
(the model of key_layout_cases.tied_after_key_sort) is nonzero where pairs were planted at L >= k_syms."""
import numpy as np
import pytest

import key_layout_cases as K
import oracle_lib as oracle

SINGLE_ROWS = ["general8", "general4", "general2", "dna_fast", "key16", "fused"]


def test_layout_table():
    """(bits, k_syms, window, cap) of every row, as DESIGN section 5 lists them"""
    got = {name: tuple(K.layout(name))[1:] for name in K.KEY_TABLE}
    assert got["general2"] == got["dna_fast"] == got["segmented"] == (2, 17, 128, 1041)
    assert got["general4"] == (4, 15, 64, 527) and got["general8"] == (8, 7, 32, 263)
    assert got["key16"] == got["fused"] == (2, 16, 128, 1040)
    assert got["independent"] == got["independent_mirrored"] == (2, 12, 128, 1036) and got["rec_fast"] == (2, 14, 128, 1038)
    for name in K.KEY_TABLE:
        lay = K.layout(name, 4)
        assert lay.cap == lay.k_syms + lay.window  # NOLZSS_REFINE_WORDS=4: the cap on the first window edge
        assert {lay.cap - 1, lay.cap, lay.cap + 1} <= set(K.boundary_lengths(K.layout(name)))


@pytest.mark.parametrize("row", SINGLE_ROWS)
def test_single_texts(row):
    # (the prepared strings of the dna_fast and key16 rows: test_prepared_strings)
    cases = [c for c in K.cases_of(row) if c.kind == "text" and not K.classify(c.data)[2]]
    lay = cases[0].lay
    want_bits = lay.bits
    kinds, end_lengths, sizes, run_tails = set(), set(), set(), set()
    for c in cases:
        t = c.data
        sigma, bits, segmented = K.classify(t)
        assert bits == want_bits and not segmented, (c.name, sigma, bits)
        if "sigma" in c.name:
            assert sigma == int(c.name.rsplit("sigma", 1)[1]), c.name
        for p, q, L, kind in c.plants:
            assert K.naive_lcp(t, p, q) == L, (c.name, p, q, L)
            if kind == "end":
                assert q + L == len(t)  # the shorter suffix is a prefix of the longer one
                end_lengths.add(L)
            else:
                kinds.add((L, kind))
        codes, lim = K.text_view(t)
        m = K.tied_after_key_sort(codes, lim, bits, lay.k_syms)
        if any(L >= lay.k_syms for _, _, L, _ in c.plants):
            assert m > 0, c.name
        # the model from the other side: a suffix is tied iff it shares k_syms symbols with a neighbour in suffix order
        sa = oracle.suffix_array(t)
        assert m == K.tied_at_depth(oracle.lcp_array(t, sa), lay.k_syms), c.name
        if "padding_run" in c.name:
            a = np.frombuffer(t, dtype=np.uint8)
            pad = int(a.min())
            assert K.dense_codes(t)[a == pad].max() == 0  # the padding byte is the smallest present
            tail = len(a) - (np.flatnonzero(a != pad)[-1] + 1)
            run_tails.add(tail)
            sizes.add(len(t))
    lengths = K.boundary_lengths(lay)
    assert kinds >= {(L, kind) for L in lengths for kind in ("low", "high")}, sorted(kinds)
    assert end_lengths == set(lengths)
    k, w = lay.k_syms, lay.window
    assert {k - 1, k, k + 1, w - 1, w, w + 1} <= run_tails | {0}
    assert {k - 1, k, k + 1} <= run_tails
    if row != "fused":  # (the fused sort starts at 32 bases)
        assert {64, 65, 4097} <= sizes and (want_bits == 8 or {32, 33} <= sizes)
    assert max(len(c.data) for c in cases) <= 300_000


def test_key16_edges():
    """texts of the key16 rows that the 16-base key does not take, named for what keeps them out"""
    plans = {c.name: c.plan for c in K.cases_of("key16")}
    assert set(plans.values()) == {"key16", "dna_fast"}
    assert plans["key16_no_rc_three_edges_16_17"] == "key16" and plans["key16_no_rc_three_edge_15"] == "dna_fast"
    assert plans["key16_rc_one_of_31"] == "key16" and plans["key16_rc_one_of_30"] == "dna_fast"
    assert plans["key16_no_rc_four_shared"] == "key16" and plans["key16_rc_four_shared"] == "dna_fast"
    assert plans["key16_rc_one_planted"] == "key16" and plans["key16_no_rc_two_planted_shared"] == "key16"
    for c in K.cases_of("key16"):
        if c.kind == "text" and len(c.data) < 32:
            assert c.plan == "dna_fast"


def test_prepared_strings():
    """the segmented forms: the restated prepared string equals the oracle's, every sequence set has the terminator table it
    is named for, and the shared suffixes are tied only through the terminators"""
    lay = K.layout("segmented")
    sets = K.sequence_sets(lay)
    counts = {name: len(seqs) for name, (seqs, _) in sets.items()}
    assert {1, 2, 3, 4, 5, 32, 33, 64, 65, 70} == set(counts.values())
    # more equal short suffixes than a wavefront has lanes (the regroup kernel sees only the key of the element behind lane 63)
    tails = K.prepare_no_rc(*sets["seventy_shared_tails"])
    for L in range(1, 11):
        assert tails.count(b"GATTACAGAT"[-L:] + b"\x01") == 1 and sum(
            tails[p - L:p] == b"GATTACAGAT"[-L:] for p in range(len(tails)) if tails[p] not in K.NUCLEOTIDES) == 70
    for name, (seqs, trailing) in sets.items():
        if len(seqs) <= 33:
            S, orig, sent = oracle.prepare_multiple_dna_w_rc(seqs)
            assert K.prepare_rc(seqs) == S, name
            assert K.classify(S) == (4, 2, True)
        T = K.prepare_no_rc(seqs, trailing)
        a = np.frombuffer(T, dtype=np.uint8)
        sentinels = a[~np.isin(a, K.NUCLEOTIDES)]
        assert len(sentinels) == len(seqs) - (0 if trailing else 1) and len(set(sentinels.tolist())) == len(sentinels)
        assert K.classify(T) == (4, 2, True), name
        # the 64-sentinel rule: the first 64 sentinels lie below 'A' and rise with their index
        assert bool((sentinels < ord("A")).all()) == (len(sentinels) <= 64), name
    assert [len(s) for s in sets["three_edges_16_17"][0]][1:] == [16, 17] and len(sets["three_edge_15"][0][1]) == 15
    # short terminator tables (nfew): 2, 3 and 4 entries with the end of the text
    for name, entries in (("two_shared", 2), ("three_edges_16_17", 3), ("four_shared", 4)):
        T = K.prepare_no_rc(*sets[name])
        assert int((~np.isin(np.frombuffer(T, dtype=np.uint8), K.NUCLEOTIDES)).sum()) + 1 == entries
    k = lay.k_syms
    for L in (k - 1, k, k + 1):
        a, b = K.shared_suffix_pair(L, 800 + L)
        assert a[-L:] == b[-L:] and a[-L - 1] != b[-L - 1]
    planted = 0
    for row in ("segmented", "dna_fast", "key16"):
        for c in K.cases_of(row):
            S = K.prepare_rc(c.data) if c.kind == "prepared_rc" else c.data
            if not K.classify(S)[2]:
                continue
            codes, lim = K.text_view(S)
            m = K.tied_after_key_sort(codes, lim, 2, c.lay.k_syms)
            sa = oracle.suffix_array(S)
            assert m == K.tied_at_depth(oracle.lcp_array(S, sa), c.lay.k_syms), c.name
            if "planted" in c.name:
                assert m > 0
                planted += 1
    assert planted >= 6


@pytest.mark.parametrize("row", ["independent", "independent_mirrored", "rec_fast"])
def test_batch_records(row):
    (case,) = K.cases_of(row)
    lay, recs = case.lay, case.data
    k = lay.k_syms
    for p, q, L, kind in case.plants:
        assert K.naive_lcp(recs[0], p, q) == L
    assert {(L, kind) for _, _, L, kind in case.plants} == {(L, kind) for L in K.boundary_lengths(lay) for kind in ("low", "high")}
    for j, L in enumerate(K.short_lengths(lay)):
        r = recs[1 + j]
        assert K.naive_lcp(r, 4 + 9, len(r) - L) == L  # the record ends L symbols into a copy
    # one block in two different records: it ties in the text, and must not tie in the batch
    first = 1 + len(K.short_lengths(lay))
    for j, L in enumerate((k - 1, k, k + 1, k + lay.window)):
        a, b = recs[first + 2 * j], recs[first + 2 * j + 1]
        assert a[30:30 + L] == b[25:25 + L] and a[30 + L] != b[25 + L]
    assert all(set(bytes(r)) <= set(b"ACGT") for r in recs)
    m = K.batch_model(recs, lay)
    assert m > 0
    # the same suffixes without the record number in the key tie more often
    joined = K.prepare_no_rc(recs, True)
    codes, lim = K.text_view(joined)
    assert K.tied_after_key_sort(codes, lim, 2, k) > m
    assert sum(len(r) for r in recs) <= 300_000
