"""The model of the LDS sub-bucket sort (tests/local_sort_model.py) without a GPU: the regroup model against a pure-Python
brute force on the symbol strings the keys encode and against tied_after_key_sort() of key_layout_cases.py, the emulation
of the kernel's ranking and store against the reference, and the inputs of tests/test_gpu_local_sort.py against the
mistakes they are there to see -- for every mistake a named case whose expected output differs."""
import numpy as np
import pytest

import key_layout_cases as K
import local_sort_model as M


# ---- keys by definition ------------------------------------------------------------------------------------------------------
def pairs_of_text(codes, form):
    """What the most-significant-digit pass of the key sorts makes of a plain 2-bit text (Text16Src / Text35Src,
    radix_sort.hip): element e < 16 is suffix n - 1 - e, the others suffix e - 16; the key is the zero-padded window of
    16 bases (35 bits), its first byte the bucket, the rest the stored word above the tag min(n - s, full); the pass is
    stable.  -> words, suffixes, bucket starts"""
    n = len(codes)
    bits = 32 if form is M.KEY16 else 35
    suffix = np.concatenate([n - 1 - np.arange(16), np.arange(n - 16)])
    padded = np.concatenate([np.asarray(codes, dtype=np.int64), np.zeros(18, dtype=np.int64)])
    win = np.zeros(n, dtype=np.int64)
    for j in range(18):
        win = (win << 2) | padded[suffix + j]
    key = win >> (36 - bits)
    tag = np.minimum(n - suffix, form.tag_full)
    bucket = key >> (bits - 8)
    words = ((key & ((1 << (bits - 8)) - 1)) << form.shift0) | tag
    order = np.argsort(bucket, kind="stable")
    starts = np.concatenate([[0], np.cumsum(np.bincount(bucket, minlength=256))])
    return words[order].astype(np.uint32), suffix[order].astype(np.uint32), starts.astype(np.uint32)


def brute_force_regroup(codes, form):
    """the same on the symbol strings, element by element: order, heads, LCPs, tied list"""
    n, full = len(codes), form.tag_full
    codes = [int(c) for c in codes]
    suffixes = [n - 1 - e for e in range(16)] + list(range(n - 16))

    def sort_key(s):
        sym = (codes[s:s + 18] + [0] * 18)[:18]
        return tuple(sym[:16]) if form is M.KEY16 else tuple(sym[:17]) + (sym[17] >> 1,)

    order = sorted(suffixes, key=sort_key)  # (stable)
    lim = [n - s for s in order]
    keys = [sort_key(s) for s in order]
    head, lcp = [], []
    for p in range(n):
        if p == 0:
            head.append(True)
            lcp.append(0)
            continue
        h = lim[p] < full or lim[p - 1] < full or keys[p] != keys[p - 1]
        head.append(h)
        common = 0
        while common < full and keys[p][common] == keys[p - 1][common]:
            common += 1
        lcp.append(min(common, lim[p], lim[p - 1], full) if h else M.PENDING)
    slot, grp, last_head = [], [], 0
    for p in range(n):
        if head[p]:
            last_head = p
        if not (head[p] and (p + 1 == n or head[p + 1])):
            slot.append(p)
            grp.append(last_head)
    return order, lcp, slot, grp


def pin_texts():
    rng = np.random.default_rng(5)
    out = []
    for k in (0, 1, 5, 15, 16, 17, 18, 25):
        block = rng.integers(0, 4, size=37)
        t = np.concatenate([block, block, rng.integers(0, 4, size=9), block[:30], np.zeros(21, dtype=np.int64), rng.integers(1, 4, size=3),
                            block[5:], rng.integers(1, 4, size=1), np.zeros(k, dtype=np.int64)])
        out.append(t)
    out.append(rng.integers(0, 4, size=32))
    out.append(np.zeros(60, dtype=np.int64))
    out.append(np.tile(np.array([0, 1, 2, 3]), 40))
    return out


@pytest.mark.parametrize("form", [M.KEY16, M.KEY35], ids=lambda f: f.name)
def test_the_regroup_model_matches_a_brute_force_on_symbol_strings(form):
    tied = short_in_front = 0
    for codes in pin_texts():
        words, suffix, starts = pairs_of_text(codes, form)
        sw, sv = M.stable_sort(words, suffix, starts, form.shift0)
        lcp, slot, grp, head = M.regroup(sw, M.bucket_of(starts), form)
        order, b_lcp, b_slot, b_grp = brute_force_regroup(codes, form)
        assert sv.tolist() == order
        assert lcp.tolist() == b_lcp
        assert slot.tolist() == b_slot and grp.tolist() == b_grp
        tied += len(slot)
        tag = sw & ((1 << form.shift0) - 1)
        short_in_front += int(((tag[:-1] < form.tag_full) & ((sw[1:] >> form.shift0) == (sw[:-1] >> form.shift0))).sum())
    assert tied > 500 and short_in_front > 20  # (short suffixes in front of longer ones with the same padded key occur)


def test_the_regroup_model_matches_the_tied_counts_of_the_key_layout_cases():
    texts = [c.data for c in K.cases_of("key16") if c.kind == "text" and c.plan == "key16" and not K.classify(c.data)[2]]
    picked = texts[:3] + texts[-6:]
    assert len(picked) == 9
    seen = 0
    for t in picked:
        codes, lim = K.text_view(t)
        words, suffix, starts = pairs_of_text(codes, M.KEY16)
        sw, _ = M.stable_sort(words, suffix, starts, 8)
        _, slot, _, _ = M.regroup(sw, M.bucket_of(starts), M.KEY16)
        assert len(slot) == K.tied_after_key_sort(codes, lim, 2, 16), len(t)
        seen += len(slot)
    assert seen > 0


# ---- the emulation of the kernel -----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def case_sets():
    return {(f.name, fused): {c.name: c for c in M.all_cases(f, fused)}
            for f in (M.KEY16, M.KEY35, M.RECORDS) for fused in ((False, True) if f is not M.RECORDS else (False,))}


def sub_bucket(case, label):
    first, count = case.subs[label]
    return case.words[first:first + count], np.arange(first, first + count, dtype=np.uint32), first, count


def reference_of_sub(words, values, form):
    order = np.argsort(words.astype(np.int64) >> form.shift0, kind="stable")
    return words[order], values[order]


def test_the_emulated_kernel_is_a_stable_sort(case_sets):
    """every labelled sub-bucket of the pattern and bin cases (they lie in sub-bucket order) through the emulation"""
    checked = 0
    for form in (M.KEY16, M.KEY35, M.RECORDS):
        cs = case_sets[(form.name, False)]
        names = [n for n in cs if n.startswith("patterns_d") and not n.endswith("shuffled")] + ["all_ones"] + (["key35_bins"] if form.key35 else [])
        for name in names:
            for label, (first, count) in cs[name].subs.items():
                if count > 5000 and not (form is M.KEY16 and name == "patterns_d0"):
                    continue  # (the large ones once)
                w, v, _, _ = sub_bucket(cs[name], label)
                ew, ev = M.emulate_sub_bucket(w, v, form)
                rw, rv = reference_of_sub(w, v, form)
                assert np.array_equal(ev, rv) and np.array_equal(ew, rw), (form.name, name, label)
                checked += 1
    assert checked > 300


def test_the_store_covers_every_sub_bucket_exactly_once():
    for first in range(4):
        for count in list(range(1, 40)) + [767, 768, 769, 4607, 18431, 18432]:
            assert M.store_written(first, count).all(), (first, count)


# ---- every mistake is seen by a named case -------------------------------------------------------------------------------------
def emulated_differs(case, label, form, mistake, only_pass=None):
    w, v, _, _ = sub_bucket(case, label)
    assert np.array_equal(M.emulate_sub_bucket(w, v, form)[1], reference_of_sub(w, v, form)[1])
    return not np.array_equal(M.emulate_sub_bucket(w, v, form, mistake, only_pass)[1], reference_of_sub(w, v, form)[1])


@pytest.mark.parametrize("form", [M.KEY16, M.KEY35, M.RECORDS], ids=lambda f: f.name)
def test_lanes_served_in_another_order_on_later_rows_are_seen(case_sets, form):
    """row 0 meets no contention (64 different digits: the kernel's own check of row 0 passes whatever the order), every
    later row has all 64 lanes on one counter"""
    cs = case_sets[(form.name, False)]
    for j in range(len(form.widths)):
        case = cs[f"patterns_d{j}"]
        for size in (1537, 4609, 17665):
            assert emulated_differs(case, f"row0_distinct_then_one/{size}", form, "lanes_reversed_rows_ge_1", j), (j, size)
        w, _, _, _ = sub_bucket(case, "row0_distinct_then_one/1537")
        shift = form.shift0 + sum(form.widths[:j])
        wave, row, lane = M.places(len(w))
        d = (w.astype(np.int64) >> shift) & ((1 << form.widths[j]) - 1)
        row0 = [d[(wave == k) & (row == 0)].tolist() for k in range(12)]
        assert all(len(set(x)) == len(x) for x in row0) and sum(len(x) == 64 for x in row0) >= 8
        assert len(set(d[row >= 1].tolist())) == 1


@pytest.mark.parametrize("form", [M.KEY16, M.KEY35, M.RECORDS], ids=lambda f: f.name)
def test_pads_ranked_as_key_zero_are_seen(case_sets, form):
    cs = case_sets[(form.name, False)]
    assert emulated_differs(cs["sizes"], "size769", form, "pads_zero")
    assert emulated_differs(cs["sizes"], "size17665", form, "pads_zero")
    assert emulated_differs(cs["all_ones"], "ones1000", form, "pads_zero")
    # the words of all ones lie in a partial last row and sort to the very end, in front of the pad keys
    if form is not M.RECORDS:
        w, _, first, count = sub_bucket(cs["all_ones"], "ones769")
        assert count % M.THREADS and int((w == 0xffffffff).sum()) > 100
        assert first + count == len(cs["all_ones"].words)


def test_a_dropped_head_or_tail_of_an_unaligned_store_is_seen(case_sets):
    for key in case_sets:
        case = case_sets[key]["residues"]
        seen = set()
        for label, (first, count) in case.subs.items():
            assert label == f"size{count}@{first % 4}"
            seen.add((count, first % 4))
        assert seen == {(c, r) for c in range(1, 16) for r in range(4)}
        assert len(case.words) % 4 != 0
        first, count = case.subs["size2@1"]   # inside one quad: all of it is the head
        assert not M.store_written(first, count, "head_dropped").any() and M.store_written(first, count, "tail_dropped").all()
        first, count = case.subs["size2@3"]   # across a quad edge: one element of head, one of tail
        assert M.store_written(first, count, "head_dropped").tolist() == [False, True]
        assert M.store_written(first, count, "tail_dropped").tolist() == [True, False]
        for r in (1, 2, 3):
            first, count = case.subs[f"size15@{r}"]
            assert not M.store_written(first, count, "head_dropped").all()
        # the last sub-bucket of `sizes` ends at n, which is no multiple of 4: a tail
        sizes = case_sets[key]["sizes"]
        first, count = sizes.subs["last"]
        assert first + count == len(sizes.words) and (first + count) % 4 != 0
        assert not M.store_written(first, count, "tail_dropped").all()


def test_the_bin_of_a_two_bin_owner_off_by_one_is_seen(case_sets):
    case = case_sets[("key35", False)]["key35_bins"]
    assert emulated_differs(case, "bins1537/10", M.KEY35, "two_bin_owner")
    assert emulated_differs(case, "bins4609/11", M.KEY35, "two_bin_owner")
    w, _, _, _ = sub_bucket(case, "bins1537/11")
    assert set(((w >> 5) & 1023).tolist()) == set(M.KEY35_BINS0) and set(((w >> 15) & 511).tolist()) == set(M.KEY35_BINS1)


def test_capacity_off_by_one_is_seen(case_sets):
    for key in case_sets:
        case = case_sets[key]["capacity_edge"]
        assert M.listed_count(case.words, case.starts) == 1
        assert M.listed_count(case.words, case.starts, M.CAP - 1) == 2 and M.listed_count(case.words, case.starts, M.CAP + 1) == 0
        over = case_sets[key]["overflow"]
        assert M.listed_count(over.words, over.starts) == 5
        sizes = M.sub_sizes(over.words, over.starts)
        big = np.flatnonzero(sizes > M.CAP)
        assert 40000 in sizes[big] and (np.diff(big) == 1).any()                      # ten tiles; two neighbours
        lone = [s for s in big if 0 < sizes[s - 1] <= M.CAP and 0 < sizes[s + 1] <= M.CAP]
        assert lone                                                                   # one between two that fit


@pytest.mark.parametrize("form", [M.KEY16, M.KEY35, M.RECORDS], ids=lambda f: f.name)
def test_low_bits_in_the_order_and_an_ignored_top_digit_are_seen(case_sets, form):
    for name in ("sizes", "turns", "random_shuffled"):
        case = case_sets[(form.name, False)][name]
        values = np.arange(len(case.words), dtype=np.uint32)
        ref = M.stable_sort(case.words, values, case.starts, form.shift0)[1]
        if form.shift0:
            assert not np.array_equal(M.stable_sort(case.words, values, case.starts, form.shift0, "low_bits")[1], ref)
        assert not np.array_equal(M.stable_sort(case.words, values, case.starts, form.shift0, "no_top_digit", form)[1], ref)


@pytest.mark.parametrize("form", [M.KEY16, M.KEY35], ids=lambda f: f.name)
def test_the_regroup_mistakes_are_seen(case_sets, form):
    cs = case_sets[(form.name, True)]

    def outputs(case, variant=None):
        sw, _ = M.stable_sort(case.words, np.arange(len(case.words), dtype=np.uint32), case.starts, form.shift0)
        return M.regroup(sw, M.bucket_of(case.starts), form, variant)

    places = cs["fused_places"]
    ref = outputs(places)
    one_tag = outputs(places, "lcp_one_tag")
    assert not np.array_equal(one_tag[0], ref[0])                              # an LCP capped by one tag only
    kept = outputs(places, "short_kept")
    assert len(kept[1]) != len(ref[1])                                         # a short-tag element kept as tied
    byte = cs["fused_bucket_byte"]
    assert not np.array_equal(outputs(byte, "no_bucket_byte")[0], outputs(byte)[0])   # the first boundary without the bucket byte
    # .. in every bit of the bucket byte and of the sub-bucket's byte: LCPs 0 .. 7 from them
    assert set(outputs(byte)[0].tolist()) >= set(range(8))


@pytest.mark.parametrize("form", [M.KEY16, M.KEY35], ids=lambda f: f.name)
def test_the_fused_inputs_hold_what_they_are_there_for(case_sets, form):
    case = case_sets[(form.name, True)]["fused_places"]
    full, tb = form.tag_full, form.shift0
    sw, _ = M.stable_sort(case.words, np.arange(len(case.words), dtype=np.uint32), case.starts, tb)
    lcp, slot, grp, head = M.regroup(sw, M.bucket_of(case.starts), form)
    tied = np.zeros(len(sw), dtype=bool)
    tied[slot] = True
    tag = sw.astype(np.int64) & ((1 << tb) - 1)

    def at(label, place):
        first, count = case.subs[label]
        return first + (place if place >= 0 else count + place)

    # ties that stay tied at the first place, the last place and across a 64-place edge (63 | 64, 127 | 128, 767 | 768)
    for place in (0, 1, -1, -2, 63, 64, 127, 128, 767, 768):
        assert tied[at("ties", place)], place
    for place in (64, 128, 768, 1536):
        assert not head[at("ties", place)], place
    # short tags inside runs of equal keys at the same places: heads, not tied, and so is whoever follows
    for place in (0, 63, 64, 127, 128, 767, 768, 1535, 1536):
        p = at("short_in_runs", place)
        assert tag[p] < full and head[p] and (p + 1 == len(sw) or head[p + 1]), place
        assert (sw[p] >> tb) == (sw[p - 1] >> tb) or (sw[p] >> tb) == (sw[p + 1] >> tb)
    # a sub-bucket that is one group, one that is all heads
    for label in ("one_group_769", "one_group_65"):
        first, count = case.subs[label]
        assert head[first] and not head[first + 1:first + count].any() and tied[first:first + count].all()
    first, count = case.subs["all_heads"]
    assert head[first:first + count].all() and not tied[first:first + count].any()
    # boundaries decided by the key bits at every depth, and by the tag
    first, count = case.subs["key_bit_depths"]
    assert set(lcp[first + 1:first + count].tolist()) >= set(range(8, full))
    first, count = case.subs["tag_decides"]
    seg = slice(first + 1, first + count)
    untagged = ((sw.astype(np.int64) >> tb) << tb | full).astype(np.uint32)  # the same keys, every tag full: what the key bits share
    shared = M.regroup(untagged, M.bucket_of(case.starts), form)[0]
    assert (shared[seg] != M.PENDING).all()
    by_tag = lcp[seg] < shared[seg]
    assert by_tag.sum() > 10 and (lcp[seg][by_tag] == np.minimum(tag[seg], tag[first:first + count - 1])[by_tag]).all()
    assert (~by_tag).sum() > 3
