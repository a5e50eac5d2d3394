"""The LDS sub-bucket sort (local_sort.hpp: local_sort_kernel, local_sort_sub_buckets) in plain numpy -- TEST
INFRASTRUCTURE ONLY.  Three things:

  * the reference: per bucket a stable sort by word >> shift0 (stable_sort), the regroup of round 0 on the sorted words
    (regroup), the number of sub-buckets beyond a workgroup (listed_count);
  * a small emulation of how the kernel ranks and stores one sub-bucket (emulate_sub_bucket, store_written) and wrong
    variants of both and of the reference, so that tests/test_local_sort_model_host.py can show that the inputs tell
    the reference apart from every mistake they are there for;
  * the inputs (cases, fused_cases): words and bucket starts for nolzss_debug_local_sort, values = arange(n).

A form is (shift0, digit widths from shift0 up, 35-bit key?, full tag): the digits end at bit 24, the byte above them is
the digit of the segmented pass in front of the kernel (256 sub-buckets per bucket).
"""
from collections import namedtuple

import numpy as np

THREADS, ROWS = 768, 24          # kLocalThreads, kLocalRows
CAP = THREADS * ROWS             # kLocalCap: 18 432 pairs
PENDING = 0xffffffff             # kLcpPending: not a group head

Form = namedtuple("Form", "name shift0 widths key35 tag_full")
KEY16 = Form("key16", 8, (8, 8), False, 16)
KEY35 = Form("key35", 5, (10, 9), True, 17)
RECORDS = Form("records", 0, (8, 8, 8), False, None)
FORMS = {f.name: f for f in (KEY16, KEY35, RECORDS)}


# ---- the reference ---------------------------------------------------------------------------------------------------------
def bucket_of(starts):
    starts = np.asarray(starts, dtype=np.int64)
    return np.repeat(np.arange(len(starts) - 1, dtype=np.int64), np.diff(starts))


def sub_of(words, starts):
    return bucket_of(starts) * 256 + (np.asarray(words, dtype=np.int64) >> 24)


def sub_sizes(words, starts):
    return np.bincount(sub_of(words, starts), minlength=256 * (len(starts) - 1))


def listed_count(words, starts, cap=CAP):
    return int((sub_sizes(words, starts) > cap).sum())


def stable_sort(words, values, starts, shift0, variant=None, form=None):
    """-> (words, values) of every bucket sorted stably by word >> shift0.  Wrong variants: "low_bits" (the bits below
    shift0 take part in the order), "no_top_digit" (the last digit below bit 24 is ignored; needs the form)."""
    w = np.asarray(words, dtype=np.int64)
    key = w >> shift0
    if variant == "low_bits":
        key = w
    elif variant == "no_top_digit":
        kept = sum(form.widths[:-1])
        key = ((w >> 24) << kept) | ((w >> shift0) & ((1 << kept) - 1))
    else:
        assert variant is None
    perm = np.lexsort((key, bucket_of(starts)))
    return np.asarray(words, dtype=np.uint32)[perm], np.asarray(values, dtype=np.uint32)[perm]


def _bit_length(x):
    return np.frexp(x.astype(np.float64))[1].astype(np.int64)  # (exact below 2^53; 0 -> 0)


def regroup(sorted_words, bucket, form, variant=None):
    """The regroup of round 0 (layouts 3 and 4) on the sorted words and the bucket each lies in.  The key of an element
    is its bucket byte followed by the stored key bits (24 or 27); the low bits of the word are its tag.
      head:  the first element, or one whose word or bucket differs from its predecessor's (so whoever follows a short
             element is a head too), or one whose tag is short (below tag_full);
      lcp of a head: min(tag, predecessor's tag, whole leading symbols the two keys share), 0 for the first element;
             of the others PENDING;
      tied:  every element that is not both a head and followed by a head (the last element is followed by one), in slot
             order, with the slot of the nearest head at or in front of it.
    -> lcp, new_slot, new_grp, head (bool).  Wrong variants: "lcp_one_tag", "short_kept", "no_bucket_byte"."""
    assert variant in (None, "lcp_one_tag", "short_kept", "no_bucket_byte")
    w = np.asarray(sorted_words, dtype=np.int64)
    b = np.asarray(bucket, dtype=np.int64)
    n = len(w)
    tag_bits, key_bits = form.shift0, 32 - form.shift0
    tag, kb = w & ((1 << tag_bits) - 1), w >> tag_bits
    assert int(tag.max()) <= form.tag_full, "the tag precondition of the form with the regroup on the way"
    key = (b << key_bits) | kb
    head = np.ones(n, dtype=bool)
    head[1:] = (w[1:] != w[:-1]) | (b[1:] != b[:-1])
    if variant != "short_kept":
        head |= tag < form.tag_full
    x = key[1:] ^ key[:-1]
    if variant == "no_bucket_byte":  # (the first place of a sub-bucket: the stored words alone)
        first_of_sub = (b[1:] * 256 + (w[1:] >> 24)) != (b[:-1] * 256 + (w[:-1] >> 24))
        x = np.where(first_of_sub, kb[1:] ^ kb[:-1], x)
    shared = (8 + key_bits - _bit_length(x)) >> 1
    cap = tag[1:] if variant == "lcp_one_tag" else np.minimum(tag[1:], tag[:-1])
    lcp = np.full(n, PENDING, dtype=np.int64)
    lcp[0] = 0
    lcp[1:] = np.where(head[1:], np.minimum(shared, cap), PENDING)
    keep = ~(head & np.append(head[1:], True))
    head_at = np.maximum.accumulate(np.where(head, np.arange(n), 0))
    new_slot = np.flatnonzero(keep)
    return lcp.astype(np.uint32), new_slot.astype(np.uint32), head_at[new_slot].astype(np.uint32), head


# ---- the kernel's ranking and its store, emulated ------------------------------------------------------------------------------
def places(count):
    """(wave, row, lane) of every place of a sub-bucket in input order, as local_load deals them: a wave's stretch is
    rows * 64 pairs, row r of it the 64 pairs from r * 64"""
    rows = -(-count // THREADS)
    p = np.arange(count, dtype=np.int64)
    return p // (rows * 64), (p % (rows * 64)) // 64, p % 64


def emulate_sub_bucket(words, values, form, mistake=None, only_pass=None):
    """One sub-bucket of at most CAP pairs the way local_sort_kernel orders it: per digit, every place takes a ticket from
    its wave's counter of the digit (rows in order, the lanes of a row in lane order), the counters become start
    positions (bins in order, waves in order inside a bin), everybody moves.  The places behind the end hold the first
    pair again under a key of all ones.  -> the first `count` (words, values) of the staging buffer.
    Mistakes: "lanes_reversed_rows_ge_1" (rows >= 1 served from lane 63 down), "pads_zero" (pad keys 0),
    "two_bin_owner" (35-bit key, 1024 bins: the second bin of a thread that owns two starts where the first one starts
    plus the count of the bin BEHIND it -- an index off by one).  only_pass: the digit at which the lanes are reversed
    (all of them otherwise -- on pairs that keep their places, two reversals give the right order back)."""
    assert mistake in (None, "lanes_reversed_rows_ge_1", "pads_zero", "two_bin_owner")
    count = len(words)
    assert 0 < count <= CAP
    rows = -(-count // THREADS)
    total = rows * THREADS
    pad_key = 0 if mistake == "pads_zero" else 0xffffffff
    k = np.full(total, pad_key, dtype=np.int64)
    k[:count] = words
    w_out = k.copy()  # (what is staged as the word of a pad does not matter to the reference: it must not be stored)
    v = np.full(total, int(values[0]), dtype=np.int64)
    v[:count] = values
    wave, row, lane = places(total)
    shift = form.shift0
    for j, bits in enumerate(form.widths):
        d = (k >> shift) & ((1 << bits) - 1)
        reverse = mistake == "lanes_reversed_rows_ge_1" and only_pass in (None, j)
        serve = np.where((row >= 1) & reverse, 63 - lane, lane)
        # ticket = how many of my wave with my digit were served before me
        order = np.lexsort((serve, row, d, wave))
        grp = wave[order] * (1 << bits) + d[order]
        first = np.flatnonzero(np.append(True, grp[1:] != grp[:-1]))
        ticket = np.empty(total, dtype=np.int64)
        ticket[order] = np.arange(total) - np.repeat(first, np.diff(np.append(first, total)))
        cnt = np.zeros((THREADS // 64, 1 << bits), dtype=np.int64)
        np.add.at(cnt, (wave, d), 1)
        tot = cnt.sum(axis=0)
        bin_start = np.cumsum(tot) - tot
        if mistake == "two_bin_owner" and (1 << bits) > THREADS:
            extra = (1 << bits) - THREADS
            second = np.arange(1, 2 * extra, 2)
            bin_start[second] = bin_start[second - 1] + tot[second + 1]
        start = bin_start[None, :] + np.cumsum(cnt, axis=0) - cnt
        rank = np.clip(ticket + start[wave, d], 0, total - 1)
        nk, nv, nw = np.empty_like(k), np.empty_like(v), np.empty_like(w_out)
        nk[rank], nv[rank], nw[rank] = k, v, w_out
        k, v, w_out = nk, nv, nw
        shift += bits
    return w_out[:count].astype(np.uint32), v[:count].astype(np.uint32)


def store_written(first, count, mistake=None):
    """Which of the `count` elements of a sub-bucket that starts at element `first` local_store / local_store_buf write:
    whole 16-byte quads by every thread, the up to three elements in front of the first whole quad by threads 0 .. 2, those
    behind the last one by threads 3 .. 5.  Mistakes: "head_dropped", "tail_dropped"."""
    assert mistake in (None, "head_dropped", "tail_dropped")
    lo = first & 3
    hi = lo + count
    written = np.zeros(hi + 4, dtype=bool)
    qlo, qhi = (lo + 3) & ~3, hi & ~3
    iters = (CAP // 4 + 1 + THREADS - 1) // THREADS
    for j in range(iters):
        i0 = 4 * (j * THREADS + np.arange(THREADS))
        on = (i0 >= qlo) & (i0 + 4 <= qhi)
        for q in range(4):
            written[(i0 + q)[on]] = True
    head_end = min(qlo, hi)
    for tid in range(6):
        if tid < 3:
            e = lo + tid
            on = e < head_end and mistake != "head_dropped"
        else:
            e = max(qhi, head_end) + tid - 3
            on = e < hi and e >= head_end and mistake != "tail_dropped"
        if on:
            assert not written[e], "an element stored twice"
            written[e] = True
    assert not written[:lo].any() and not written[hi:].any(), "a store outside the sub-bucket"
    return written[lo:hi]


# ---- inputs ----------------------------------------------------------------------------------------------------------------
Case = namedtuple("Case", "name words starts subs")  # subs: {label: (first element, count)} of the sub-buckets it names


class Builder:
    """sub-buckets in index order -> words (already in sub-bucket order: the pass by the byte at bit 24 is the identity,
    the place of every pair under the caller's control) and bucket starts"""

    def __init__(self, form, nb, seed, tagged):
        self.form, self.nb, self.tagged = form, nb, tagged
        self.rng = np.random.default_rng(seed)
        self.pieces = []  # (sub, words, label)

    def low(self, count):
        """the bits below shift0: free, or a tag that meets the precondition of the regroup on the way (mostly full)"""
        f = self.form
        if f.shift0 == 0:
            return np.zeros(count, dtype=np.int64)
        if not self.tagged:
            return self.rng.integers(0, 1 << f.shift0, size=count)
        t = np.full(count, f.tag_full, dtype=np.int64)
        short = self.rng.random(count) < 0.02
        t[short] = self.rng.integers(0, f.tag_full, size=int(short.sum()))
        return t

    def random_digits(self, count):
        return [self.rng.integers(0, 1 << b, size=count) for b in self.form.widths]

    def add(self, sub, digits, low=None, label=None):
        f = self.form
        count = len(digits[0])
        assert 0 <= sub < 256 * self.nb and (not self.pieces or sub > self.pieces[-1][0]), "sub-buckets in index order"
        w = np.full(count, (sub & 255) << 24, dtype=np.int64)
        shift = f.shift0
        for d, bits in zip(digits, f.widths):
            d = np.asarray(d, dtype=np.int64)
            assert len(d) == count and d.min() >= 0 and d.max() < (1 << bits)
            w |= d << shift
            shift += bits
        w |= np.asarray(self.low(count) if low is None else low, dtype=np.int64)
        self.pieces.append((sub, w, label))

    def add_random(self, sub, count, label=None):
        self.add(sub, self.random_digits(count), label=label)

    def add_words(self, sub, low24, label=None):
        """a sub-bucket from the 24 bits below its byte, as they are"""
        low24 = np.asarray(low24, dtype=np.int64)
        assert low24.min() >= 0 and low24.max() < (1 << 24)
        assert 0 <= sub < 256 * self.nb and (not self.pieces or sub > self.pieces[-1][0]), "sub-buckets in index order"
        self.pieces.append((sub, ((sub & 255) << 24) | low24, label))

    def finish(self, name, shuffle=False):
        counts = np.zeros(self.nb, dtype=np.int64)
        subs, at = {}, 0
        for sub, w, label in self.pieces:
            counts[sub >> 8] += len(w)
            if label is not None:
                subs[label] = (at, len(w))
            at += len(w)
        starts = np.concatenate([[0], np.cumsum(counts)])
        words = np.concatenate([w for _, w, _ in self.pieces])
        if shuffle:  # inside every bucket: the pass by the byte at bit 24 does real work
            for b in range(self.nb):
                lo, hi = int(starts[b]), int(starts[b + 1])
                words[lo:hi] = words[lo:hi][self.rng.permutation(hi - lo)]
        assert len(words) <= 150_000, (name, len(words))
        return Case(name, words.astype(np.uint32), starts.astype(np.uint32), subs)


SIZES = [1, 2, 3, 4, 5, 7, 8, 63, 64, 65, 767, 768, 769, 1535, 1536, 1537, 4607, 4608, 4609, 17663, 17664, 17665, 18431, 18432]
KEY35_BINS0 = [0, 1, 255, 256, 510, 511, 512, 513, 767, 768, 1022, 1023]
KEY35_BINS1 = [0, 1, 255, 256, 510, 511]


def pattern_digit(name, count, bits, rng):
    """a digit for every place of a sub-bucket of `count` pairs, by wave stretch, row and lane"""
    wave, row, lane = places(count)
    p = np.arange(count)
    ones = (1 << bits) - 1
    if name == "one_digit":
        return np.full(count, 5)
    if name == "lane_and_1":
        return lane & 1
    if name == "lane_shr_5":
        return lane >> 5
    if name == "lane":
        return lane
    if name == "lane_reversed":
        return 63 - lane
    if name == "two_and_a_rare_third":
        return np.where(p % 97 == 96, 2, p & 1)
    if name == "row0_distinct_then_one":  # what the check of row 0 cannot see: every later row on ONE counter
        return np.where(row == 0, lane, 7)
    if name == "row0_one_then_distinct":
        return np.where(row == 0, 7, lane)
    if name == "uniform":
        return rng.integers(0, 1 << bits, size=count)
    if name == "three_values":
        return np.array([0, 100, ones])[rng.integers(0, 3, size=count)]
    if name == "all_ones":
        return np.full(count, ones)
    if name == "ones_and_zero":  # the last bin against the pad keys behind a partial row, lane by lane
        return np.where(lane & 1, ones, 0)
    raise KeyError(name)


PATTERNS = ["one_digit", "lane_and_1", "lane_shr_5", "lane", "lane_reversed", "two_and_a_rare_third", "row0_distinct_then_one",
            "row0_one_then_distinct", "uniform", "three_values", "all_ones", "ones_and_zero"]
PATTERN_SIZES = (65, 1537, 4609)
ROW_PATTERN_SIZE = 17665  # 24 rows, the last one partial: the two row patterns once more


def _spread(num_sub, k, base=5):
    """k sub-bucket indices spread over [base, num_sub)"""
    step = max(1, (num_sub - base - 1) // max(k, 1))
    return [base + j * step for j in range(k)]


def pattern_case(form, tagged, target, seed, shuffle=False):
    """every pattern on the digit(s) `target` (a tuple of digit indices); the other digits are one value, so that the
    passes in front of a target digit leave every pair at its place"""
    nb = 256 if form is not RECORDS else 5
    B = Builder(form, nb, seed, tagged)
    todo = [(pat, c) for pat in PATTERNS for c in PATTERN_SIZES]
    todo += [(pat, ROW_PATTERN_SIZE) for pat in ("row0_distinct_then_one", "row0_one_then_distinct")]
    for sub, (pat, c) in zip(_spread(256 * nb, len(todo)), todo):
        digits = [pattern_digit(pat, c, bits, B.rng) if j in target else np.full(c, 3) for j, bits in enumerate(form.widths)]
        B.add(sub, digits, label=f"{pat}/{c}")
    name = "patterns_d" + "".join(str(j) for j in target) + ("_shuffled" if shuffle else "")
    return B.finish(name, shuffle)


def cases(form, tagged=False):
    """the inputs of one form (module docstring of tests/test_gpu_local_sort.py says what each is there for); tagged: the
    bits below shift0 are tags that meet the precondition of the regroup on the way"""
    assert not (tagged and form is RECORDS)
    out = []
    seed = 1000 * (1 + list(FORMS).index(form.name)) + (500 if tagged else 0)
    nb = 256 if form is not RECORDS else 5
    ns = 256 * nb

    # every size at which the kernel takes another number of rows, up to its capacity
    B = Builder(form, nb, seed + 1, tagged)
    for sub, c in zip(_spread(ns, len(SIZES)), SIZES):
        B.add_random(sub, c, label=f"size{c}")
    B.add_random(ns - 1, 6, label="last")  # (n = 110 819: the last sub-bucket ends at n, no multiple of 4, with a tail)
    out.append(B.finish("sizes"))

    # beyond the capacity: the list and the segmented passes (40 000: ten tiles of them); two overflowing neighbours; an
    # overflowing one between two that fit
    B = Builder(form, nb, seed + 2, tagged)
    at = 300
    for c, label in ((100, None), (18433, "cap+1"), (40000, "tiles10"), (18433, "nbr0"), (18500, "nbr1"), (100, "fit0"), (19000, "between"),
                     (100, "fit1")):
        B.add_random(at, c, label=label)
        at += 1 if label in ("nbr0", "fit0", "between") else 211
    B.add_random(ns - 3, 3, label="last")
    out.append(B.finish("overflow"))
    B = Builder(form, nb, seed + 3, tagged)
    B.add_random(77, 18433, label="cap+1")
    B.add_random(78, 18432, label="cap")
    out.append(B.finish("capacity_edge"))

    # every size below 16 at every start residue mod 4 (fillers of 1 .. 4 pairs in front), the last sub-bucket ending at n
    B = Builder(form, nb, seed + 4, tagged)
    sub, at = 10, 0
    for c in range(1, 16):
        for r in range(4):
            fill = (r - at) % 4
            if fill or at == 0 and r:
                B.add_random(sub, fill)
                at += fill
                sub += 1
            B.add_random(sub, c, label=f"size{c}@{r}")
            assert at % 4 == r
            at += c
            sub += 3
    if at % 4 == 0:
        B.add_random(sub, 1)
    out.append(B.finish("residues"))

    # more non-empty sub-buckets than workgroups: every workgroup takes several turns, the keys of the next turn are
    # handed over; sizes mixed
    B = Builder(form, nb, seed + 5, tagged)
    k = 1500 if ns >= 4096 else ns - 6
    for sub in np.sort(B.rng.choice(ns, size=k, replace=False)).tolist():
        c = int(B.rng.integers(700, 900)) if B.rng.random() < 0.03 else int(B.rng.integers(1, 41))
        B.add_random(sub, c)
    out.append(B.finish("turns"))
    # .. one more than 256 workgroups (the second turn of one of them is the last of all), 255, 2, 1
    for name, subs, c in (("grid_plus_one", list(range(257)), 50), ("few_255", [3 + 5 * j for j in range(255)], 60),
                          ("few_2", [40, ns - 1], 1000), ("few_1", [ns // 2], 1000)):
        B = Builder(form, nb, seed + 6 + len(subs), tagged)
        for sub in subs:
            B.add_random(sub, c + sub % 7)
        out.append(B.finish(name))

    # the digit patterns by place: on the first digit, the second, (the third,) all of them; one shuffled inside the buckets
    nd = len(form.widths)
    for j in range(nd):
        out.append(pattern_case(form, tagged, (j,), seed + 20 + j))
    out.append(pattern_case(form, tagged, tuple(range(nd)), seed + 24))
    out.append(pattern_case(form, tagged, tuple(range(nd)), seed + 25, shuffle=True))
    B = Builder(form, nb, seed + 26, tagged)
    for sub, c in zip(_spread(ns, 6), (1000, 769, 4609, 18431, 65, 5000)):
        B.add_random(sub, c)
    out.append(B.finish("random_shuffled", shuffle=True))

    # digits of all ones in a sub-bucket whose last row is partial -- and, where the low bits are free, whole words of all
    # ones in the last sub-bucket of all: they must stay in front of the pad keys
    B = Builder(form, nb, seed + 27, tagged)
    for sub, c, label in ((200, 1000, "ones1000"), (ns - 1, 769, "ones769")):
        ones = B.rng.random(c) < 0.5
        digits = [np.where(ones, (1 << bits) - 1, d) for bits, d in zip(form.widths, B.random_digits(c))]
        low = B.low(c) if tagged else np.where(ones, (1 << form.shift0) - 1, B.low(c))
        B.add(sub, digits, low=low, label=label)
    out.append(B.finish("all_ones"))

    if form.key35:
        # the bins around the threads that own two of them (1024 bins on 768 threads: thread t < 256 owns 2t and 2t + 1,
        # the others t + 256) and around the edge between the two rules, on either digit
        B = Builder(form, nb, seed + 28, tagged)
        for sub, (c, on0, on1) in zip(_spread(ns, 6), [(1537, True, False), (1537, False, True), (1537, True, True), (65, True, True),
                                                       (4609, True, True), (769, True, False)]):
            p = np.arange(c)
            d0 = np.array(KEY35_BINS0)[(p * 7) % 12] if on0 else np.full(c, 3)
            d1 = np.array(KEY35_BINS1)[(p // 5) % 6] if on1 else np.full(c, 3)
            B.add(sub, [d0, d1], label=f"bins{c}/{int(on0)}{int(on1)}")
        out.append(B.finish("key35_bins"))
    return out


def record_bucket_cases():
    """records form: other numbers of buckets (1, 2, 3, 257; cases() has 5)"""
    out = []
    for nb in (1, 2, 3, 257):
        B = Builder(RECORDS, nb, 7000 + nb, False)
        sizes = [1, 3, 64, 65, 769, 1537, 4609, 2, 768, 18433 if nb == 3 else 300]
        for sub, c in zip(_spread(256 * nb, len(sizes), base=0), sizes):
            B.add_random(sub, c)
        B.add_random(256 * nb - 1, 6)
        out.append(B.finish(f"records_nb{nb}", shuffle=nb != 2))
    return out


def _in_design_order(design_keys, rng):
    """a random input order of elements given in sorted order that keeps the elements of one sort key in their order: the
    stable sort gives the design back"""
    c = len(design_keys)
    slots = rng.permutation(c)
    cls = np.asarray(design_keys)
    assert (np.diff(cls) >= 0).all()
    slot_of = slots[np.lexsort((slots, cls))]
    src = np.empty(c, dtype=np.int64)
    src[slot_of] = np.arange(c)
    return src  # input place -> design index


def fused_cases(form):
    """inputs for the form with the regroup on the way, designed in SORTED order (sort key = the bits above the tag, tags
    as given) and dealt out in a random input order that keeps equal keys in their order"""
    assert form in (KEY16, KEY35)
    full, tb = form.tag_full, form.shift0
    kbits = 24 - tb
    rng = np.random.default_rng(31 + tb)
    out = []

    def piece(keys, tags):
        keys, tags = np.asarray(keys, dtype=np.int64), np.asarray(tags, dtype=np.int64)
        src = _in_design_order(keys, rng)
        return ((keys << tb) | tags)[src]

    def runs(c, run_starts):
        """c elements, keys rising by one from run to run: run_starts = the places at which a new key starts"""
        key = np.zeros(c, dtype=np.int64)
        key[np.asarray(run_starts)] = 1
        key[0] = 0
        return np.cumsum(key) * 3 + 1

    # ties that stay tied at a sub-bucket's first place, its last place and across a 64-place edge; short tags inside runs
    # of equal keys at the same places; the sub-buckets are neighbours, so first and last places meet
    B = Builder(form, 256, 41, True)
    c = 1537
    edges = [2, 10, 60, 70, 126, 130, 191, 193, 300, 700, 766, 770, 1000, 1535]
    key = runs(c, edges)
    tags = np.full(c, full)
    B.add_words(1000, piece(key, tags), label="ties")
    tags = np.full(c, full)
    tags[[0, 1, 63, 64, 65, 127, 128, 767, 768, 1535, 1536]] = [3, full - 1, 0, 5, full - 1, 7, 7, 1, 2, 15, 4]
    tags[[400, 401, 402, 403]] = [6, 6, full, full]  # (two short elements with ONE word: heads all the same)
    B.add_words(1001, piece(key, tags), label="short_in_runs")
    B.add_words(1002, piece(np.full(769, 12345 % (1 << kbits)), np.full(769, full)), label="one_group_769")
    B.add_words(1003, piece(np.full(65, 0), np.full(65, full)), label="one_group_65")
    B.add_words(1004, piece(np.arange(4609) * 3, np.full(4609, full)), label="all_heads")
    # boundaries decided by the key bits at every depth (keys that differ in one bit, from the lowest up), by the tag (a
    # short element between equal keys; neighbours with long common prefixes and short tags)
    depth_keys = np.sort(np.concatenate([[0], 1 << np.arange(kbits), (1 << np.arange(kbits)) + 1]))
    depth_keys = np.unique(depth_keys)
    B.add_words(1005, piece(depth_keys, np.full(len(depth_keys), full)), label="key_bit_depths")
    t = rng.integers(0, full + 1, size=len(depth_keys))
    B.add_words(1006, piece(depth_keys, t), label="tag_decides")
    out.append(B.finish("fused_places"))

    # the bucket byte: empty sub-buckets between two whose last and first stored words are equal but whose buckets differ,
    # in every bit of the bucket byte; and the first boundary of a sub-bucket inside one bucket
    B = Builder(form, 256, 42, True)
    wlow = (0x2a5a5a & ((1 << 24) - 1 - ((1 << tb) - 1))) | full
    subs = [bucket * 256 + 0x5a for bucket in (0, 1, 2, 3, 4, 8, 16, 32, 64, 128, 129, 255)]
    subs += [200 * 256 + byte for byte in (0, 1, 2, 4, 8, 16, 32, 64, 128, 255)]  # (.. and of the byte below it)
    for sub in sorted(subs):
        B.add_words(sub, np.full(3 if sub % 2 else 1, wlow), label=f"sub{sub}")
    out.append(B.finish("fused_bucket_byte"))

    # random keys from few values (long runs), sizes at the row edges, sub-buckets side by side: many turns per workgroup
    B = Builder(form, 256, 43, True)
    sub = 20000
    for c in (1, 2, 3, 64, 65, 767, 768, 769, 1537, 4609, 18431, 18432, 5):
        key = np.sort(rng.integers(0, max(2, c // 3), size=c))
        tags = np.where(rng.random(c) < 0.05, rng.integers(0, full, size=c), full)
        B.add_words(sub, piece(key, tags), label=f"runs{c}")
        sub += 1 if c % 2 else 255
    out.append(B.finish("fused_sizes"))
    return out


def all_cases(form, fused):
    """every input a form is run on: plain -> free low bits; fused -> tags"""
    if form is RECORDS:
        assert not fused
        return cases(form) + record_bucket_cases()
    return cases(form, True) + fused_cases(form) if fused else cases(form, False)


def expected(case, form, fused):
    """-> dict of what the hook must return for a case"""
    n = len(case.words)
    values = np.arange(n, dtype=np.uint32)
    sw, sv = stable_sort(case.words, values, case.starts, form.shift0)
    exp = {"words": sw, "values": sv, "listed": listed_count(case.words, case.starts)}
    if fused and exp["listed"] == 0:
        lcp, slot, grp, _ = regroup(sw, bucket_of(case.starts), form)
        exp.update(lcp=lcp, new_slot=slot, new_grp=grp, survivors=len(slot))
    return exp
