"""The permutation into text order (text_order.hpp: bucketed_scatter, permute_packed) in plain numpy -- TEST
INFRASTRUCTURE, nothing of it is taken from the code under test:
  * the reference: out[idx[k]] = val[k] for idx[k] < n_out, out2[idx[k]] = k + 1, every other target keeps the fill word;
    the 16-bit codes min(code, max) and the wide-code list; for permute_packed the low half of a word to out, the high
    half to out2 (scatter, narrow_codes, wide_list, permute; expected puts them together for a case);
  * what the chooser must do with a shape, after the comments of text_order.hpp / text_order.hip: index_bits,
    window_bits_of, is_big, esc_threshold, exc_capacity, expected_form;
  * the inputs of tests/test_gpu_text_order_direct.py (the *_cases functions; the arrays are made when asked for);
  * wrong variants of the reference (MISTAKES), so that tests/test_text_order_model_host.py can show without a GPU that
    for each of them the list holds an input whose expected result differs.
idx never names a target below n_out twice: the plain scatter is a race on duplicates and no caller sends them."""
import functools

import numpy as np

U32 = np.uint32
FILL = 0xA5C3F00D          # what the targets hold before the call
RADIX_BITS = 8
WINDOW_BITS_MAX = 14
LB_TILE = 1 << 14          # pairs per tile of the look-back passes
SORT_TILE = 4096           # pairs per tile of the passes with histograms
PARTIAL_WINDOW_BITS = 19   # the window of a partial scatter
MULT = 2654435761          # a prime above 2^31: k -> (k * MULT + add) % n is a bijection of [0, n) for every n below it
SEPARATOR_ERROR = "record scatter: a separator suffix is not the first of its record"


# ---- what the chooser does ------------------------------------------------------------------------------------------
def index_bits(n_out):
    """bits of a target position below n_out (at least 1)"""
    nb = 1
    while nb < 32 and (1 << nb) < n_out:
        nb += 1
    return nb


def window_bits_of(nb):
    """what two digits of 8 bits leave of nb index bits, 2^10 entries at least"""
    return nb - 2 * RADIX_BITS if nb > 2 * RADIX_BITS + 10 else 10


def two_passes(nb):
    return nb <= 2 * RADIX_BITS + WINDOW_BITS_MAX


def is_big(n_out, count):
    """a target beyond 64 MiB and more than 2^22 pairs"""
    return n_out * 4 > (64 << 20) and count > (1 << 22)


def esc_threshold(n_out, knob=None):
    """codes at or above it are escaped by the packed form: the word [code | rank : nb | low wb + 8 index bits] leaves
    64 - nb - wb - 8 bits to the code, and the largest value of that field marks an escape (NOLZSS_TEXT_ORDER_ESC lowers it)"""
    nb = index_bits(n_out)
    esc = (1 << (64 - nb - window_bits_of(nb) - RADIX_BITS)) - 1
    return esc if knob is None else min(esc, knob)


def exc_capacity(count):
    """entries of the packed form's exception list"""
    return max(count // 64, 1024)


def expected_form(n_out, count, want_out2=False, short_codes=True, narrow=False, plan=False, hist_knob=False, escaped=0):
    """-> {"form", "packed_tried", "list_overflow", "result", "partition_passes"} for a call of bucketed_scatter"""
    big = is_big(n_out, count)
    perm = big and count == n_out
    nb = index_bits(n_out)
    two_value = want_out2 and perm and two_passes(nb) and not plan
    tried = two_value and short_codes and not hist_knob
    overflow = tried and escaped > exc_capacity(count)
    r = {"packed_tried": tried, "list_overflow": overflow, "result": True, "partition_passes": 0}
    if count == 0:
        r.update(form="none", result=not narrow)
    elif tried and not overflow:
        r.update(form="packed")
    elif narrow:
        r.update(form="none", result=False)
    elif two_value:
        r.update(form="two_value_hist")
    elif plan and count == n_out:
        r.update(form="record_plan2" if want_out2 else "record_plan")
    elif perm:
        r.update(form="window_perm")
    else:
        passes = 0
        if big and nb > PARTIAL_WINDOW_BITS:
            passes = 2 if nb > PARTIAL_WINDOW_BITS + RADIX_BITS else 1
        r.update(form="partial_then_plain" if passes else "plain", partition_passes=passes)
    return r


def expected_permute_form(count):
    return "permute_plain" if count <= (1 << 22) or not two_passes(index_bits(count)) else "permute_windows"


def plan_is_made(lens, bucket_min):
    """record_scatter_plan: two records at least, none empty or beyond 2^22 bases, records of bucket_min symbols on average"""
    n = sum(lens) + len(lens) - 1
    return len(lens) >= 2 and bucket_min > 0 and len(lens) * bucket_min <= n and all(0 < x <= 1 << 22 for x in lens)


# ---- the reference --------------------------------------------------------------------------------------------------
# the wrong variants: name -> what a kernel with that mistake would deliver (tests/test_text_order_model_host.py)
MISTAKES = ("rank_without_plus_one", "window_mask_one_bit_short", "last_partial_window_dropped", "escape_on_greater",
            "halves_swapped", "dropped_written_modulo", "untouched_zeroed", "keep_val_ignored", "separator_to_rank",
            "saturation_at_max_minus_one")


def scatter(idx, val, n_out, fill=FILL, mistake=None, wb=None):
    """-> (out, out2): out[idx[k]] = val[k], out2[idx[k]] = k + 1 for idx[k] < n_out; fill elsewhere"""
    idx = np.asarray(idx, dtype=U32)
    val = np.asarray(val, dtype=U32)
    rank = np.arange(1, idx.size + 1, dtype=U32)
    if mistake == "rank_without_plus_one":
        rank = rank - U32(1)
    out = np.full(n_out, 0 if mistake == "untouched_zeroed" else fill, dtype=U32)
    out2 = out.copy()
    keep = idx < n_out
    at = idx[keep].astype(np.int64)
    if mistake in ("window_mask_one_bit_short", "last_partial_window_dropped"):
        W = 1 << (window_bits_of(index_bits(n_out)) if wb is None else wb)
        if mistake == "window_mask_one_bit_short":
            at = (at & ~(W - 1)) | (at & (W // 2 - 1))
        else:
            stay = at < n_out // W * W
            at, keep = at[stay], np.flatnonzero(keep)[stay]
    out[at] = val[keep]
    out2[at] = rank[keep]
    if mistake == "dropped_written_modulo":
        out[idx[~keep].astype(np.int64) % n_out] = val[~keep]
    return out, out2


def narrow_codes(codes, code_max, mistake=None):
    """the 16-bit form of codes in text order: min(code, max)"""
    top = code_max - 1 if mistake == "saturation_at_max_minus_one" else code_max
    return np.minimum(codes, U32(top)).astype(np.uint16)


def wide_list(codes, code_max, esc, mistake=None):
    """the wide-code list of codes in text order, sorted: position | code << 32 for every code >= max -- and, as the
    comment of window_unpack16_kernel says, an escaped code is listed twice where the threshold reaches max: once with
    the threshold as its value, by the windows, and once with the true one, by escape_fixup_kernel"""
    codes = np.asarray(codes, dtype=U32)
    pos = np.flatnonzero(codes >= code_max)
    items = [pos.astype(np.uint64) | (codes[pos].astype(np.uint64) << np.uint64(32))]
    if esc >= code_max:
        twice = np.flatnonzero(codes > esc if mistake == "escape_on_greater" else codes >= esc)
        items.append(twice.astype(np.uint64) | (np.uint64(esc) << np.uint64(32)))
    return np.sort(np.concatenate(items))


def list_as_bounds(items):
    """position -> the largest code listed for it (code16.hpp: `the larger entry counts`)"""
    d = {}
    for x in np.asarray(items, dtype=np.uint64).tolist():
        p, c = x & 0xffffffff, x >> 32
        d[p] = max(d.get(p, 0), c)
    return d


def escaped_count(val, esc, mistake=None):
    val = np.asarray(val, dtype=U32)
    return int((val > esc).sum() if mistake == "escape_on_greater" else (val >= esc).sum())


def permute(idx, packed, mistake=None):
    """-> (out, out2) of permute_packed: idx is a permutation of [0, count)"""
    packed = np.asarray(packed, dtype=np.uint64)
    lo, hi = (packed & np.uint64(0xffffffff)).astype(U32), (packed >> np.uint64(32)).astype(U32)
    if mistake == "halves_swapped":
        lo, hi = hi, lo
    out, out2 = np.empty(idx.size, dtype=U32), np.empty(idx.size, dtype=U32)
    out[idx] = lo
    out2[idx] = hi
    return out, out2


# ---- the inputs -----------------------------------------------------------------------------------------------------
def hash32(count, seed, first=0):
    """arbitrary 32-bit words: the high half of (k * odd + seed) mod 2^64"""
    k = np.arange(first, first + count, dtype=np.uint64)
    return ((k * np.uint64(0x9E3779B97F4A7C15) + np.uint64(seed * 0x632BE59BD9B4E019 % (1 << 64))) >> np.uint64(32)).astype(U32)


def affine(n, count=None, add=12345):
    """the first `count` values of the bijection k -> (k * MULT + add) % n of [0, n)"""
    k = np.arange(n if count is None else count, dtype=np.uint64)
    return ((k * np.uint64(MULT) + np.uint64(add)) % np.uint64(n)).astype(U32)


@functools.lru_cache(maxsize=4)
def permutation(n, kind="affine"):
    """a permutation of [0, n) (read-only: shared by the cases of one size)"""
    if kind == "affine":
        p = affine(n)
    elif kind == "identity":
        p = np.arange(n, dtype=U32)
    elif kind == "reverse":
        p = np.arange(n, dtype=U32)[::-1].copy()
    elif kind == "random":
        p = np.random.default_rng(n).permutation(n).astype(U32)
    else:
        raise ValueError(kind)
    p.setflags(write=False)
    return p


@functools.lru_cache(maxsize=4)
def inverse(n, kind="affine"):
    inv = np.empty(n, dtype=U32)
    inv[permutation(n, kind)] = np.arange(n, dtype=U32)
    inv.setflags(write=False)
    return inv


def partial_indices(n_out, count, layout, seed=1):
    """count indices for a partial scatter, no target below n_out named twice, about 5 % at or above n_out (n_out itself,
    2^nbits, 2^31, 0xffffffff among them).  layout "spread": over the whole target; "cluster": the first 2^19 pairs fill
    ONE window of 2^19 targets (every pair of 128 tiles in one bin), the rest is spread over the others"""
    idx = affine(n_out, count, add=seed)
    drop = hash32(count, seed + 77) % U32(20) == 0
    if layout == "cluster":
        wsize = 1 << PARTIAL_WINDOW_BITS
        w = (n_out >> PARTIAL_WINDOW_BITS) // 2
        m = min(wsize, count, n_out - w * wsize)
        drop |= (idx >> U32(PARTIAL_WINDOW_BITS)) == w
        idx[:m] = U32(w * wsize) + affine(m, add=seed + 5)
        drop[:m] = False
    elif layout != "spread":
        raise ValueError(layout)
    drop[-2:] = True   # (n_out itself and 0xffffffff are always there)
    ks = np.flatnonzero(drop)
    idx[ks] = (np.uint64(n_out) + np.arange(ks.size, dtype=np.uint64)).astype(U32)   # (n_out itself is the first)
    for k, v in zip(ks[1:], (0xffffffff, 0xfffffffe, 1 << 31, 1 << index_bits(n_out), (1 << 31) + 12345)):
        if v >= n_out + ks.size:
            idx[k] = v
    return idx


def record_layout(lens):
    """the block-diagonal permutation of a text of records of lens[k] bases with a separator behind all but the last,
    as record_scatter_plan describes it: the separator behind record k is the first rank of the record's ranks, the
    ranks behind it hold the record's positions -> (idx, rec_ends)"""
    n = sum(lens) + len(lens) - 1
    idx = np.empty(n, dtype=U32)
    ends, start = [], 0
    for k, length in enumerate(lens):
        inner = U32(start) + affine(length, add=k + 3)
        if k + 1 < len(lens):
            idx[start] = start + length
            idx[start + 1:start + 1 + length] = inner
            ends.append(start + length)
            start += length + 1
        else:
            idx[start:start + length] = inner
            ends.append(n)
    return idx, np.array(ends, dtype=U32)


def edge_ranks(n_out, count, kind):
    """list positions at the edges of the look-back tiles and the pairs whose targets lie at the edges of the windows"""
    W = 1 << window_bits_of(index_bits(n_out))
    last_tile = (count - 1) // LB_TILE * LB_TILE
    ks = [0, 63, 64, SORT_TILE - 1, SORT_TILE, LB_TILE - 1, LB_TILE, last_tile - 1, last_tile, count - 1]
    last_w = (n_out - 1) // W * W
    ps = [0, W - 1, W, 256 * W - 1, 256 * W, last_w - 1, last_w, n_out - 1]
    inv = inverse(n_out, kind)
    return sorted({k for k in ks + [int(inv[p]) for p in ps if p < n_out] if 0 <= k < count})


def packed_codes(n_out, codes, esc, kind="affine", seed=3):
    """the code sets of the packed form, count = n_out:
      below     every code below the threshold (threshold - 1 among them)
      planted   small codes; threshold - 1, threshold, threshold + 1 and 0xffffffff around every edge of edge_ranks
      many      one code in 1024 at or above the threshold: at least 10 000 of them, and they fit the exception list
      overflow  one in 32: more than the list holds"""
    small = U32(min(esc, 1000))
    val = hash32(n_out, seed) % small
    if codes == "below":
        val = hash32(n_out, seed) % U32(esc)
        val[5] = esc - 1
    elif codes == "planted":
        special = (esc - 1, esc, esc + 1, 0xffffffff)
        for e, k0 in enumerate(edge_ranks(n_out, n_out, kind)):
            for j in range(4):  # the four values around every edge, in another rotation at each
                k = k0 + j - 1
                if 0 <= k < n_out:
                    val[k] = special[(e + j) % 4]
    elif codes in ("many", "overflow"):
        step = 1024 if codes == "many" else 32
        big = hash32(len(val[::step]), seed + 1)
        val[::step] = np.maximum(big, U32(esc))
        val[0], val[step] = esc, 0xffffffff
    else:
        raise ValueError(codes)
    return val


def narrow_code_values(n_out, code_max, esc, seed=4):
    """codes for the 16-bit form: below max and the threshold, and one in 4096 from max - 1, max, max + 1, threshold - 1,
    threshold, threshold + 1, 0xffffffff in turn"""
    val = hash32(n_out, seed) % U32(min(code_max, esc))
    special = np.array([code_max - 1, code_max, code_max + 1, esc - 1, esc, esc + 1, 0xffffffff], dtype=np.uint64).astype(U32)
    ks = np.arange(0, n_out, 4096)
    val[ks] = special[np.arange(ks.size) % 7]
    val[n_out - 1] = code_max
    return val


class Case:
    """one call of the hook: name, how to make its arrays, the arguments, what must come of it"""

    def __init__(self, name, n_out, count, make, permute=False, kind="affine", rec_lens=None, partial=None, esc_knob=None, **kw):
        self.name, self.n_out, self.count, self._make, self.is_permute = name, n_out, count, make, permute
        # where idx comes from: record_layout(rec_lens), partial_indices(n_out, count, partial) or permutation(n_out, kind)
        self.kind, self.rec_lens, self.partial, self.esc_knob = kind, rec_lens, partial, esc_knob
        self.kw = dict(keep_input=True, keep_val=True, short_codes=True, want_out2=False, narrow=None)
        self.kw.update(kw)

    def arrays(self):
        """-> (idx, val or packed, rec_ends or None)"""
        got = self._make()
        return got if len(got) == 3 else (got[0], got[1], None)

    def esc(self):
        return esc_threshold(self.n_out, self.esc_knob)

    def __repr__(self):
        return self.name


BIG_SIZES = ((1 << 24) + 1, (1 << 24) + 4097, 1 << 25, (1 << 25) + 1)   # index bits 25 25 25 26, windows of 2^10
WB11_SIZE = (1 << 26) + 4097                                             # the smallest target with windows of 2^11
KEEPS = ((True, True), (True, False), (False, True))                     # keep_input, keep_val


def perm_case(name, n, kind, seed, **kw):
    return Case(name, n, n, lambda: (permutation(n, kind), hash32(n, seed)), kind=kind, **kw)


def small_cases():
    """the plain scatter, with the rank scatter beside it for out2: whole permutations up to the largest target that is
    not big, and partial ones with dropped indices"""
    cases = []
    for n in (1, 63, 4097, 1 << 24):
        cases.append(perm_case(f"small_perm_{n}", n, "affine", n, want_out2=True))
    for n, count in ((63, 40), (4097, 3000), (4097, 4097), (1 << 24, 3 << 20)):
        cases.append(Case(f"small_partial_{n}_{count}", n, count,
                          lambda n=n, count=count: (partial_indices(n, count, "spread"), hash32(count, n + 1)),
                          partial="spread", want_out2=True, keep_input=(n != 4097)))
    cases.append(Case("small_partial_no_out2", 4097, 2000, lambda: (partial_indices(4097, 2000, "spread"), hash32(2000, 9)),
                      partial="spread"))
    return cases


def window_cases():
    """the one-value window permutation: every size under every legal keep_input / keep_val, the window of 2^11 once"""
    cases = [perm_case(f"window_{n}_keep{int(ki)}{int(kv)}", n, "affine", n + 1, keep_input=ki, keep_val=kv)
             for n in BIG_SIZES for ki, kv in KEEPS]
    cases.append(perm_case(f"window_random_{BIG_SIZES[0]}", BIG_SIZES[0], "random", 5))
    cases.append(perm_case(f"window_identity_{BIG_SIZES[1]}", BIG_SIZES[1], "identity", 6, keep_val=False))
    cases.append(perm_case(f"window_wb11_{WB11_SIZE}", WB11_SIZE, "affine", 7))
    return cases


def hist_cases():
    """the two-value form with histograms, as rc.hip asks for it (short_codes = false): values of 32 bits"""
    cases = [perm_case(f"hist_{n}", n, "affine", n + 2, want_out2=True, short_codes=False) for n in BIG_SIZES]
    cases.append(perm_case(f"hist_reverse_{BIG_SIZES[1]}_keep0", BIG_SIZES[1], "reverse", 8, want_out2=True, short_codes=False,
                           keep_input=False))
    return cases


def packed_cases(esc_knob=None):
    """the packed form (or, under NOLZSS_TEXT_ORDER_HIST, the histogram form on the same inputs): four code sets a size"""
    cases = []
    for n in BIG_SIZES:
        for codes in ("below", "planted", "many", "overflow"):
            kind = "reverse" if (n, codes) == (BIG_SIZES[2], "planted") else "affine"
            cases.append(Case(f"packed_{n}_{codes}", n, n,
                              lambda n=n, codes=codes, kind=kind: (permutation(n, kind), packed_codes(n, codes, esc_threshold(n, esc_knob), kind)),
                              kind=kind, esc_knob=esc_knob, want_out2=True))
    return cases


NARROW_SHAPES = ((BIG_SIZES[1], 0xffff, 1 << 16), (BIG_SIZES[1], 0xffff, 100), (BIG_SIZES[1], 1000, 1 << 16),
                 (BIG_SIZES[1], 1000, 100), (BIG_SIZES[3], 0xffff, 1 << 16), (BIG_SIZES[3], 1000, 100))


def narrow_cases(esc_knob=None):
    """the packed form writing 16-bit codes: both saturation values, a list that holds the wide codes and one that does
    not; then the two ways to `false`: a target the packed form does not take, an exception list that overflows"""
    cases = []
    for n, code_max, cap in NARROW_SHAPES:
        cases.append(Case(f"narrow_{n}_max{code_max}_cap{cap}", n, n,
                          lambda n=n, code_max=code_max: (permutation(n), narrow_code_values(n, code_max, esc_threshold(n, esc_knob))),
                          esc_knob=esc_knob, want_out2=True, narrow=(cap, code_max)))
    n = 1 << 24
    cases.append(Case(f"narrow_not_applicable_{n}", n, n, lambda: (permutation(1 << 24), hash32(1 << 24, 11) % U32(1000)),
                      esc_knob=esc_knob, want_out2=True, narrow=(1 << 16, 0xffff)))
    n = BIG_SIZES[0]
    cases.append(Case(f"narrow_overflow_{n}", n, n, lambda: (permutation(n), packed_codes(n, "overflow", esc_threshold(n, esc_knob))),
                      esc_knob=esc_knob, want_out2=True, narrow=(1 << 16, 0xffff)))
    return cases


def partial_cases():
    """a partial scatter into a big target: 2^22 pairs (not big: the plain scatter alone), 2^22 + 1 and 2^23 + 77 (one
    partition pass), a target of 2^27 + 4097 (two); spread and clustered indices, some at or above n_out"""
    cases = []
    n = BIG_SIZES[1]
    for count in (1 << 22, (1 << 22) + 1, (1 << 23) + 77):
        for layout in ("spread", "cluster"):
            for ki in (True, False):
                cases.append(Case(f"partial_{count}_{layout}_keep{int(ki)}", n, count,
                                  lambda count=count, layout=layout: (partial_indices(n, count, layout), hash32(count, count)),
                                  partial=layout, keep_input=ki, keep_val=(layout == "spread"),
                                  want_out2=(count == (1 << 22) + 1 and ki)))
    n2, c2 = (1 << 27) + 4097, (1 << 22) + 77
    cases.append(Case(f"partial_two_passes_{n2}", n2, c2, lambda: (partial_indices(n2, c2, "spread"), hash32(c2, 13)), partial="spread"))
    return cases


MIXED_RECORDS = (1, 63, 64, 65, 4095, 4096, 4097, 1 << 14, (1 << 14) + 1, 1 << 22, 1, 1, 64, 4097, 2, 16383)
ABOVE_2_24 = (1 << 22, 65, (1 << 22) - 1, 1 << 22, 4096, 1 << 22, 1, 63, 1 << 14)      # 2^24 + 20 668 symbols
DEFAULT_RECORDS = (1 << 22, (1 << 16) + 1, 1 << 17, 70000, 1 << 16)                      # 65 536 symbols a record or more


def record_case(name, lens, bucket_min, seed, **kw):
    n = sum(lens) + len(lens) - 1

    def make():
        idx, ends = record_layout(lens)
        return idx, hash32(n, seed), ends
    c = Case(name, n, n, make, rec_lens=tuple(lens), **kw)
    c.plan = plan_is_made(lens, bucket_min)
    return c


def record_cases(bucket_min):
    """block-diagonal permutations with a plan.  bucket_min = 1 (NOLZSS_REC_BUCKET_MIN=1): records of every length at
    which the first tile, a tile or a window ends, up to the limit of 2^22 bases and one beyond it (no plan: the general
    form).  bucket_min = 2^16: the default, which wants 65 536 symbols a record"""
    if bucket_min != 1:
        return [record_case("records_default", DEFAULT_RECORDS, bucket_min, 21, want_out2=True),
                record_case("records_default_one_value", DEFAULT_RECORDS, bucket_min, 22, keep_input=True, keep_val=False)]
    cases = []
    for two in (False, True):
        t = "2" if two else "1"
        cases.append(record_case(f"records_mixed_{t}", MIXED_RECORDS, 1, 23, want_out2=two))
        cases.append(record_case(f"records_two_only_{t}", (4097, 63), 1, 24, want_out2=two))
        cases.append(record_case(f"records_above_2_24_{t}", ABOVE_2_24, 1, 25, want_out2=two))
    cases.append(record_case("records_two_of_one_base", (1, 1), 1, 26, want_out2=True))
    cases.append(record_case("records_beyond_limit", (100, (1 << 22) + 1, 64), 1, 27, want_out2=True))
    return cases


def separator_error_case():
    """records_default with the rank of one separator and the rank behind it swapped: still a permutation, no longer
    block-diagonal"""
    c = record_case("records_separator_swapped", DEFAULT_RECORDS, 1 << 16, 28, want_out2=True)
    make = c._make

    def swapped():
        idx, val, ends = make()
        idx = idx.copy()
        r = int(ends[0]) + 1        # the separator behind record 1: the first of the ranks of record 1
        idx[[r, r + 1]] = idx[[r + 1, r]]
        return idx, val, ends
    c._make = swapped
    return c


PERMUTE_COUNTS = (1, 4097, 1 << 22, (1 << 22) + 1, (1 << 24) + 4097, (1 << 25) + 1)


def permute_cases():
    """permute_packed: the plain scatter up to 2^22 pairs, two passes and the windows beyond"""
    def make(n):
        return permutation(n), hash32(n, n + 3).astype(np.uint64) | (hash32(n, n + 4).astype(np.uint64) << np.uint64(32))
    return [Case(f"permute_{n}", n, n, lambda n=n: make(n), permute=True) for n in PERMUTE_COUNTS]


def in_process_cases():
    return (small_cases() + window_cases() + hist_cases() + packed_cases() + narrow_cases() + partial_cases() +
            record_cases(1 << 16) + permute_cases())


ESC_KNOB = 100   # NOLZSS_TEXT_ORDER_ESC of the child process: below both saturation values of the 16-bit cases


def child_cases():
    """what the child processes run on top (their knobs are frozen at first use)"""
    return {"hist": packed_cases() + narrow_cases()[:1], "esc": packed_cases(ESC_KNOB) + narrow_cases(ESC_KNOB), "records": record_cases(1)}


# ---- what a call must deliver -----------------------------------------------------------------------------------------
def expected(case, hist_knob=False, mistake=None, arrays=None):
    """everything the hook returns for `case`, by the reference: {"form", "packed_tried", "list_overflow", "result",
    "partition_passes", "escaped", "nbits", "wb", "out", "out2", "narrow", "list", "listed", "idx_survives",
    "val_survives"} (entries that do not apply, or that a `false` result leaves open: None)"""
    idx, val, ends = arrays if arrays is not None else case.arrays()
    kw = case.kw
    if case.is_permute:
        out, out2 = permute(idx, val, mistake)
        nb = index_bits(case.count)
        return {"form": expected_permute_form(case.count), "packed_tried": False, "list_overflow": False, "result": True,
                "partition_passes": 0, "escaped": 0, "nbits": nb, "wb": window_bits_of(nb), "out": out, "out2": out2,
                "narrow": None, "list": None, "listed": 0, "idx_survives": False, "val_survives": False}
    plan = ends is not None and getattr(case, "plan", False)
    esc = case.esc()
    shape = expected_form(case.n_out, case.count, kw["want_out2"], kw["short_codes"], kw["narrow"] is not None, plan, hist_knob)
    escaped = escaped_count(val, esc, mistake) if shape["packed_tried"] else 0
    r = expected_form(case.n_out, case.count, kw["want_out2"], kw["short_codes"], kw["narrow"] is not None, plan, hist_knob, escaped)
    nb = index_bits(case.n_out)
    r.update(escaped=escaped, nbits=nb, wb=WINDOW_BITS_MAX if r["form"].startswith("record_plan") or not two_passes(nb) else window_bits_of(nb),
             narrow=None, list=None, listed=0)
    sep_mistake = mistake == "separator_to_rank" and plan
    out, out2 = scatter(idx, val, case.n_out, mistake=mistake, wb=r["wb"] if plan else None)
    if sep_mistake:
        # the separator at position ends[k] is the suffix of rank (ends[k - 1] + 1, or 0): the first of its record's ranks
        starts = np.concatenate([[0], ends[:-2].astype(np.int64) + 1]).astype(np.int64)
        seps = ends[:-1].astype(np.int64)
        out[seps], out2[seps] = FILL, FILL
        out[starts], out2[starts] = val[starts], starts.astype(U32) + U32(1)
    if not kw["want_out2"]:
        out2 = None
    if kw["narrow"] is not None:
        cap, code_max = kw["narrow"]
        if r["result"]:
            items = wide_list(out, code_max, esc, mistake)
            r.update(narrow=narrow_codes(out, code_max, mistake), listed=len(items), list=items if len(items) <= cap else None,
                     codes=out)
        out = None   # (not used with the 16-bit codes)
    if not r["result"]:
        out = out2 = None   # nothing usable is written (the windows may have run: the wide-code list holds anything)
        r["listed"] = None
    keeps = kw["keep_input"] or r["form"].startswith("record_plan")
    r.update(out=out, out2=out2, idx_survives=keeps, val_survives=keeps and (kw["keep_val"] or r["form"].startswith("record_plan")))
    if mistake == "keep_val_ignored" and kw["keep_input"] and kw["keep_val"] and r["form"] in ("window_perm", "partial_then_plain"):
        r["val_after"] = stable_partition(idx, val, r["wb"] + RADIX_BITS if r["form"] == "window_perm" else PARTIAL_WINDOW_BITS + RADIX_BITS)
    return r


def stable_partition(idx, val, shift):
    """val in the order of a stable partition of the pairs by the 8-bit digit of idx at `shift`: what val[0] holds after
    the second pass when it serves as a ping-pong buffer"""
    return np.asarray(val)[np.argsort(((np.asarray(idx) >> U32(shift)) & U32(255)).astype(np.uint8), kind="stable")]
