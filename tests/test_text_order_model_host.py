"""tests/text_order_model.py without a GPU: the reference against plain Python loops, every input generator against its
own conditions, the chooser's predictions against the figures of text_order.hpp, and -- for each of ten mistakes a
kernel of text_order.hip could plausibly make -- an input of tests/test_gpu_text_order_direct.py whose expected result
would differ.  The two caps the packed-form cases depend on are computed here, so that the GPU test cannot hide behind a
miscounted input."""
import numpy as np
import pytest

import text_order_model as M


def all_gpu_cases():
    cases = M.in_process_cases()
    for extra in M.child_cases().values():
        cases += extra
    return cases


def named(name, cases=None):
    got = [c for c in (cases or all_gpu_cases()) if c.name == name]
    assert got, name
    return got[0]


# ---- the reference against plain loops ------------------------------------------------------------------------------
def loop_scatter(idx, val, n_out, fill):
    out, out2 = [fill] * n_out, [fill] * n_out
    for k, (i, v) in enumerate(zip(idx.tolist(), val.tolist())):
        if i < n_out:
            out[i] = v
            out2[i] = k + 1
    return out, out2


@pytest.mark.parametrize("case", [c for c in M.small_cases() if c.n_out <= 4097] + M.record_cases(1)[1:2], ids=repr)
def test_scatter_is_the_plain_loop(case):
    idx, val, _ = case.arrays()
    out, out2 = M.scatter(idx, val, case.n_out)
    lo, lo2 = loop_scatter(idx, val, case.n_out, M.FILL)
    assert out.tolist() == lo and out2.tolist() == lo2
    exp = M.expected(case)
    assert exp["out"].tolist() == lo and (exp["out2"] is None or exp["out2"].tolist() == lo2)


def test_permute_is_the_plain_loop():
    case = named("permute_4097")
    idx, packed, _ = case.arrays()
    out, out2 = M.permute(idx, packed)
    for k in range(0, 4097, 13):
        assert out[idx[k]] == int(packed[k]) & 0xffffffff and out2[idx[k]] == int(packed[k]) >> 32


def test_narrow_codes_and_list_are_the_plain_loop():
    codes = np.array([0, 999, 1000, 1001, 2046, 2047, 2048, 0xffffffff, 5], dtype=np.uint32)
    assert M.narrow_codes(codes, 1000).tolist() == [min(c, 1000) for c in codes.tolist()]
    # the threshold (2047) at or above max: the escaped codes are listed twice, once with the threshold as their value
    want = sorted([p | c << 32 for p, c in enumerate(codes.tolist()) if c >= 1000] + [p | 2047 << 32 for p, c in enumerate(codes.tolist()) if c >= 2047])
    assert M.wide_list(codes, 1000, 2047).tolist() == want
    # the threshold below max: once
    assert M.wide_list(codes, 1000, 100).tolist() == sorted(p | c << 32 for p, c in enumerate(codes.tolist()) if c >= 1000)
    assert M.list_as_bounds(M.wide_list(codes, 1000, 2047)) == {p: c for p, c in enumerate(codes.tolist()) if c >= 1000}
    assert M.escaped_count(codes, 2047) == 3


# ---- what the chooser does, against the figures of the header -------------------------------------------------------
def test_chooser_predictions():
    assert [M.index_bits(n) for n in (0, 1, 2, 3, 1 << 24, (1 << 24) + 1, 1 << 25, (1 << 25) + 1, (1 << 26) + 4097, (1 << 32) - 1)] == \
        [1, 1, 1, 2, 24, 25, 25, 26, 27, 32]
    assert [M.window_bits_of(nb) for nb in (1, 24, 25, 26, 27, 30)] == [10, 10, 10, 10, 11, 14]
    assert M.two_passes(30) and not M.two_passes(31)
    # big: a target beyond 2^24 words and more than 2^22 pairs
    assert not M.is_big(1 << 24, 1 << 24) and M.is_big((1 << 24) + 1, (1 << 22) + 1) and not M.is_big((1 << 24) + 1, 1 << 22)
    # the code field: 64 - nb - wb - 8 bits -- 72 - 2 * nb from 26 index bits up, 21 at 25 (text_order.hpp), 12 at 2^30 targets
    assert [M.esc_threshold(n) for n in ((1 << 24) + 1, 1 << 25, (1 << 25) + 1, (1 << 26) + 4097, 1 << 30)] == \
        [(1 << 21) - 1, (1 << 21) - 1, (1 << 20) - 1, (1 << 18) - 1, (1 << 12) - 1]
    assert all(64 - nb - M.window_bits_of(nb) - 8 == 72 - 2 * nb for nb in range(26, 31))
    assert M.esc_threshold(1 << 25, 100) == 100 and M.esc_threshold(1 << 30, 1 << 20) == (1 << 12) - 1
    assert M.exc_capacity(1000) == 1024 and M.exc_capacity(1 << 25) == 1 << 19
    n = (1 << 24) + 4097
    f = lambda *a, **k: M.expected_form(*a, **k)["form"]  # noqa: E731
    assert f(n, n) == "window_perm" and f(n, n, want_out2=True) == "packed" and f(n, n, want_out2=True, short_codes=False) == "two_value_hist"
    assert f(n, n, want_out2=True, hist_knob=True) == "two_value_hist" and f(n, n, want_out2=True, plan=True) == "record_plan2"
    assert f(n, n, want_out2=True, escaped=M.exc_capacity(n)) == "packed" and f(n, n, want_out2=True, escaped=M.exc_capacity(n) + 1) == "two_value_hist"
    assert M.expected_form(n, n, want_out2=True, narrow=True, escaped=M.exc_capacity(n) + 1) == \
        {"form": "none", "packed_tried": True, "list_overflow": True, "result": False, "partition_passes": 0}
    assert f(1 << 24, 1 << 24, want_out2=True) == "plain" and f(1 << 24, 1 << 24, want_out2=True, narrow=True) == "none"
    assert f(n, 1 << 22) == "plain" and f(n, (1 << 22) + 1) == "partial_then_plain"
    assert M.expected_form((1 << 27) + 4097, (1 << 22) + 77)["partition_passes"] == 2 and M.expected_form(n, n - 1)["partition_passes"] == 1
    assert f(100, 100, plan=True) == "record_plan" and f(100, 0) == "none"
    assert [M.expected_permute_form(c) for c in M.PERMUTE_COUNTS] == ["permute_plain"] * 3 + ["permute_windows"] * 3
    assert M.plan_is_made((1, 1), 1) and not M.plan_is_made((5,), 1) and not M.plan_is_made((5, (1 << 22) + 1), 1)
    assert M.plan_is_made((1 << 22, 5), 1) and not M.plan_is_made((100, 100), 1 << 16) and M.plan_is_made(M.DEFAULT_RECORDS, 1 << 16)


# ---- the generators meet their own conditions ---------------------------------------------------------------------
def is_permutation(idx, n):
    if idx.size != n or (n and int(idx.max()) >= n):
        return False
    seen = np.zeros(n, dtype=bool)   # n values below n that name every target: each once
    seen[idx] = True
    return bool(seen.all())


PERMUTATION_CASES = [c for c in all_gpu_cases() if c.rec_lens is None and c.partial is None]
PERMUTATION_SHAPES = sorted({(c.n_out, c.kind) for c in PERMUTATION_CASES})


@pytest.mark.parametrize("n,kind", PERMUTATION_SHAPES)
def test_permutations_are_permutations(n, kind):
    assert all(c.count == c.n_out for c in PERMUTATION_CASES) and len(PERMUTATION_SHAPES) >= 10
    p = M.permutation(n, kind)
    assert is_permutation(p, n)
    inv = M.inverse(n, kind)
    probe = np.arange(0, n, max(n // 1000, 1))
    assert (p[inv[probe]] == probe).all()
    M.permutation.cache_clear()
    M.inverse.cache_clear()


def test_partial_indices_are_free_of_duplicates_and_drop_some():
    cases = [c for c in all_gpu_cases() if c.partial is not None]
    assert len(cases) >= 17
    seen = set()
    for c in cases:
        if (c.n_out, c.count, c.partial) in seen:
            continue
        seen.add((c.n_out, c.count, c.partial))
        idx = M.partial_indices(c.n_out, c.count, c.partial)
        below = idx[idx < c.n_out]
        assert idx.size == c.count and np.unique(idx).size == c.count, c      # (none twice, dropped ones included)
        dropped = c.count - below.size
        assert 2 <= dropped and (c.count < 1000 or c.count // 40 <= dropped <= c.count // 5), (c, dropped)
        assert c.n_out in idx and 0xffffffff in idx
        if c.partial == "cluster":
            w = (c.n_out >> M.PARTIAL_WINDOW_BITS) // 2
            head = idx[:1 << M.PARTIAL_WINDOW_BITS]
            assert ((head >> M.PARTIAL_WINDOW_BITS) == w).all() and ((below >> M.PARTIAL_WINDOW_BITS) == w).sum() == 1 << M.PARTIAL_WINDOW_BITS
        elif c.count > 1 << 20:   # spread: every window of 2^19 targets is named, the last (partial) one too
            assert np.unique(below >> M.PARTIAL_WINDOW_BITS).size == (c.n_out - 1 >> M.PARTIAL_WINDOW_BITS) + 1


def test_record_layouts_are_block_diagonal_with_each_separator_first():
    cases = [c for c in all_gpu_cases() if c.rec_lens is not None]
    lens_seen = {c.rec_lens for c in cases}
    assert {1, 63, 64, 65, 4095, 4096, 4097, 1 << 14, (1 << 14) + 1, 1 << 22} <= set(M.MIXED_RECORDS)
    assert any(len(x) == 2 for x in lens_seen) and any(max(x) == (1 << 22) + 1 for x in lens_seen)
    assert any(sum(x) + len(x) - 1 > 1 << 24 for x in lens_seen) and any(sum(x) + len(x) - 1 < 1 << 24 for x in lens_seen)
    for lens in sorted(lens_seen):
        idx, ends = M.record_layout(lens)
        n = sum(lens) + len(lens) - 1
        assert is_permutation(idx, n) and ends[-1] == n and len(ends) == len(lens)
        start = 0
        for k, length in enumerate(lens):
            last = k + 1 == len(lens)
            if not last:
                assert idx[start] == start + length == ends[k]          # the separator: the first rank of its record
            ranks = idx[start + (0 if last else 1):start + length + (0 if last else 1)]
            assert ranks.size == length and int(ranks.min()) == start and int(ranks.max()) == start + length - 1
            start += length + (0 if last else 1)
    # the swapped input is a permutation still, and the separator of record 1 is no longer the first of its record
    c = M.separator_error_case()
    idx, _, ends = c.arrays()
    r = int(ends[0]) + 1
    assert is_permutation(idx, c.n_out) and idx[r] != ends[1] and idx[r + 1] == ends[1]


# ---- the two caps of the packed-form cases ----------------------------------------------------------------------------
@pytest.mark.parametrize("knob", [None, M.ESC_KNOB])
def test_escape_counts_of_the_many_and_overflow_inputs(knob):
    for n in M.BIG_SIZES if knob is None else M.BIG_SIZES[::3]:   # (the knob gives one threshold to every size)
        esc, cap = M.esc_threshold(n, knob), M.exc_capacity(n)
        assert cap == max(n // 64, 1024)
        many = M.escaped_count(M.packed_codes(n, "many", esc), esc)
        over = M.escaped_count(M.packed_codes(n, "overflow", esc), esc)
        assert 10_000 <= many <= cap < over, (n, many, cap, over)
        assert M.escaped_count(M.packed_codes(n, "below", esc), esc) == 0
    n = M.BIG_SIZES[0]
    esc = M.esc_threshold(n, knob)
    planted = M.packed_codes(n, "planted", esc)
    assert all((planted == v).sum() >= 8 for v in (esc - 1, esc, esc + 1, 0xffffffff))
    assert 24 <= M.escaped_count(planted, esc) <= 200
    M.permutation.cache_clear()
    M.inverse.cache_clear()


@pytest.mark.parametrize("knob", [None, M.ESC_KNOB])
def test_16_bit_inputs_fit_the_exception_list_and_straddle_both_bounds(knob):
    for n, code_max, cap in M.NARROW_SHAPES:
        esc = M.esc_threshold(n, knob)
        val = M.narrow_code_values(n, code_max, esc)
        assert M.escaped_count(val, esc) <= M.exc_capacity(n)
        assert all((val == v).any() for v in (code_max - 1, code_max, code_max + 1, esc - 1, esc, esc + 1, 0xffffffff))
        listed = len(M.wide_list(val, code_max, esc))
        assert (100 < listed <= 1 << 16) and cap in (100, 1 << 16)     # one capacity holds them, the other does not


# ---- for each plausible mistake, an input of the GPU list that tells ------------------------------------------------------
def differs(a, b):
    return a is not None and not np.array_equal(a, b)


TELLS = {   # mistake -> (case of the GPU list, what of its expected result differs)
    "rank_without_plus_one": ("small_perm_63", "out2"),
    "window_mask_one_bit_short": (f"window_{(1 << 24) + 1}_keep11", "out"),
    "last_partial_window_dropped": (f"window_{(1 << 24) + 1}_keep11", "out"),
    "escape_on_greater": (f"packed_{(1 << 24) + 1}_planted", "escaped"),
    "halves_swapped": ("permute_4097", "out"),
    "dropped_written_modulo": ("small_partial_4097_3000", "out"),
    "untouched_zeroed": ("small_partial_4097_3000", "out"),
    "keep_val_ignored": (f"window_{(1 << 24) + 1}_keep11", "val_after"),
    "separator_to_rank": ("records_two_only_2", "out"),
    "saturation_at_max_minus_one": (f"narrow_{(1 << 24) + 4097}_max1000_cap{1 << 16}", "narrow"),
}


@pytest.mark.parametrize("mistake", M.MISTAKES)
def test_each_mistake_is_told_by_an_input_of_the_gpu_list(mistake):
    name, key = TELLS[mistake]
    case = named(name)
    arrays = case.arrays()
    right, wrong = M.expected(case, arrays=arrays), M.expected(case, mistake=mistake, arrays=arrays)
    if key == "val_after":   # the input that must survive is not what a ping-pong buffer would hold after the passes
        assert right["val_survives"] and differs(wrong["val_after"], arrays[1])
    elif key == "escaped":
        assert right["escaped"] != wrong["escaped"] and right["form"] == "packed"
    else:
        assert differs(wrong[key], right[key])
    if mistake == "escape_on_greater":   # ... and in the 16-bit form the list tells as well
        c16 = named(f"narrow_{(1 << 24) + 4097}_max1000_cap{1 << 16}")
        val = M.narrow_code_values(c16.n_out, 1000, c16.esc())
        assert len(M.wide_list(val, 1000, c16.esc())) != len(M.wide_list(val, 1000, c16.esc(), mistake))
    if mistake == "last_partial_window_dropped":   # every size of the window forms has a partial last window but 2^25
        assert [n % 1024 for n in M.BIG_SIZES] == [1, 1, 0, 1] and M.WB11_SIZE % 2048 == 1
    M.permutation.cache_clear()
    M.inverse.cache_clear()


def test_the_mistakes_are_all_named():
    assert set(TELLS) == set(M.MISTAKES) and len(M.MISTAKES) == 10
