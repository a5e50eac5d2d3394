"""The greedy cursor (chain.hip: chain_exit_kernel, the node graph, wyllie_kernel, tile_entries_kernel, chain_mark_kernel,
emit_positions_kernel, length_hist_kernel, gather_lengths_kernel), the widening of 16-bit codes (lpnf.hip:
widen_codes_kernel, apply_wide_codes_kernel) and the per-range count on caller codes, through nolzss_debug_chain -- the
production functions mark_chain, chain_starts, chain_lengths, widened_lstar and rlz_count_per_target -- against the model
of tests/chain_model.py by integer equality: z, the starts, the lengths, the histogram, the tail list (sorted), the
widened array, the counts.  tests/test_chain_model_host.py proves without a GPU that the model's stages give the
definition on every input, and what every input is there for.

The inputs (chain_model.CASES), at most 131 073 positions per call; every one with 32-bit codes, and with 16-bit codes
(padding poisoned with 0x0000 and with 0xffff) wherever all codes lie below 0xffff:
  sizes        n = 1 .. 3 * 4096 + 1 on and around 64 and the tile, from start positions 0, 1, 2, 4095 .. 4097, odd, n - 1, n, n + 5
  literals     all codes 0 and all codes 1 over 1 .. 32 whole tiles and one position more: one node per tile, K + 1 on both
               sides of the powers of two of the Wyllie round count, all twelve doubling rounds, full bitmap words
  constant     L = 2 from an even and an odd start; L = 4095, 4096, 4097 over nine tiles
  seams        codes at offset 4095 and 0 of a tile that end on, behind and tiles behind the seam; 0xfffe from both, into a
               whole and into a partial last tile; one factor over the whole text
  realistic    ramps of copies over literals (code[i + 1] >= code[i] - 1), heavy tail up to 20 000
  adversarial  independent uniform codes in [0, 8], [0, 5000], [4096, 8191], [0, 0xfffe]: thousands of nodes
  strand       bit 31 on half of the non-zero codes, histogram and tail split by it
  bins         chains of factors of 2047, of 2048 and of 2047 / 2048 / 1
  overshoot    a last code that runs past n (z and the starts only)
  widening     n = 1, 2, 7, 4097 saturated at 0xffff and at 64: one entry, two in either order, positions beyond n, a
               list longer than `listed`, listed = 0; then the cursor over the widened array
  ranges       counts of the starts in empty, single-position, touching and whole-text ranges, and k = 0
"""
import numpy as np
import pytest

import chain_model as M

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def native():
    from nolzss_amd import _noLZSS as native
    assert native.device_count() >= 1, "no MI355X visible"
    return native


def run_one(native, name, width, poison=0):
    """one call of the hook, everything it returns against the model"""
    c, exp = M.case(name), M.expected(name, width)
    full = c.compare == "all" and (width == 32 or c.widening is not None)  # (the length kernels read 32-bit codes)
    kw = {}
    if c.widening is not None:
        kw = dict(wide_list=c.widening[0], listed=c.widening[1], list_max=c.widening[2])
    got = native.debug_chain(c.codes, c.start, width, poison, with_strand=c.with_strand, bounds=c.bounds, want_lengths=full,
                             want_hist=full, **kw)
    where = (name, width, hex(poison))
    assert got["z"] == exp["z"], (where, got["z"], exp["z"])
    for key in ("starts", "widened", "counts") + (("lengths", "hist", "tail") if full else ()):
        if exp[key] is None:
            assert got[key] is None, (where, key)
            continue
        assert got[key].shape == exp[key].shape, (where, key, got[key].shape, exp[key].shape)
        bad = np.nonzero(got[key] != exp[key])[0]
        assert bad.size == 0, (where, key, bad[:8].tolist(), got[key][bad[:8]].tolist(), exp[key][bad[:8]].tolist())
    return exp


def run_case(native, name):
    calls = 0
    for width in M.widths_of(name):
        for poison in (M.POISONS if width == 16 else (0,)):
            run_one(native, name, width, poison)
            calls += 1
    return calls


@pytest.mark.parametrize("n", M.SIZES)
def test_sizes_and_start_positions(native, n):
    for s in M.starts_for(n):
        run_case(native, f"size_{n}_s{s}")


@pytest.mark.parametrize("name", M.FAMILIES["literals"])
def test_literals_and_ones(native, name):
    run_case(native, name)


@pytest.mark.parametrize("name", M.FAMILIES["constant"])
def test_constant_lengths(native, name):
    run_case(native, name)


@pytest.mark.parametrize("name", M.FAMILIES["seams"])
def test_tile_seams(native, name):
    run_case(native, name)


@pytest.mark.parametrize("name", M.FAMILIES["realistic"])
def test_realistic_codes(native, name):
    run_case(native, name)


@pytest.mark.parametrize("name", M.FAMILIES["adversarial"])
def test_adversarial_codes(native, name):
    run_case(native, name)


@pytest.mark.parametrize("name", M.FAMILIES["strand"])
def test_strand(native, name):
    assert run_case(native, name) == 1  # (bit 31: 32-bit codes only)


@pytest.mark.parametrize("name", M.FAMILIES["bins"])
def test_lengths_at_the_bin_boundary(native, name):
    run_case(native, name)


@pytest.mark.parametrize("name", M.FAMILIES["overshoot"])
def test_overshoot(native, name):
    run_case(native, name)


@pytest.mark.parametrize("name", M.FAMILIES["widening"])
def test_widening(native, name):
    assert run_case(native, name) == 2


@pytest.mark.parametrize("name", M.FAMILIES["ranges"])
def test_per_range_counts(native, name):
    run_case(native, name)


def test_a_call_leaves_no_state_behind(native):
    """narrow, wide, widened and narrow again, a large input between small ones"""
    for name, width, poison in (("size_65_s1", 16, 0xffff), ("lit_t32_p1", 32, 0), ("widen_4097_m64_two_large_first", 16, 0),
                                ("size_65_s1", 16, 0), ("adv_49155_4096_8191_s0", 16, 0xffff), ("size_1_s0", 32, 0)):
        run_one(native, name, width, poison)


def test_lengths_of_16_bit_codes_are_refused_by_the_stage_itself(native):
    codes = M.case("size_4097_s0").codes
    for kw in (dict(want_lengths=True, want_hist=False), dict(want_lengths=False, want_hist=True)):
        with pytest.raises(RuntimeError, match="the length kernels read 32-bit codes"):
            native.debug_chain(codes, 0, 16, **kw)
    assert native.debug_chain(codes, 4097, 16)["z"] == 0          # nothing to take lengths of: no stage is reached
    run_one(native, "size_4097_s0", 16)                           # ... and the call behind a refusal is served


def test_bad_arguments_are_refused(native):
    codes = np.array([3, 0, 0, 2, 0, 1, 0], dtype=np.uint32)
    got = native.debug_chain(codes, 0, 16, 0xffff, want_lengths=False, want_hist=False)
    assert got["z"] == 4 and got["starts"].tolist() == [0, 3, 5, 6]
    bad = [
        dict(width=8), dict(width=16, poison=0x10000),
        dict(codes=[3, 0, 0xffff], width=16),                                     # the saturation value among 16-bit codes
        dict(width=32, wide_list=[3 | (9 << 32)], list_max=64),                   # a list with 32-bit codes
        dict(width=16, wide_list=[3 | (9 << 32)], listed=2, list_max=64),         # listed beyond the list
        dict(width=16, wide_list=[3 | (9 << 32)]),                                # a list without its saturation value
        dict(width=16, list_max=2),                                               # a code above the saturation value
        dict(bounds=[0, 3, 2, 7]), dict(bounds=[0, 3, 7]),                        # descending, odd
    ]
    for kw in bad:
        kw = dict(dict(codes=codes, want_lengths=False, want_hist=False), **kw)
        with pytest.raises(ValueError):
            native.debug_chain(**kw)
    empty = native.debug_chain(np.zeros(0, dtype=np.uint32), 0, 32)
    assert empty["z"] == 0 and empty["starts"].size == 0 and not empty["hist"].any() and empty["tail"].size == 0
