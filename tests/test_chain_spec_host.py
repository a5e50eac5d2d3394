"""The model of the speculative cursor (tests/chain_spec_model.py) against the definition (chain_model.cursor), without a
GPU: the three steps give the definition on every input of tests/test_gpu_chain_spec.py whenever no tile fails; every
input takes the path and fails the tiles that its case states; the inputs are what their names say (where the walk from
the entry lands, what is cleared); and each named mistake of the steps changes the result on the inputs that are there
for it:
  keep_below_m       a head fix that keeps the marks of step 1 in front of the position where the walks meet
  accept_any_exit    a head fix that accepts a walk which leaves the tile elsewhere than the speculative walk did
  follow_unreached   a tile path that hands on the exit of a tile the chain never enters
"""
import numpy as np
import pytest

import chain_model as M
import chain_spec_model as S

TILE = S.TILE


@pytest.mark.parametrize("name", list(S.CASES))
def test_the_steps_give_the_definition_and_the_stated_path(name):
    c = S.case(name)
    assert c.codes.size <= 131073
    st = S.staged(c.codes, c.start)
    starts, path, failed = S.run(c.codes, c.start)
    assert (path, failed) == (c.path, c.failed), (name, path, failed)
    truth = M.cursor(c.codes, c.start)
    assert np.array_equal(starts, truth)
    if not st["failed"]:  # no fall-back was needed: the three steps alone are exact
        assert np.array_equal(st["starts"], truth)
    assert np.array_equal(S.expected(name)["starts"], truth)


def test_the_inputs_are_what_their_names_say():
    merges = lambda name: S.staged(S.case(name).codes, S.case(name).start)["merges"]  # noqa: E731
    for name in ("entry_is_tile_start_twos", "entry_is_tile_start_literals"):
        assert merges(name) == {}
    assert merges("merge_hop0_offset1") == {1: (0, 1)} and merges("merge_hop0_offset777") == {1: (0, 777)}
    for x in (63, 64, 1023, 1024, 4095):
        assert merges(f"merge_first_hop_{x}")[1] == (1, x)
        hops, m = merges(f"merge_far_{x}")[1]
        assert m == x and hops == (x - (2 if x % 2 else 1)) // 2 + 1
    assert merges("merge_far_4095")[2] == (1, 2)                      # the tile behind is entered at offset 1
    assert merges("merge_far_1024")[1] == (512, 1024)                 # the first position behind the first 1024 codes
    assert merges("leaves_at_spec_exit") == {1: (2048, None)}
    assert S.staged(S.case("leaves_at_spec_exit").codes, 5)["cleared"] == 2048
    assert merges("leaves_beside_spec_exit") == {1: (2048, None)}
    assert merges("partial_tile_last_position") == {2: (1, None)} and merges("partial_tile_last_position_marked") == {2: (0, 99)}
    for name in ("jumped_tiles_literals", "jumped_tiles_ramps"):
        c = S.case(name)
        st = S.staged(c.codes, c.start)
        truth = M.cursor(c.codes, c.start)
        assert st["cleared"] > 4 * 100 and 5 in st["merges"] and not ((truth >= TILE) & (truth < 5 * TILE)).any()
    assert S.staged(S.case("lands_20_tiles_on").codes, 3)["reached"] == 6 and S.widths_of("lands_20_tiles_on") == (32,)
    assert S.widths_of("whole_text_16") == (32, 16) and S.widths_of("whole_text_32") == (32,)
    assert S.case("start_mid_tile").start // TILE == 2 and S.case("start_mid_tile").start % TILE
    for name in S.CASES:
        if name.startswith("ramps_"):
            codes = S.case(name).codes.astype(np.int64)
            assert (codes[1:] >= codes[:-1] - 1).all()
            st = S.staged(S.case(name).codes, S.case(name).start)
            assert st["failed"] == 0 and len(st["merges"]) >= 8, (name, len(st["merges"]))
        if name.startswith("dense_ramps_"):
            codes = S.case(name).codes.astype(np.int64)
            assert (codes[1:] >= codes[:-1] - 1).all()
            st = S.staged(S.case(name).codes, S.case(name).start)
            hops = [h for h, _ in st["merges"].values()]
            assert st["failed"] == 0 and len(hops) >= 24 and max(hops) >= 3, (name, hops)


def _wrong(name, bug):
    c = S.case(name)
    return not np.array_equal(S.run(c.codes, c.start, bug)[0], M.cursor(c.codes, c.start))


def test_every_mistake_is_exposed():
    for x in (63, 64, 1023, 1024, 4095):
        assert _wrong(f"merge_first_hop_{x}", "keep_below_m") and _wrong(f"merge_far_{x}", "keep_below_m")
    assert _wrong("merge_hop0_offset1", "keep_below_m") and _wrong("leaves_at_spec_exit", "keep_below_m")
    assert sum(_wrong(n, "keep_below_m") for n in S.CASES if n.startswith(("ramps_", "dense_ramps_"))) == 10
    for name in ("leaves_beside_spec_exit", "twos_from_odd_start", "twos_from_odd_start_5_tiles", "interleaved_far_exits",
                 "start_mid_tile_twos", "uniform_0_5000", "uniform_0_fffe"):
        assert _wrong(name, "accept_any_exit"), name
    for name in ("jumped_tiles_literals", "jumped_tiles_ramps", "lands_20_tiles_on", "whole_text_16", "whole_text_32"):
        assert _wrong(name, "follow_unreached"), name
    assert not any(_wrong(name, None) for name in S.CASES)  # ... and by nothing but the mistake
