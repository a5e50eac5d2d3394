"""The LDS tile searches (nearest_lds.hpp: stage_tile, build_block_tables, lds_search_wave_blocks), run on the device by
nolzss_debug_lds_search with the template arguments of the plain and of the reverse-complement candidate kernel, and
compared by integer equality with the brute-force numpy model (tests/lds_search_model.py).  The inputs are arrays, not
texts: one design whose first n ranks make the case of size n.  Each case asserts what it holds (lds_search_model.EXPECT):
searches that end at every distance from 17 to 272 -- so in every block of round B --, at every rank of the stopping
block of round C, in the first and the last block of the staged span, exactly at the last rank in reach and at the first
beyond it; a minimum that reaches 0 one block in front of the qualifying suffix; equal minima in two blocks; wavefronts
with 0, 1, 15, 16, 17, 32, 33 and 64 or more searches pending after round A, one way only and both ways; a last tile with
ranks past n.  Each runs with the padding behind the arrays poisoned with 0x00 and with 0xFF.
tests/test_lds_search_model_host.py shows that these inputs see the mistakes a lane-group rewrite of rounds B + C can make."""
import numpy as np
import pytest

import lds_search_model as M

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def native():
    from nolzss_amd import _noLZSS
    assert _noLZSS.device_count() >= 1, "no MI355X visible"
    return _noLZSS


def same(got, exp, what):
    got, exp = np.asarray(got), np.asarray(exp)
    assert got.shape == exp.shape, what
    bad = np.argwhere(got != exp)
    assert not len(bad), (what, len(bad), "first at (search, rank)", bad[0].tolist(), hex(int(got[tuple(bad[0])])),
                          hex(int(exp[tuple(bad[0])])))


@pytest.mark.parametrize("form", [M.PLAIN, M.RC], ids=["plain", "rc"])
@pytest.mark.parametrize("n", M.SIZES)
def test_searches(native, n, form):
    c = M.case(n)
    f = M.check_features(c, form)
    exp_len, exp_pos = M.answers(c.sa, c.lcp, form, M.STRAND)
    for poison in M.POISONS:
        got_len, got_pos = native.debug_lds_search(c.sa, c.lcp, form, M.STRAND, poison=poison)
        same(got_len, exp_len, (n, form, poison, "len"))
        same(got_pos, exp_pos, (n, form, poison, "pos"))
    print(f"n={n} form={form}: long searches per kind {[len(d) for d in f['distances']]} distances, "
          f"pending per wavefront (up, down) {f['wave_counts']}")


def test_refusals_come_back_as_errors(native):
    sa = np.arange(10, dtype=np.uint32)
    with pytest.raises(ValueError, match="lcp"):
        native.debug_lds_search(sa, np.ones(11, dtype=np.uint32))
    with pytest.raises(ValueError):
        native.debug_lds_search(sa, np.zeros(11, dtype=np.uint32), form=2)
    with pytest.raises(ValueError):
        native.debug_lds_search(sa, np.zeros(11, dtype=np.uint32), poison=0x55)
