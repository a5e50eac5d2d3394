"""The pair-run pass and the periodic pass of the suffix-array construction (sa_repeats.hip, 17 kernels, and the
regroup<false> behind the periodic pass) and count_large_groups on caller states, through nolzss_debug_repeat_pass --
periodic_pass and pair_run_pass of the construction themselves, behind the driver's own set_up_late_rounds -- against the
round-level models of tests/sa_repeats_model.py by integer equality: sa, lcp (pending codes included) and rank over all
entries, the next active list and its length, the four counts, the return value, per_hint and per_attempts.  On top of
that every output of the GPU must be a refinement of the state that went in under the TRUE suffix and LCP arrays
(check_refinement, which knows nothing of the models): a misreading that the model shares with the kernels still fails.
tests/test_sa_repeats_model_host.py proves without a GPU that the true arrays are those of the definition, that the
models' outputs are such refinements, that every branch is reached and what every input is there for.

The inputs (sa_repeats_model.CASES), 120 to 12 400 symbols at 2, 4 and 8 bits per symbol, one of 2^20 + 300:
  pr_xx_*, pr_xxc, pr_xyx      XX whose run ends with the text (everything deferred, over 1 and 3 passes), XX and one more
                               symbol, XX of DNA at depth 20, XYX
  pr_three_1 .. _3             three copies, one differs behind the run: 1, 2 and 3 passes
  pr_copies_*, pr_*_splits     2, 3, 15, 16 and 17 copies; a group of exactly 16 (and of 17) that splits into classes, next to
                               other groups; pr_only_large: nothing but groups of 20
  pr_nested, pr_overlap        repeats whose group size or link distance changes mid-run
  pr_partly*                   an end group that separates into classes that stay tied (1 pass), finished by 3
  pr_mixed_depth, pr_compared* groups refined to different depths side by side; kLcpPendingCompared inside groups;
                               lcp[n] = 0xffffffff, 0 and 12345
  pr_w4, pr_w8, pr_periodic_text
  per_p1 .. p23                periods 1, 2, 3, 7, 23 with breaks up, down and at the end of the text
  per_two_runs, per_q_*        two runs of one unit in one group; q == depth and depth + 1; q = 4096 (taken) and 4097
                               (flagged, hint), three periods each; per_q4096_tail: flagged by the run check
  per_lookalike*, per_tied_E*  U^40 V^40; E and E + q tied with each other (q > depth and q == depth); per_short_run
  per_text_end*                the text ends inside a period
  per_link_paths, per_m*       groups of 684, 172 and few members: all reductions of per_link_kernel; lists of 255, 256, 257
  per_first_*, per_cand_*, per_attempts_3
                               the gate of the first call (taken and passed), cand < m / 16 and just above, attempts = 3
  per_mixed_depth, per_w4, per_w8, per_segmented (terminators: no text check, qmax = depth), per_big (A^(2^20) C A^299)
  cnt_*                        groups of 16 and 17, neighbours 4096 and 4097 apart
A pending range minimum (`lam`) has no case: the head entry of the upper group ends every range and is decided in every
state the hook accepts.

Out of scope: reverse-complement (mirrored) texts and merged batches -- the hook takes bytes only -- and the stride of the
sweep kernels beyond 4 M threads, which tests/test_gpu_scale.py keeps, end to end.
"""
import numpy as np
import pytest

import sa_repeats_model as R

pytestmark = pytest.mark.gpu

ARRAYS = ("sa", "lcp", "rank", "new_slot", "new_grp")
SCALARS = ("new_m", "counts", "ret", "per_hint", "per_attempts")


@pytest.fixture(scope="module")
def native():
    from nolzss_amd import _noLZSS as native
    assert native.device_count() >= 1, "no MI355X visible"
    return native


def call(native, name, order):
    c = R.CASES[name]
    text, st = R.made(name)[0], R.state(name, order)
    return native.debug_repeat_pass(text.data, st.sa, st.lcp, st.rank, st.slot, st.grp, c.h, c.which, c.arg)


def run_one(native, name, order):
    """one call of the hook: the refinement property of what the GPU returned, then everything against the model"""
    text, truth = R.made(name)
    st, exp = R.state(name, order), R.expected(name, order)
    got = call(native, name, order)
    where = (name, order)
    assert (got["bits"], got["terms"], got["segmented"]) == (text.bits, text.terms.size, text.segmented), where
    print(f"{where}: m {st.slot.size} -> {got['new_m']} (model {exp['new_m']}), counts {got['counts']} (model {exp['counts']}), "
          f"ret / hint / attempts {got['ret']} {got['per_hint']} {got['per_attempts']} "
          f"(model {exp['ret']} {exp['per_hint']} {exp['per_attempts']})")
    R.check_refinement(truth, st, got, where)
    for k in SCALARS:
        assert got[k] == exp[k], (where, k, got[k], exp[k])
    for k in ARRAYS:
        bad = np.nonzero(got[k] != exp[k])[0]
        assert bad.size == 0, (where, k, bad[:8].tolist(), got[k][bad[:8]].tolist(), exp[k][bad[:8]].tolist())
    return got


@pytest.mark.parametrize("name", list(R.CASES))
def test_pass_matches_the_model(native, name):
    for order in R.CASES[name].orders:
        run_one(native, name, order)


def test_lcp_n_is_never_read(native):
    """the entry behind the last slot goes in as the caller gives it, comes back untouched and changes nothing else"""
    for name, order in (("pr_three_2", "shuffle"), ("per_p7", "shuffle")):
        c = R.CASES[name]
        text, st = R.made(name)[0], R.state(name, order)
        exp = R.expected(name, order)
        for last in (0, 1, 0x12345678, R.COMPARED):
            lcp = st.lcp.copy()
            lcp[-1] = last
            got = native.debug_repeat_pass(text.data, st.sa, lcp, st.rank, st.slot, st.grp, c.h, c.which, c.arg)
            assert got["lcp"][-1] == last and np.array_equal(got["lcp"][:-1], exp["lcp"][:-1])
            assert all(np.array_equal(got[k], exp[k]) for k in ARRAYS if k != "lcp") and all(got[k] == exp[k] for k in SCALARS)


def test_a_call_leaves_no_state_behind(native):
    """one case three times, with other passes, widths and sizes in between"""
    first = run_one(native, "per_mixed_depth", "shuffle")
    run_one(native, "pr_w8", "reversed")
    second = run_one(native, "per_mixed_depth", "shuffle")
    run_one(native, "per_attempts_3", "text")
    run_one(native, "per_q4097", "shuffle")
    run_one(native, "cnt_17", "text")
    third = run_one(native, "per_mixed_depth", "shuffle")
    for other in (second, third):
        assert all(np.array_equal(first[k], other[k]) for k in ARRAYS) and all(first[k] == other[k] for k in SCALARS)
    a = run_one(native, "pr_partly_3", "reversed")
    run_one(native, "per_first_gate", "shuffle")
    b = run_one(native, "pr_partly_3", "reversed")
    assert all(np.array_equal(a[k], b[k]) for k in ARRAYS) and all(a[k] == b[k] for k in SCALARS)


def test_bad_arguments_are_refused(native):
    P = R.PENDING
    text = b"ACGTACGTACGTACGTAACC"   # (the state need not be true: everything here is refused on the host, or counted only)
    n = 20
    sa = np.arange(n, dtype=np.uint32)
    lcp = np.array([0, 1, 2, 3, P, 5, 6, 7, P, P] + list(range(10, 20)) + [P], dtype=np.uint32)   # groups {3, 4} and {7, 8, 9}
    rank = np.array([1, 2, 3, 4, 4, 6, 7, 8, 8, 8] + list(range(11, 21)), dtype=np.uint32)
    ok = dict(text=text, sa=sa, lcp=lcp, rank=rank, slot=[3, 4, 7, 8, 9], grp=[3, 3, 7, 7, 7], h=1, which=R.COUNTS, arg=0)
    got = native.debug_repeat_pass(**ok)
    assert got["counts"] == [0, 0, 2, 3] and got["new_m"] == 5 and got["new_slot"].tolist() == [3, 4, 7, 8, 9]
    assert np.array_equal(got["sa"], sa) and np.array_equal(got["lcp"], lcp) and np.array_equal(got["rank"], rank)
    none = native.debug_repeat_pass(text, sa, list(range(21)), list(range(1, 21)), [], [], 1, R.COUNTS)   # nothing tied
    assert none["counts"] == [0, 0, 0, 0] and none["new_m"] == 0

    def changed(arr, at, value):
        out = arr.copy()
        out[at] = value
        return out
    bad = [
        dict(ok, text=b"", sa=sa[:0], lcp=lcp[:1], rank=rank[:0], slot=[], grp=[]),   # no text
        dict(ok, which=3), dict(ok, which=-1),                          # another pass
        dict(ok, arg=1),                                                # the counts take no argument
        dict(ok, which=R.PERIODIC, arg=4), dict(ok, which=R.PERIODIC, arg=-1),
        dict(ok, which=R.PAIR_RUNS, arg=0), dict(ok, which=R.PAIR_RUNS, arg=11),
        dict(ok, slot=[7, 8, 9, 3, 4], grp=[7, 7, 7, 3, 3]),            # the list is not in ascending slot order
        dict(ok, slot=[3, 4, 4, 8, 9], grp=[3, 3, 3, 8, 8]),            # a slot twice
        dict(ok, slot=[3, 5, 7, 8, 9], grp=[3, 3, 7, 7, 7]),            # a group with a hole in its slots
        dict(ok, slot=[4, 5, 7, 8, 9], grp=[3, 3, 7, 7, 7]),            # a group that does not start at its head slot
        dict(ok, slot=[3, 4, 7, 8, 9], grp=[4, 4, 7, 7, 7]),            # grp > slot
        dict(ok, slot=[3, 4, 7, 8, 20], grp=[3, 3, 7, 7, 7]),           # slot >= n
        dict(ok, slot=[3, 4, 7, 8, 9], grp=[3, 3, 7, 8, 8]),            # a listed group of one member
        dict(ok, slot=[3, 4, 7, 8, 12], grp=[3, 3, 7, 7, 12]),          # ... at the end of the list
        dict(ok, slot=[3, 4, 7, 8], grp=[3, 3, 7, 7]),                  # a slot inside a group (by lcp) that is not listed
        dict(ok, slot=[3, 4], grp=[3, 3]),                              # ... a whole group
        dict(ok, slot=[3, 4, 7, 8, 9, 12, 13], grp=[3, 3, 7, 7, 7, 12, 12]),   # a listed group that lcp does not know
        dict(ok, sa=changed(sa, 5, 6)),                                 # sa is no permutation
        dict(ok, sa=changed(sa, 5, 20)),                                # ... a suffix that is none
        dict(ok, rank=changed(rank, 4, 5)),                             # rank is not the head slot + 1 (a member)
        dict(ok, rank=changed(rank, 15, 15)),                           # ... (a finished suffix)
        dict(ok, rank=changed(rank, 0, 0)),
        dict(ok, lcp=changed(lcp, 8, 4)),                               # a decided entry inside a listed group
        dict(ok, lcp=changed(lcp, 7, P)),                               # a pending entry at the head of a listed group
        dict(ok, lcp=changed(lcp, 0, P)),                               # lcp[0] pending
        dict(ok, lcp=changed(lcp, 15, R.COMPARED)),                     # a pending entry among the finished suffixes
        dict(ok, sa=sa[:19]), dict(ok, lcp=lcp[:20]), dict(ok, rank=rank[:19]), dict(ok, grp=[3, 3, 7, 7]),   # lengths that do not fit
    ]
    for kw in bad:
        with pytest.raises(ValueError):
            native.debug_repeat_pass(**kw)
    # every pending code counts as one: 0xffffffbf is the least
    low = native.debug_repeat_pass(**dict(ok, lcp=changed(changed(lcp, 4, R.PENDING_MIN), 8, R.COMPARED)))
    assert low["counts"] == [0, 0, 2, 3]
    with pytest.raises(ValueError):
        native.debug_repeat_pass(**dict(ok, lcp=changed(lcp, 4, R.PENDING_MIN - 1)))
    from nolzss_amd._lib import lib
    t = np.frombuffer(text, dtype=np.uint8)
    slot, grp = np.array(ok["slot"], dtype=np.uint32), np.array(ok["grp"], dtype=np.uint32)
    w_sa, w_lcp, w_rank = sa.copy(), lcp.copy(), rank.copy()
    new_slot, new_grp = np.zeros(5, dtype=np.uint32), np.zeros(5, dtype=np.uint32)
    new_m, counts, per = np.zeros(1, dtype=np.uint32), np.zeros(4, dtype=np.uint32), np.zeros(3, dtype=np.uint32)
    args = [t.ctypes.data, n, w_sa.ctypes.data, w_lcp.ctypes.data, w_rank.ctypes.data, slot.ctypes.data, grp.ctypes.data, 5, 1,
            R.COUNTS, 0, 0, new_slot.ctypes.data, new_grp.ctypes.data, new_m.ctypes.data, counts.ctypes.data, None, per.ctypes.data]
    assert lib.nolzss_debug_repeat_pass(*args) == 0
    for null_at in (0, 2, 3, 4, 5, 6, 12, 13, 14, 15, 17):
        a = list(args)
        a[null_at] = None
        assert lib.nolzss_debug_repeat_pass(*a) != 0, null_at
    for size in (0, 1 << 31, (1 << 31) + 5):   # (refused before anything is read: positions carry a flag in bit 31)
        a = list(args)
        a[1] = size
        assert lib.nolzss_debug_repeat_pass(*a) != 0, size
    a = list(args)
    a[7] = 21   # more list entries than suffixes
    assert lib.nolzss_debug_repeat_pass(*a) != 0
