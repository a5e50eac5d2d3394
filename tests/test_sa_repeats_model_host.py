"""What the inputs of tests/test_gpu_sa_repeats.py are there for, shown without a GPU (tests/sa_repeats_model.py):

  * the true arrays every state is cut from agree with the definition, Text.compare, pair by pair; the closed form for
    A^p C A^q agrees with the general construction;
  * every state the builder makes is a valid partial state, and every model output is a valid refinement of it
    (check_refinement): each new group a range of the true suffix array, every decided LCP the true one, ranks head + 1;
  * the model applied until nothing changes and finished by brute force gives the true arrays;
  * every named branch is reached by a named case, and the sizes and edges the cases are named after are really in them;
  * every named mistake changes the expected output of at least one case (printed), and the three that cannot change
    any output on a valid state change none.
"""
import functools
import time

import numpy as np
import pytest

import sa_repeats_model as R

SMALL = [(name, order) for name, order in R.runs() if name != "per_big"]


def test_true_arrays_agree_with_the_definition():
    for name in R.CASES:
        text, (sa, lcp) = R.made(name)
        n = text.n
        assert np.array_equal(np.sort(sa), np.arange(n)) and lcp[0] == 0 and lcp[n] == 0
        ranks = range(1, n) if n <= 20000 else np.random.default_rng(5).integers(1, n, 3000).tolist()
        for r in ranks:
            assert text.compare(int(sa[r - 1]), int(sa[r])) == (-1, int(lcp[r])), (name, r)


def test_closed_form_of_apcaq():
    for p, q in ((40, 7), (7, 40), (12, 12), (30, 0), (1, 1), (64, 63)):
        text = R.Text(b"A" * p + b"C" + b"A" * q)
        sa, lcp = R.true_arrays(text)
        sa2, lcp2 = R.true_arrays_apcaq(p, q)
        assert np.array_equal(sa, sa2) and np.array_equal(lcp, lcp2), (p, q)


def check_state(text, truth, st, h):
    """the builder's output is what the hook checks on the host -- and a true partial order of the text"""
    sa_t, lcp_t = truth
    n = text.n
    dec = st.lcp[:n] < R.PENDING_MIN
    assert dec[0] and np.array_equal(st.lcp[:n][dec], lcp_t[:n][dec])
    assert (lcp_t[:n][~dec] >= h).all(), "a group that does not agree on h symbols"
    hs = R._heads_of(st.lcp, n)
    assert np.array_equal(st.sa[np.lexsort((st.sa, hs))], sa_t[np.lexsort((sa_t, hs))])
    assert np.array_equal(st.rank[st.sa], hs + 1)
    slot, grp = R._listed(st.lcp, n)
    assert np.array_equal(slot, st.slot) and np.array_equal(grp, st.grp)


@pytest.mark.parametrize("name,order", R.runs())
def test_model_output_is_a_valid_refinement(name, order):
    c = R.CASES[name]
    text, truth = R.made(name)
    st = R.state(name, order)
    check_state(text, truth, st, c.h)
    t0 = time.perf_counter()
    exp = R.expected(name, order)
    print(f"{name} {order}: n {text.n}, m {st.slot.size} -> {exp['new_m']}, model {time.perf_counter() - t0:.2f} s")
    R.check_refinement(truth, st, exp, (name, order))
    if c.which == R.COUNTS:
        assert all(np.array_equal(exp[k], np.asarray(v).astype(np.uint32)) for k, v in (("sa", st.sa), ("lcp", st.lcp), ("rank", st.rank)))


def finish_by_brute_force(text, st):
    """every group that is left, sorted by Text.compare; the LCP of its boundaries from Text.lcp"""
    sa, lcp = st.sa.copy(), st.lcp.copy()
    heads = np.unique(st.grp)
    sizes = np.bincount(st.grp, minlength=sa.size)
    for g in heads:
        k = int(sizes[g])
        mem = sorted(sa[g:g + k].tolist(), key=functools.cmp_to_key(lambda a, b: text.compare(a, b)[0]))
        sa[g:g + k] = mem
        for j in range(1, k):
            lcp[g + j] = text.lcp(mem[j - 1], mem[j])
    return sa, lcp


@pytest.mark.parametrize("name,order", [(n, o) for n, o in SMALL if R.CASES[n].which != R.COUNTS and o != "reversed"])
def test_model_to_the_end_gives_the_true_arrays(name, order):
    c = R.CASES[name]
    text, (sa_t, lcp_t) = R.made(name)
    st = R.state(name, order)
    for _ in range(64):
        if c.which == R.PAIR_RUNS:
            nxt = R.pair_run_pass(st)[0]
        else:
            nxt = R.periodic_pass(text, st, c.h, 1, R.count_large(st))[0]
        same = all(np.array_equal(a, b) for a, b in zip(nxt, st))
        st = nxt
        if same:
            break
    else:
        raise AssertionError("the model does not settle")
    sa, lcp = finish_by_brute_force(text, st)
    assert np.array_equal(sa, sa_t) and np.array_equal(lcp[:text.n], lcp_t[:text.n])


def test_every_branch_is_reached_by_a_named_case():
    reached = {}
    for name, order in R.runs():
        for b in R.expected(name, order)["branches"]:
            reached.setdefault(b, name)
    for b in R.BRANCHES:
        print(f"{b}: {reached.get(b)}")
    assert set(reached) == set(R.BRANCHES)
    br = lambda name, order=None: R.expected(name, order or R.CASES[name].orders[0])["branches"]  # noqa: E731
    assert {"link:block", "link:wave", "link:mixed", "link:padding"} <= br("per_link_paths")
    assert br("per_m256") & {"link:block", "link:wave", "link:mixed", "link:padding"} == {"link:block"}
    assert "link:padding" in br("per_m255") and "link:padding" in br("per_m257")
    assert "gate:first_call" in br("per_first_gate") and "gate:first_call" not in br("per_first_pass")
    assert "gate:candidates" in br("per_cand_none") and "gate:candidates" not in br("per_cand_between")
    assert "gate:attempts" in br("per_attempts_3")
    assert "rho:tied_E" in br("per_tied_E") and "rho:text_end" in br("per_text_end_q_gt")
    assert "rho:short_run" in br("per_short_run") and "rho:short_run" in br("per_lookalike")
    assert "verify:text" in br("per_lookalike_len") and "verify:text" not in br("per_lookalike")
    assert "flags:hint" in br("per_q4097") and "flags:hint" not in br("per_q4096") and "flags:hint" in br("per_segmented")
    assert {"end:off_end", "end:off_end_other"} <= br("pr_xx_deferred") and "end:classes_tied" in br("pr_partly")


def test_the_cases_hold_what_they_are_named_after():
    def sizes(name, order=None):
        st = R.state(name, order or R.CASES[name].orders[0])
        return np.bincount(st.grp)[np.unique(st.grp)] if st.slot.size else np.zeros(0, dtype=np.int64)
    for k in (2, 3, 15, 16, 17):
        assert sizes(f"pr_copies_{k}").max() == k
    assert sizes("cnt_16").max() == 16 and sizes("cnt_17").max() == 17
    assert (sizes("pr_16_splits") == 16).any() and sizes("pr_16_splits").max() == 16 and (sizes("pr_17_splits") == 17).any()
    assert sizes("pr_only_large").min() > 16
    for name in ("pr_only_large", "pr_xx_deferred", "pr_xx_deferred_3", "per_first_gate", "per_cand_none", "per_attempts_3"):
        for order in R.CASES[name].orders:  # nothing may change
            st, exp = R.state(name, order), R.expected(name, order)
            assert exp["new_m"] == st.slot.size and np.array_equal(exp["sa"], st.sa) and np.array_equal(exp["lcp"], st.lcp), name
    assert [R.expected(f"pr_three_{k}", "shuffle")["new_m"] for k in (1, 2, 3)] == [220, 0, 0]
    assert 0 < R.expected("pr_partly", "text")["new_m"] and R.expected("pr_partly_3", "reversed")["new_m"] == 0
    for m in (255, 256, 257):
        assert R.state(f"per_m{m}", "reversed").slot.size == m
    assert R.expected("cnt_near_4096", "text")["counts"][3] == 84 and R.expected("cnt_near_4097", "text")["counts"][3] == 0
    assert R.expected("cnt_16", "text")["counts"][:2] == [0, 0] and R.expected("cnt_17", "text")["counts"][1] > 0
    assert R.expected("per_q4096", "shuffle")["per_hint"] == 0 and R.expected("per_q4097", "shuffle")["per_hint"] == 4097
    assert R.expected("per_q4096", "shuffle")["new_m"] == 0
    assert R.expected("per_segmented", "text")["per_hint"] == 8 and R.made("per_segmented")[0].segmented
    assert R.made("per_big")[0].n == (1 << 20) + 300
    assert {R.CASES[n].bits for n in R.CASES} == {2, 4, 8}
    for name in ("pr_mixed_depth", "per_mixed_depth"):  # groups of different depth side by side
        text, (_, lcp_t) = R.made(name)
        st = R.state(name, "shuffle")
        inside = lcp_t[:text.n][st.lcp[:text.n] >= R.PENDING_MIN]
        assert inside.min() >= R.CASES[name].h and np.unique(lcp_t[st.grp + 1] >= 2 * R.CASES[name].h).size == 2
    st = R.state("pr_compared", "shuffle")
    assert (st.lcp == R.COMPARED).any() and (st.lcp == R.PENDING).any() and st.lcp[-1] == 0
    cand = R.CASES["per_cand_between"]
    assert cand.which == R.PERIODIC and cand.arg == 1


def test_hook_is_exported():
    from nolzss_amd import _lib, _noLZSS
    header = open(_lib.__file__.replace("nolzss_amd/_lib.py", "include/nolzss_hip.h")).read()
    name = "nolzss_debug_repeat_pass"
    assert name in _lib.EXPORTED_SYMBOLS and hasattr(_lib.lib, name) and f"{name}(" in header
    assert (_noLZSS.REPEAT_PASS_COUNTS, _noLZSS.REPEAT_PASS_PERIODIC, _noLZSS.REPEAT_PASS_PAIR_RUNS) == (R.COUNTS, R.PERIODIC, R.PAIR_RUNS)


def _differs(a, b):
    if b is None:  # (the mistake spoilt the state until the model of the next pass gave up)
        return True
    return any(not np.array_equal(a[k], b[k]) for k in ("sa", "lcp", "rank", "new_slot", "new_grp")) or \
        any(a[k] != b[k] for k in ("new_m", "counts", "ret", "per_hint", "per_attempts"))


def test_every_mistake_changes_an_expected_output():
    caught = {}
    for bug in R.BUGS + R.NEUTRAL_BUGS:
        caught[bug] = [f"{name}/{order}" for name, order in SMALL if _differs(R.expected(name, order), R.expected_with(name, order, bug))]
        print(f"{bug}: {len(caught[bug])} runs, first {caught[bug][:4]}")
    assert all(caught[bug] for bug in R.BUGS), [bug for bug in R.BUGS if not caught[bug]]
    # the guard, the excuse and the defence: no state the hook accepts can show them (sa_repeats_model.NEUTRAL_BUGS)
    assert not any(caught[bug] for bug in R.NEUTRAL_BUGS)
    # ... and the cases that are there for one mistake catch that one
    for bug, run in (("group_limit_17", "pr_copies_17/text"), ("off_end_own_only", "pr_xx_deferred/reversed"),
                     ("still_tied_limit_15", "pr_16_splits/text"), ("no_same_before", "pr_partly/text"),
                     ("own_chain", "pr_overlap/text"), ("end_lcp_no_steps", "pr_xyx/text"),
                     ("q_lt_depth", "per_segmented/text"), ("verify_4097", "per_q4097/shuffle"),
                     ("no_short_run_check", "per_short_run/shuffle"), ("no_text_end", "per_text_end_q_gt/text"),
                     ("tied_E_not_flagged", "per_tied_E_q_le_depth/text"), ("cand_gate_m8", "per_cand_between/shuffle"),
                     ("near_4097", "cnt_near_4097/text"), ("down_up_swapped", "per_p2/text"), ("lcp_max_across", "per_p2/text")):
        assert run in caught[bug], (bug, run, caught[bug][:6])
    assert any(r.startswith("per_segmented") or r.startswith("per_cand_between") for r in caught["hint_not_lowered"])
