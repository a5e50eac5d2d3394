"""The LDS sub-bucket sort (local_sort.hpp: local_sort_kernel in its five instantiations, local_sort_sub_buckets with the
list of large sub-buckets and the segmented passes behind it) on caller pairs, through nolzss_debug_local_sort, against
the numpy reference of tests/local_sort_model.py by integer equality: per bucket a stable sort by word >> shift0 (values =
arange(n): any instability shows in them), and for the form with the regroup of round 0 on the way the LCPs, the tied
list and the survivors.  tests/test_local_sort_model_host.py proves without a GPU what every input is there for.

The inputs (local_sort_model.cases, fused_cases, record_bucket_cases), at most 150 000 pairs per call:
  sizes          every sub-bucket size at which the number of rows changes, 1 .. 18 432 (capacity); n no multiple of 4
  overflow       18 433 and 40 000 pairs (the list, ten tiles of segmented passes), overflowing neighbours, one between two that fit
  capacity_edge  18 433 next to 18 432
  residues       every size below 16 at every start residue mod 4 (heads and tails of the 16-byte stores)
  turns          1500 non-empty sub-buckets: several turns per workgroup, prefetched keys handed over
  grid_plus_one, few_255, few_2, few_1     more, fewer workgroups than sub-buckets; a last turn that finds nothing
  patterns_d*    digit patterns by place (wave stretch, row, lane) on each digit and on all, in sub-bucket order (the pass
                 by the byte at bit 24 is the identity) and shuffled; row 0 distinct and every later row on one counter
  all_ones       digits and whole words of all ones in a partial last row, in front of the pad keys
  key35_bins     the bins around the threads that own two of 1024
  records_nb*    records form with 1, 2, 3, 257 buckets (5 elsewhere)
  fused_*        ties, short tags, LCPs decided by tag, key bits and bucket byte at first / last places and 64-place edges
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import local_sort_model as M

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run_case(native, case, form, fused):
    """one call of the hook, everything it returns against the model; -> what ran"""
    exp = M.expected(case, form, fused)
    n = len(case.words)
    got = native.debug_local_sort(case.words, np.arange(n, dtype=np.uint32), case.starts, form.shift0, len(form.widths), form.key35,
                                  want_regroup=fused)
    where = (form.name, fused, case.name)
    assert got["listed"] == exp["listed"], where
    assert np.array_equal(got["values"], exp["values"]), where
    if got["fused"]:
        assert fused and exp["listed"] == 0 and not got["lookback_gave_up"] and not got["lane_order"], where
        assert got["survivors"] == exp["survivors"], where
        assert np.array_equal(got["lcp"], exp["lcp"]), where
        assert np.array_equal(got["new_slot"], exp["new_slot"]) and np.array_equal(got["new_grp"], exp["new_grp"]), where
    else:
        assert np.array_equal(got["words"], exp["words"]), where
    return {"case": case.name, "fused": got["fused"], "gave_up": got["lookback_gave_up"], "lane_order": got["lane_order"],
            "listed": got["listed"], "fusable": bool(fused and exp["listed"] == 0), "pairs": n,
            "subs": int((M.sub_sizes(case.words, case.starts) > 0).sum())}


def run_form(native, form, fused):
    return [run_case(native, case, form, fused) for case in M.all_cases(form, fused)]


@pytest.fixture(scope="module")
def native():
    from nolzss_amd import _noLZSS as native
    assert native.device_count() >= 1, "no MI355X visible"
    return native


@pytest.mark.parametrize("form", [M.KEY16, M.KEY35, M.RECORDS], ids=lambda f: f.name)
def test_plain_form_is_a_stable_sort(native, form):
    """local_sort_kernel<2>, <2, false, true>, <3>: words and values of every case, the list count, the lane-order flag"""
    ran = run_form(native, form, False)
    assert not any(r["fused"] or r["gave_up"] for r in ran)
    assert not any(r["lane_order"] for r in ran), "LDS atomics were not served in lane order: a finding about the device (DESIGN section 5)"
    assert sum(r["listed"] for r in ran) >= 6
    print(f"{form.name}: {len(ran)} cases, {sum(r['subs'] for r in ran)} sub-buckets, {sum(r['pairs'] for r in ran)} pairs")


@pytest.mark.parametrize("form", [M.KEY16, M.KEY35], ids=lambda f: f.name)
def test_fused_form_sorts_and_regroups(native, form):
    """local_sort_kernel<2, true>, <2, true, true>: values, LCPs, tied list and survivors of every case; where a sub-bucket
    overflows the plain kernel runs (and is checked); a look-back that gave up is a fallback, checked as well, but more
    than one call in ten is a failure"""
    ran = run_form(native, form, True)
    assert not any(r["lane_order"] for r in ran), "LDS atomics were not served in lane order: a finding about the device (DESIGN section 5)"
    fusable = [r for r in ran if r["fusable"]]
    assert len(fusable) >= 15 and not any(r["fused"] for r in ran if not r["fusable"])
    gave_up = [r["case"] for r in fusable if r["gave_up"]]
    assert all(r["fused"] or r["gave_up"] for r in fusable)
    assert 10 * len(gave_up) <= len(fusable), gave_up
    print(f"{form.name} fused: {len(ran)} cases, {sum(r['subs'] for r in ran)} sub-buckets, {sum(r['pairs'] for r in ran)} pairs; gave up: {gave_up}")


CHILD = r'''
import json, sys
sys.path.insert(0, "tests")
import local_sort_model as M
import test_gpu_local_sort as T
from nolzss_amd import _noLZSS as native
assert native.device_count() >= 1, "no MI355X visible"
form = M.FORMS[sys.argv[1]]
ran = T.run_form(native, form, False)
if form is not M.RECORDS:
    ran += T.run_form(native, form, True)
print("RAN " + json.dumps(ran))
'''


@pytest.mark.parametrize("form", ["key16", "key35", "records"])
@pytest.mark.parametrize("knob", ["NOLZSS_TEST_LOCAL_ORDER_FAILS", "NOLZSS_TEST_LOCAL_LOOKBACK_FAILS"])
def test_fallback_paths_in_a_child_process(knob, form):
    """The knobs are frozen at first use: one child per knob and form, every case checked in the child as above.
    NOLZSS_TEST_LOCAL_ORDER_FAILS: every sub-bucket is redone by the segmented passes (the fused form is not taken).
    NOLZSS_TEST_LOCAL_LOOKBACK_FAILS: the fused form reports the fallback and the plain kernel runs."""
    env = dict(os.environ, **{knob: "1"})
    r = subprocess.run([sys.executable, "-c", CHILD, form], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    lines = [x for x in r.stdout.splitlines() if x.startswith("RAN ")]
    assert r.returncode == 0 and lines, r.stdout[-2000:] + r.stderr[-4000:]
    ran = json.loads(lines[-1][4:])
    assert len(ran) >= 15 and not any(x["fused"] or x["lane_order"] for x in ran)
    fusable = [x for x in ran if x["fusable"]]
    if knob.endswith("LOOKBACK_FAILS"):
        assert all(x["gave_up"] for x in fusable) and (form == "records" or len(fusable) >= 15)
    else:
        assert not any(x["gave_up"] for x in ran)


def test_bad_arguments_are_refused(native):
    w = np.arange(8, dtype=np.uint32)
    v = np.arange(8, dtype=np.uint32)
    s256 = np.concatenate([[0], np.full(256, 8)]).astype(np.uint32)
    ok = dict(words=w, values=v, starts=s256, shift0=8, npass=2)
    assert np.array_equal(native.debug_local_sort(**ok)["values"], v)
    bad = [
        dict(ok, starts=np.array([0, 5, 3, 8], dtype=np.uint32)),              # starts that do not ascend
        dict(ok, starts=np.array([0, 7], dtype=np.uint32)),                    # .. that do not end at n
        dict(ok, starts=np.array([1, 8], dtype=np.uint32)),                    # .. that do not begin at 0
        dict(ok, starts=np.array([8], dtype=np.uint32)),                       # no bucket
        dict(ok, npass=1), dict(ok, npass=4),                                  # npass outside 2 .. 3
        dict(ok, shift0=5, npass=3, key35=True), dict(ok, shift0=8, npass=2, key35=True),   # key35 with another shift0 or npass
        dict(ok, shift0=9, npass=2), dict(ok, shift0=1, npass=3), dict(ok, shift0=-1),      # digits beyond bit 24 / below bit 0
        dict(ok, starts=np.array([0, 8], dtype=np.uint32), want_regroup=True),            # nb * 256 no multiple of 1024
        dict(ok, shift0=0, npass=3, want_regroup=True), dict(ok, shift0=0, npass=2, want_regroup=True),   # no key layout
        dict(ok, words=w[:0], values=v[:0], starts=np.zeros(257, dtype=np.uint32)),       # no pairs
    ]
    for kw in bad:
        with pytest.raises(ValueError):
            native.debug_local_sort(**kw)
    from nolzss_amd._lib import lib
    st = np.zeros(1, dtype=np.uint32)
    args = [w.ctypes.data, v.ctypes.data, 8, s256.ctypes.data, 256, 8, 2, 0, 0, 0, w.ctypes.data, v.ctypes.data, None, None, None, None,
            st.ctypes.data]
    for null_at in (0, 1, 3, 10, 11, 16):
        a = list(args)
        a[null_at] = None
        assert lib.nolzss_debug_local_sort(*a) != 0, null_at
    a = list(args)
    a[8] = 1  # want_regroup without its outputs
    assert lib.nolzss_debug_local_sort(*a) != 0
    a = list(args)
    a[2] = 1 << 31  # (refused before anything is read)
    assert lib.nolzss_debug_local_sort(*a) != 0


def test_a_call_leaves_no_state_behind(native):
    """one case as key35 and then as key16 gives what it gives in the other order, fused and plain"""
    case = {c.name: c for c in M.all_cases(M.KEY16, True)}["fused_sizes"]  # (tags <= 16: good for either layout)
    values = np.arange(len(case.words), dtype=np.uint32)

    def call(form, fused):
        got = native.debug_local_sort(case.words, values, case.starts, form.shift0, 2, form.key35, want_regroup=fused)
        return {k: (v.tolist() if isinstance(v, np.ndarray) else v) for k, v in got.items() if k != "lookback_gave_up"}

    for fused in (False, True):
        a35 = call(M.KEY35, fused)
        a16 = call(M.KEY16, fused)
        b16 = call(M.KEY16, fused)
        b35 = call(M.KEY35, fused)
        if a35["fused"] == b35["fused"] and a16["fused"] == b16["fused"]:
            assert a35 == b35 and a16 == b16
        for got, form in ((a35, M.KEY35), (b35, M.KEY35), (a16, M.KEY16), (b16, M.KEY16)):
            assert got["values"] == M.stable_sort(case.words, values, case.starts, form.shift0)[1].tolist()
            assert not got["lane_order"] and got["listed"] == 0
