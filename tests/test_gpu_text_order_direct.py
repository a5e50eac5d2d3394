"""The permutation into text order (text_order.hip: bucketed_scatter with its seven forms, permute_packed) on caller pairs,
through nolzss_debug_text_order, against the numpy reference of tests/text_order_model.py by integer equality.  Every call
asserts the form the chooser took (the hook's report), its flags and its boolean result, so that no case passes on another
path than the one it is there for; no look-back may give up.  tests/test_text_order_model_host.py proves without a GPU what
the inputs are there for.  The targets are pre-filled with text_order_model.FILL: what no pair names must keep it.

The inputs (text_order_model.*_cases), the smallest shapes at which each path exists:
  small_*     plain scatter and rank scatter: targets of 1, 63, 4097, 2^24 (the largest that is not big); partial counts
              with one index in 20 at or above n_out (n_out itself, 0xffffffff)
  window_*    one-value window permutation: 2^24 + 1, 2^24 + 4097, 2^25, 2^25 + 1 (index bits 25, 25, 25, 26; a last window
              of 1, 1, 1024 and 1 targets) under every legal keep_input / keep_val, surviving inputs compared; 2^26 + 4097
              (windows of 2^11)
  hist_*      two-value form with histograms (short_codes = false), values of 32 bits
  packed_*    packed look-back form: codes below the threshold; threshold - 1, threshold, threshold + 1, 0xffffffff at the
              edges of tiles and windows; 16 385 .. 32 769 escapes (they fit the list); one in 32 (overflow: the histogram
              form delivers)
  narrow_*    16-bit codes: max 0xffff and 1000, codes around max and the threshold, a wide-code list that holds them and
              one that does not; the two `false` results
  partial_*   partial scatter into 2^24 + 4097 targets from 2^22 (plain), 2^22 + 1, 2^23 + 77 pairs (one partition pass),
              into 2^27 + 4097 (two passes); spread and clustered
  records_*   RecordScatterPlan: records of 1 .. 2^22 bases, two records, a record beyond the limit, with and without out2,
              below and above 2^24 symbols; the separator error
  permute_*   permute_packed: 1, 4097, 2^22 (plain), 2^22 + 1, 2^24 + 4097, 2^25 + 1 pairs
NOLZSS_TEXT_ORDER_HIST, NOLZSS_TEXT_ORDER_ESC and NOLZSS_REC_BUCKET_MIN are frozen at first use: one child process each.
"""
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import text_order_model as M

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run_case(native, case, hist_knob=False):
    """one call of the hook, everything it returns against the model; -> what ran"""
    arrays = case.arrays()
    idx, val, ends = arrays
    exp = M.expected(case, hist_knob, arrays=arrays)
    t0 = time.time()
    if case.is_permute:
        got = native.debug_text_order(idx, packed=val, fill=M.FILL)
    else:
        got = native.debug_text_order(idx, val, case.n_out, rec_ends=ends, fill=M.FILL, **case.kw)
    seconds = time.time() - t0
    where = case.name
    print(f"{where}: form {got['form']} escaped {got['escaped']} listed {got['listed']} result {got['result']} "
          f"passes {got['partition_passes']} nbits {got['nbits']} wb {got['wb']} {seconds:.2f} s")
    assert not got["lookback_gave_up"], where
    for key in ("form", "packed_tried", "list_overflow", "result", "partition_passes", "escaped", "nbits", "wb", "listed"):
        assert exp[key] is None or got[key] == exp[key], (where, key, got[key], exp[key])
    assert got["plan_made"] == bool(ends is not None and case.plan), where
    for key in ("out", "out2", "narrow"):
        if exp[key] is not None:
            assert np.array_equal(got[key], exp[key]), (where, key, mismatch(got[key], exp[key]))
    if exp["narrow"] is not None:
        assert (got["out"] == M.FILL).all(), (where, "out is not used with the 16-bit codes")
    if exp["list"] is not None:
        assert np.array_equal(np.sort(got["list"]), exp["list"]), (where, "list")
        codes, code_max = exp["codes"], case.kw["narrow"][1]
        at = np.flatnonzero(codes >= code_max)
        assert M.list_as_bounds(got["list"]) == dict(zip(at.tolist(), codes[at].tolist())), (where, "the larger entry counts")
    if not case.is_permute:
        if exp["idx_survives"]:
            assert np.array_equal(got["idx_after"], idx), (where, "idx[0] did not survive")
        if exp["val_survives"]:
            assert np.array_equal(got["val_after"], val), (where, "val[0] did not survive")
    return {"case": case.name, "form": got["form"], "pairs": case.count, "seconds": round(seconds, 3),
            "overflow": got["list_overflow"], "escaped": got["escaped"]}


def mismatch(got, exp):
    bad = np.flatnonzero(got != exp)
    return f"{bad.size} of {exp.size} differ, first at {bad[:4].tolist()}: got {got[bad[:4]].tolist()}, expected {exp[bad[:4]].tolist()}"


@pytest.fixture(scope="module")
def native():
    from nolzss_amd import _noLZSS as native
    assert native.device_count() >= 1, "no MI355X visible"
    return native


def by_name(cases):
    return pytest.mark.parametrize("case", cases, ids=[c.name for c in cases])


@by_name(M.small_cases())
def test_plain_scatter_and_rank_scatter(native, case):
    assert run_case(native, case)["form"] == "plain"


@by_name(M.window_cases())
def test_window_permutation(native, case):
    assert run_case(native, case)["form"] == "window_perm"


@by_name(M.hist_cases())
def test_two_value_histogram_form(native, case):
    assert run_case(native, case)["form"] == "two_value_hist"


@by_name(M.packed_cases())
def test_packed_form(native, case):
    """the overflow inputs report the overflow and the histogram form delivers the result"""
    ran = run_case(native, case)
    overflow = case.name.endswith("overflow")
    assert ran["form"] == ("two_value_hist" if overflow else "packed") and ran["overflow"] == overflow
    if case.name.endswith("many"):
        assert 10_000 <= ran["escaped"] <= M.exc_capacity(case.count)


@by_name(M.narrow_cases())
def test_packed_form_with_16_bit_codes(native, case):
    ran = run_case(native, case)
    assert ran["form"] == ("none" if "not_applicable" in case.name or "overflow" in case.name else "packed")


@by_name(M.partial_cases())
def test_partial_then_plain(native, case):
    ran = run_case(native, case)
    assert ran["form"] == ("plain" if case.count == 1 << 22 else "partial_then_plain")


@by_name(M.record_cases(1 << 16))
def test_record_plan_at_the_default(native, case):
    assert run_case(native, case)["form"].startswith("record_plan")


def test_separator_that_is_not_the_first_of_its_record(native):
    """the rank of one separator swapped with its neighbour's: the device error of bucketed_scatter, nothing else"""
    case = M.separator_error_case()
    idx, val, ends = case.arrays()
    with pytest.raises(RuntimeError) as e:
        native.debug_text_order(idx, val, case.n_out, rec_ends=ends, fill=M.FILL, **case.kw)
    assert str(e.value) == M.SEPARATOR_ERROR
    # (and the next call is not affected)
    assert run_case(native, M.record_cases(1 << 16)[0])["form"] == "record_plan2"


@by_name(M.permute_cases())
def test_permute_packed(native, case):
    assert run_case(native, case)["form"] == ("permute_plain" if case.count <= 1 << 22 else "permute_windows")


def test_bad_arguments_are_refused(native):
    idx = np.arange(8, dtype=np.uint32)
    ok = dict(idx=idx, val=idx, n_out=8)
    assert np.array_equal(native.debug_text_order(**ok)["out"], idx)
    empty = native.debug_text_order(idx[:0], idx[:0], 8, fill=7)      # count = 0: nothing runs, true
    assert empty["result"] and empty["form"] == "none" and (empty["out"] == 7).all()
    assert not native.debug_text_order(idx[:0], idx[:0], 8, want_out2=True, narrow=(4, 100))["result"]  # ... false with narrow
    big = (1 << 22) + 1
    twice = np.arange(big, dtype=np.uint32)
    twice[5] = 6
    beyond = np.arange(big, dtype=np.uint32)
    beyond[5] = big
    bad = [
        dict(ok, n_out=1 << 32), dict(ok, n_out=0),
        dict(ok, narrow=(4, 100)),                                      # 16-bit codes without out2
        dict(ok, want_out2=True, narrow=(4, 0)), dict(ok, want_out2=True, narrow=(4, 0x10000)),
        dict(ok, rec_ends=[3, 7]), dict(ok, rec_ends=[3, 3, 8]), dict(ok, rec_ends=[5, 3, 8]),   # ends that do not ascend to n
        dict(ok, idx=np.array([0, 1, 2, 3, 4, 5, 6, 6]), rec_ends=[3, 8]),   # a plan, and no permutation
        dict(idx=twice, val=twice, n_out=big), dict(idx=beyond, val=beyond, n_out=big),   # count = n_out beyond 2^22
        dict(idx=np.array([0, 0]), packed=np.zeros(2, dtype=np.uint64)), dict(idx=np.array([0, 2]), packed=np.zeros(2, dtype=np.uint64)),
    ]
    for kw in bad:
        with pytest.raises(ValueError):
            native.debug_text_order(**kw)
    from nolzss_amd._lib import lib
    out, rep = np.zeros(8, dtype=np.uint32), np.zeros(12, dtype=np.uint32)
    after = [np.zeros(8, dtype=np.uint32), np.zeros(8, dtype=np.uint32)]
    args = [idx.ctypes.data, idx.ctypes.data, None, 8, 8, 3, 0, 0, 0, None, 0, 0, out.ctypes.data, None, None, None,
            after[0].ctypes.data, after[1].ctypes.data, rep.ctypes.data]
    assert lib.nolzss_debug_text_order(*args) == 0
    for null_at in (0, 1, 12, 16, 17, 18):
        a = list(args)
        a[null_at] = None
        assert lib.nolzss_debug_text_order(*a) != 0, null_at
    for flags in (8, 32, 64):   # out2 without its array, permute_packed without its words, an unknown flag
        a = list(args)
        a[5] = flags
        assert lib.nolzss_debug_text_order(*a) != 0, flags


CHILD = r'''
import json, sys
sys.path.insert(0, "tests")
import text_order_model as M
import test_gpu_text_order_direct as T
from nolzss_amd import _noLZSS as native
assert native.device_count() >= 1, "no MI355X visible"
what = sys.argv[1]
ran = [T.run_case(native, c, hist_knob=what == "hist") for c in M.child_cases()[what]]
print("RAN " + json.dumps(ran))
'''


def run_child(env, *args):
    r = subprocess.run([sys.executable, "-c", CHILD, *args], cwd=ROOT, env=dict(os.environ, **env), capture_output=True, text=True,
                       timeout=600)
    lines = [x for x in r.stdout.splitlines() if x.startswith("RAN ")]
    assert r.returncode == 0 and lines, r.stdout[-3000:] + r.stderr[-4000:]
    print(r.stdout)
    return json.loads(lines[-1][4:])


def test_histogram_knob_in_a_child_process():
    """NOLZSS_TEXT_ORDER_HIST=1 over the packed-form list: the histogram form on every input, the packed form never tried
    (16-bit codes: false)"""
    ran = run_child({"NOLZSS_TEXT_ORDER_HIST": "1"}, "hist")
    assert len(ran) == 17 and all(x["form"] == "two_value_hist" for x in ran[:16]) and ran[16]["form"] == "none"


def test_escape_knob_in_a_child_process():
    """NOLZSS_TEXT_ORDER_ESC=100 over the packed-form list and the 16-bit cases made for that threshold: a threshold below
    both saturation values, no code listed twice"""
    ran = run_child({"NOLZSS_TEXT_ORDER_ESC": str(M.ESC_KNOB)}, "esc")
    assert len(ran) == 24 and sum(x["form"] == "packed" for x in ran) == 12 + 6 and sum(x["overflow"] for x in ran) == 5


def test_record_plan_of_short_records_in_a_child_process():
    """NOLZSS_REC_BUCKET_MIN=1: records of 1 / 63 / 64 / 65 / 4095 .. 4097 / 2^14 / 2^14 + 1 / 2^22 bases in one text, two
    records only, 2^24 symbols and more, one and two values; a record of 2^22 + 1 bases gets no plan"""
    ran = run_child({"NOLZSS_REC_BUCKET_MIN": "1"}, "records")
    forms = [x["form"] for x in ran]
    assert forms.count("record_plan") == 3 and forms.count("record_plan2") == 4 and forms.count("plain") == 1
