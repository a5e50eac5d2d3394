"""What nolzss_rlz_index_repeat_count / _repeats refuse, with the status of each, and that the refusals the contract
places before any device work leave the device alone: with the profiler on, every device path of the library runs inside
a ProfScope, so an empty report is the observable (as tests/test_gpu_rlz_archive_append.py::test_empty_batches has it).
The refusal of the hit total cannot be reached with a small reference, so the host-side decision is checked directly."""
import ctypes as C

import numpy as np
import pytest

import rlz_repeats_model as rm

pytestmark = pytest.mark.gpu

REFS = [b"ACGTACGTTTACGGACGT", b"GGACGTAC"]


@pytest.fixture(scope="module")
def rlz():
    from nolzss_amd import _noLZSS
    assert _noLZSS.device_count() >= 1, "no MI355X visible"
    from nolzss_amd.genomics import rlz
    return rlz


def _quiet(native, fn):
    """fn() with the profiler on -> (its result, the report)"""
    native.profile_enable(True)
    try:
        native.profile_reset()
        out = fn()
        return out, native.profile_report()
    finally:
        native.profile_enable(False)
        native.profile_reset()


def _raw_repeats(handle, min_length, min_count, max_hits, with_out=True):
    from nolzss_amd import _lib
    res = _lib.RlzRepeatsResult(7, 0xdead, 0xdead, 0xdead, 7)
    rc = _lib.lib.nolzss_rlz_index_repeats(handle, min_length, min_count, max_hits, C.byref(res) if with_out else None)
    return rc, res, _lib.lib.nolzss_last_error().decode()


def _raw_count(handle, min_length, min_count, with_out=True):
    from nolzss_amd import _lib
    out = C.c_uint64(7)
    rc = _lib.lib.nolzss_rlz_index_repeat_count(handle, min_length, min_count, C.byref(out) if with_out else None)
    return rc, out.value, _lib.lib.nolzss_last_error().decode()


def test_refusals_before_any_device_work(rlz):
    from nolzss_amd import _lib, _noLZSS as native
    with rlz.RlzIndex.build(REFS) as ix:
        h = ix._live()._handle()

        def all_refusals():
            seen = []
            for handle, min_length, min_count, with_out, word in ((None, 20, 2, True, "handle is null"),
                                                                  (h, 20, 2, False, "output pointer is null"),
                                                                  (h, 0, 2, True, "min_length >= 1"),
                                                                  (h, 20, 0, True, "min_count >= 2"),
                                                                  (h, 20, 1, True, "min_count >= 2")):
                rc, res, message = _raw_repeats(handle, min_length, min_count, 64, with_out)
                assert rc == _lib.ERR_INVALID_ARGUMENT and word in message, (rc, message)
                if with_out:  # the result is zeroed: nothing to free, nothing stale
                    assert (res.num_repeats, res.repeats, res.hit_offsets, res.hits, res.num_hits) == (0, None, None, None, 0)
                rc, count, message = _raw_count(handle, min_length, min_count, with_out)
                assert rc == _lib.ERR_INVALID_ARGUMENT and word in message, (rc, message)
                assert count == (0 if with_out else 7)
                seen.append(word)
            return seen

        seen, report = _quiet(native, all_refusals)
        assert len(seen) == 5 and not report, f"a refusal touched the device: {sorted(report)}"
        for call in (lambda: ix.repeats(min_length=0), lambda: ix.repeats(min_count=1), lambda: ix.repeat_count(min_length=0),
                     lambda: ix.repeat_count(min_count=1), lambda: ix.repeats(min_length=-1), lambda: ix.repeats(min_count=-2),
                     lambda: ix.repeats(max_hits=-1), lambda: ix.repeat_count(min_length=-1)):
            with pytest.raises(ValueError):
                call()
        # the handle is still good, and a query does run on the device
        exp = rm.RepeatsModel(REFS, True).repeats(2, 2, 0)
        got, report = _quiet(native, lambda: ix.repeats(2, 2, 0))
        assert all(np.array_equal(got[k], exp[k]) for k in exp) and len(got["position"]) >= 3
        assert report["rlz_index_repeats"][0] == 1 and report["rlz_repeat_flags"][0] >= 1
    for call in (lambda: ix.repeats(), lambda: ix.repeat_count()):
        with pytest.raises(ValueError, match="closed"):
            call()


def test_free_of_a_null_or_empty_result():
    from nolzss_amd import _lib
    _lib.lib.nolzss_free_rlz_repeats_result(None)
    res = _lib.RlzRepeatsResult()
    _lib.lib.nolzss_free_rlz_repeats_result(C.byref(res))
    assert (res.num_repeats, res.repeats, res.hit_offsets, res.hits, res.num_hits) == (0, None, None, None, 0)


def test_a_small_total_is_not_refused(rlz):
    """A^n with max_hits = 0 and a small n keeps the total small: the query answers"""
    n = 300
    with rlz.RlzIndex.build(b"A" * n, with_rc=False) as ix:
        got = ix.repeats(min_length=1, min_count=2, max_hits=0)
        assert got["count"].tolist() == list(range(n, 1, -1)) and int(got["offsets"][-1]) == n * (n + 1) // 2 - 1


def test_the_decision_on_the_totals():
    """the decision function itself, with totals around 2^32 and records around 2^31"""
    from nolzss_amd import _lib
    from nolzss_amd.genomics import rlz
    f = _lib.lib.nolzss_debug_rlz_repeats_refusal
    top = rlz.MAX_TEXT
    for records, total, status in ((1, top - 1, _lib.OK), (1, top, _lib.OK), (1, top + 1, _lib.ERR_INVALID_ARGUMENT),
                                   (9, (1 << 32) - 1, _lib.ERR_INVALID_ARGUMENT), (9, 1 << 32, _lib.ERR_INVALID_ARGUMENT),
                                   (9, (1 << 32) + 1, _lib.ERR_INVALID_ARGUMENT), (9, (1 << 64) - 1, _lib.ERR_INVALID_ARGUMENT),
                                   ((1 << 31) - 1, 0, _lib.OK), (1 << 31, 0, _lib.ERR_INVALID_ARGUMENT),
                                   ((1 << 31) + 1, top + 1, _lib.ERR_INVALID_ARGUMENT)):
        assert f(records, total, 11, 13) == status, (records, total)
        if status != _lib.OK:
            message = _lib.lib.nolzss_last_error().decode()
            if records >= 1 << 31:
                assert f"this one has {records}" in message and "min_length (it is 13)" in message
            else:
                assert f"repeats would report {total} hits" in message and f"more than the {top}" in message
                assert "max_hits (it is 11" in message and "min_length (it is 13)" in message
