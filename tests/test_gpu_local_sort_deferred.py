"""The deferred look-back of the sub-bucket sort with the regroup of round 0 on the way (local_sort.hpp: local_sort_kernel
<2, true> and <2, true, true>): a workgroup publishes a sub-bucket's aggregate and last key at the end of loop 1 and walks,
settles the first boundary and runs loop 2 one turn later, or in a flush behind its last turn.  Inputs that put every
part of that on the line, through nolzss_debug_local_sort against tests/local_sort_model.py by integer equality (values,
lcp, new_slot, new_grp, survivors; values = arange(n)).

G = the kernel's grid = the number of compute units (local_sort_sub_buckets); workgroup b takes the sub-buckets b, b + G, ..
All inputs fill the sub-buckets 0 .. K - 1 with no gap, so sub-bucket q is the turn q // G of workgroup q % G.  At most
150 000 pairs per call, 65 pairs per sub-bucket unless said otherwise:
  turns_K       K = 1, 2, G - 1, G, G + 1, 2G - 1, 2G, 2G + 1, 3G + 1: a flush alone; a workgroup that defers across a turn
                and then flushes; workgroups whose last turn is empty; the last sub-bucket (the total, the survivors) in a
                first and in a later turn
  zeros_*       sub-buckets with no tied element (an aggregate of 0 is a published descriptor all the same) next to
                all-tied ones, in both orders and in pairs, at the first and the last q of a turn
  boundary      the first key of q against the last key of q - 1: stored words equal up to the tag (the sub-bucket byte and
                the bucket byte decide), tags short on either side and on both, for q - 1 the same turn's neighbour and
                the last of the turn before (q = G, 2G); every other boundary differs in the key bits
  bucket_byte   equal stored words in the same byte of several buckets, nothing between: q - 1 is the workgroup's own turn before
  lagging_*     one sub-bucket of 18 432 pairs (24 rows) at q = 0, G / 2 and last: its owner publishes many small turns
                late, the walks of the others wait
The way back (NOLZSS_TEST_LOCAL_LOOKBACK_FAILS, a child process per form): not fused, the give-up reported, the plain
kernel's words and values.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import local_sort_model as M
import test_gpu_local_sort as T

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL, BIG = 65, M.CAP


def sub_bucket(rng, form, count, kind="runs", first=None, last=None):
    """the 24 bits below the byte of `count` pairs in a random input order.  kind: "runs" (few keys: ties), "zero" (all keys
    distinct, full tags: nobody stays tied), "tied" (one word).  first / last = (key, tag): the only element with the
    smallest / largest key of the sub-bucket, so that it is its first / last one in sorted order."""
    tb, full = form.shift0, form.tag_full
    kmax = (1 << (24 - tb)) - 1
    lo = first[0] + 1 if first else 0
    hi = last[0] - 1 if last else kmax
    free = count - (first is not None) - (last is not None)
    if kind == "tied":
        assert not first and not last
        keys, tags = np.full(count, 12345 & kmax), np.full(count, full)
    elif kind == "zero":
        keys, tags = rng.choice(np.arange(lo, min(hi, lo + 4 * count) + 1), size=free, replace=False), np.full(free, full)
    else:
        keys = lo + rng.integers(0, max(2, count // 3), size=free) * 5
        assert keys.max() <= hi
        tags = np.where(rng.random(free) < 0.05, rng.integers(0, full, size=free), full)
    for edge in (first, last):
        if edge:
            keys, tags = np.append(keys, edge[0]), np.append(tags, edge[1])
    order = rng.permutation(count)
    return ((keys.astype(np.int64) << tb) | tags)[order]


def consecutive(form, name, seed, kinds, sizes=None, edges=None):
    """sub-buckets 0 .. len(kinds) - 1, none empty; edges = {q: (first, last)}"""
    B = M.Builder(form, 256, seed, True)
    for q, kind in enumerate(kinds):
        first, last = (edges or {}).get(q, (None, None))
        B.add_words(q, sub_bucket(B.rng, form, sizes[q] if sizes else SMALL, kind, first, last))
    return B.finish(name)


def make_cases(form, G):
    full = form.tag_full
    out = []
    for j, K in enumerate((1, 2, G - 1, G, G + 1, 2 * G - 1, 2 * G, 2 * G + 1, 3 * G + 1)):
        if K >= 1:
            out.append(consecutive(form, f"turns_{K}", 100 + j, ["runs"] * K))
    K = 2 * G + 2
    out.append(consecutive(form, "zeros_even", 120, ["zero" if q % 2 == 0 else "tied" for q in range(K)]))
    out.append(consecutive(form, "zeros_odd", 121, ["zero" if q % 2 == 1 else "tied" for q in range(K)]))
    out.append(consecutive(form, "zeros_pairs", 122, ["zero" if q % 4 in (0, 3) else "tied" for q in range(K)]))
    # the first boundary: q -> (tag of the last element of q - 1, tag of the first element of q), the key of both X
    X = (1 << (23 - form.shift0)) + 0x155
    want = {1: (full, full), 5: (3, full), G // 2: (full, 2), G: (full, full), G + 3: (4, 4), 2 * G: (full, 1), 2 * G + 1: None}
    edges, prev = {}, -2
    for q in sorted(want):
        if want[q] is None or q - prev < 2 or q < 1 or q >= K:  # (a sub-bucket takes part in one designed boundary)
            continue
        prev = q
        edges[q - 1] = (None, (X, want[q][0]))
        edges[q] = ((X, want[q][1]), None)
    assert len(edges) >= 8 or G < 16
    out.append(consecutive(form, "boundary", 123, ["runs"] * K, edges=edges))
    # equal stored words, the bucket byte alone differs (in every bit); the same workgroup turn after turn
    B = M.Builder(form, 256, 124, True)
    word = sub_bucket(B.rng, form, 1, "tied")
    for bucket in (0, 1, 2, 3, 4, 8, 16, 32, 64, 128, 129, 255):
        B.add_words(bucket * 256 + 0x5a, np.repeat(word, 3 if bucket % 2 else 1))
    out.append(B.finish("bucket_byte"))
    K = 2 * G + 3
    for at in (0, G // 2, K - 1):
        sizes = [BIG if q == at else SMALL for q in range(K)]
        out.append(consecutive(form, f"lagging_{at}", 125, ["runs"] * K, sizes=sizes))
    assert all(len(c.words) < 150_000 for c in out)
    return out


@pytest.fixture(scope="module")
def native():
    from nolzss_amd import _noLZSS as native
    assert native.device_count() >= 1, "no MI355X visible"
    return native


@pytest.fixture(scope="module")
def grid():
    """what local_sort_sub_buckets launches: one workgroup per compute unit (hipDeviceAttributeMultiprocessorCount)"""
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


@pytest.mark.parametrize("form", [M.KEY16, M.KEY35], ids=lambda f: f.name)
def test_deferred_walk_matches_the_model(native, grid, form):
    """every input fused: all five outputs equal the model's (T.run_case asserts them and that no walk gave up where the
    call reports the fused form); a genuine give-up is a checked fallback, at most one call in ten; none is expected"""
    ran = [T.run_case(native, case, form, True) for case in make_cases(form, grid)]
    assert len(ran) >= 17 and all(r["fusable"] and r["listed"] == 0 and not r["lane_order"] for r in ran)
    gave_up = [r["case"] for r in ran if r["gave_up"]]
    assert all(r["fused"] or r["gave_up"] for r in ran)
    print(f"{form.name} deferred, grid {grid}: {len(ran)} calls, {sum(r['subs'] for r in ran)} sub-buckets, "
          f"{sum(r['pairs'] for r in ran)} pairs; gave up: {len(gave_up)} {gave_up}")
    assert 10 * len(gave_up) <= len(ran), gave_up


CHILD = r'''
import json, sys
sys.path.insert(0, "tests")
import local_sort_model as M
import test_gpu_local_sort as T
import test_gpu_local_sort_deferred as D
from nolzss_amd import _noLZSS as native
assert native.device_count() >= 1, "no MI355X visible"
form = M.FORMS[sys.argv[1]]
print("RAN " + json.dumps([T.run_case(native, case, form, True) for case in D.make_cases(form, int(sys.argv[2]))]))
'''


@pytest.mark.parametrize("form", ["key16", "key35"])
def test_the_way_back_in_a_child_process(grid, form):
    """NOLZSS_TEST_LOCAL_LOOKBACK_FAILS (frozen at first use: a child): the flag is up before the kernel starts, every
    workgroup ends behind its second turn and its flush, the host reports the give-up and sorts again with the plain
    kernel, whose words and values T.run_case checks"""
    env = dict(os.environ, NOLZSS_TEST_LOCAL_LOOKBACK_FAILS="1")
    r = subprocess.run([sys.executable, "-c", CHILD, form, str(grid)], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    lines = [x for x in r.stdout.splitlines() if x.startswith("RAN ")]
    assert r.returncode == 0 and lines, r.stdout[-2000:] + r.stderr[-4000:]
    ran = json.loads(lines[-1][4:])
    assert len(ran) >= 17 and all(x["fusable"] for x in ran)
    assert not any(x["fused"] or x["lane_order"] for x in ran) and all(x["gave_up"] for x in ran)
