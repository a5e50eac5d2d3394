"""Every row of the round-0 key plan (plan_keys, suffix_array.hip) on inputs built around its own constants
(key_layout_cases.py; test_key_layout_inputs.py is their CPU proof): pairs of suffixes whose LCP sits on the key width, on
the window edges of the first direct round and on its cap, texts that end inside a copy or in runs of the padding symbol,
and the same with sentinels.  One child process per row and environment (the knobs are read once per process) takes all its
texts; the trace proves for every text which plan ran, and every array is compared with the oracle by integer equality.

Tied count after round 0.  A key that loses information only leaves more suffixes tied, the direct round repairs the order
and the suffix array is still right: the count the trace prints is therefore compared, as an equality, with the model of
key_layout_cases.tied_after_key_sort (a suffix nearer than k_syms to its terminator is a group of its own; the others tie
exactly when their first k_syms symbols agree) on the general (2, 4 and 8 bits), dna_fast, key16 and segmented rows.
The first run of this comparison found the device one above the model on a prepared string of 64 sequences (792 against
791, dna_fast): regroup_kernel decided "the element behind me is a head" for the last lane of a wavefront from the keys
alone, so a SHORT suffix there whose copy at another terminator follows it with the same key was kept as tied and went
through the direct round as a group of one.  The kernel now applies the short-tag rule across the wavefront's edge too; the
prepared string of 70 sequences with one tail (key_layout_cases.sequence_sets, "seventy_shared_tails") holds runs of 70
equal short keys, longer than a wavefront, and is the regression input.

Cap of the direct round.  Suffixes that agree on `cap` symbols or more cannot be separated by a round that looks `cap`
symbols deep: the trace line of the direct round must report the cap of the layout and at least as many suffixes still tied
as agree that far in the oracle's LCP array (more where the round left a group untouched).  NOLZSS_REFINE_WORDS=4 moves the
cap onto the first window edge."""
import os
import pickle
import subprocess
import sys

import pytest

import key_layout_cases as K

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("row", list(K.ROWS))
def test_row(row, tmp_path):
    env_extra, has_model = K.ROWS[row]
    cases = K.cases_of(row)
    expected = [K.expected_of(c) for c in cases]
    path = tmp_path / "expected.pickle"
    with open(path, "wb") as f:
        pickle.dump(expected, f)
    env = dict(os.environ, NOLZSS_TRACE="1", **env_extra)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "key_layout_cases.py"), row, str(path)], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and f"ok {len(cases)}" in r.stdout, r.stdout[-2000:] + r.stderr[-6000:]
    trace = K.split_trace(r.stderr)
    assert sorted(trace) == list(range(len(cases)))
    refine_words = int(env_extra.get("NOLZSS_REFINE_WORDS", 32))
    seen_plans, cap_cases = set(), 0
    for i, (case, exp) in enumerate(zip(cases, expected)):
        lay = case.lay
        keys = K.TRACE_KEY.findall(trace[i])
        assert keys, (case.name, trace[i][-500:])
        # which plan ran, and on how many symbols
        k_syms = K.plan_k_syms(case.plan, lay.bits)
        assert {(int(ks), plan) for _, _, ks, plan in keys} == {(k_syms, case.plan)}, (case.name, keys)
        seen_plans.add(case.plan)
        if not has_model or case.kind in ("batch", "batch_rc"):
            continue
        S = K.prepare_rc(case.data) if case.kind == "prepared_rc" else case.data
        codes, lim = K.text_view(S)
        model = K.tied_after_key_sort(codes, lim, K.classify(S)[1], k_syms)
        on_text = [(int(m), plan) for n, m, _, plan in keys if int(n) == len(S)]
        assert on_text and all(m == model for m, _ in on_text), (case.name, "tied after round 0", on_text, "model", model)
        # the direct round: its cap, and what must still be tied behind it
        cap = k_syms + refine_words * 64 // lay.bits
        lcp = exp.lcp if case.kind == "prepared_rc" else exp["lcp"]
        beyond = K.tied_at_depth(lcp, cap)
        direct = K.TRACE_DIRECT.findall(trace[i])
        if model > 0 and k_syms < len(S):
            assert direct, (case.name, "no direct round in the trace")
        for c, still in direct:
            assert int(c) == cap and int(still) >= beyond, (case.name, "direct round", c, still, "cap", cap, "beyond it", beyond)
        if beyond and "planted" in case.name:
            cap_cases += 1
    base = row.replace("_cap_at_window", "").replace("_local", "")
    assert ("general" if base.startswith("general") else base) in seen_plans, seen_plans
    if has_model:
        assert cap_cases >= 1, "no text of this row had planted pairs still tied behind the cap of the direct round"
