#!/usr/bin/env python3
"""Relative-LZ index: what the insertion log, the normalised walk, the allele table and the consensus cost, measured
beside the add of a library built from the parent commit.

    python tools/rlz_index_consensus_probe.py [--parent nolzss_amd/libnolzss_hip.parent.so] [--lg 24] [--lgreads 18]
                                              [--lgcontigs 12] [--pairs 5] [--out profiles/r17_rlz_index_consensus.txt]

The reference and the two target sets are those of tools/rlz_index_pileup_probe.py, at the same parameters.  Per set,
on arguments marshalled once, in one process:
  - the wall time of nolzss_rlz_pileup_add with flags 0 and with NOLZSS_RLZ_PILEUP_NORMALIZE against the add of the
    parent's library (its own index and pileup handles on the same device), in alternating rounds parent / flags 0 /
    normalize after a warm-up of each; per round the two differences to the parent, then their median and spread;
  - the profiler scope rows of one add of either library side by side: the rows this one adds;
  - the device span of the new scopes: log count and growth, the shifts (accumulate with and without the flag), the
    allele table, insertions and the consensus;
  - the bytes a consensus brings down against the bytes counts() of the whole block would.
Runs on the GPU machine only.  --parent missing: the parent's columns are left out and the file says so.  No counter run.
"""
import argparse
import ctypes as C
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
sys.path.insert(0, str(ROOT / "tools"))

import numpy as np  # noqa: E402

import gen  # noqa: E402
from nolzss_amd import _lib  # noqa: E402
from nolzss_amd import _noLZSS as native  # noqa: E402
from rlz_index_seeds_probe import cuts  # noqa: E402
from rlz_probe import timed  # noqa: E402

NEW_SCOPES = ("rlz_pileup_log_count", "rlz_pileup_log_grow", "rlz_pileup_scans", "rlz_pileup_accumulate")
READ_SCOPES = ("rlz_pileup_resolve", "rlz_pileup_alleles", "rlz_pileup_insertions", "rlz_pileup_insertion_records",
               "rlz_consensus", "rlz_consensus_lengths", "rlz_consensus_text")


class Parent:
    """the few entry points of another build of the library that the comparison needs, through ctypes"""

    def __init__(self, path):
        vp, sz = C.c_void_p, C.c_size_t
        seqs = [C.POINTER(C.c_char_p), C.POINTER(sz), sz]
        self.lib = lib = C.CDLL(str(path))
        lib.nolzss_rlz_index_open.argtypes = seqs + [C.c_int, C.c_uint32, C.c_int, C.POINTER(vp)]
        lib.nolzss_rlz_index_close.argtypes = [vp]
        lib.nolzss_rlz_pileup_open.argtypes = [vp, C.POINTER(_lib.RlzAlignParams), C.POINTER(vp)]
        lib.nolzss_rlz_pileup_add.argtypes = [vp] + seqs + [C.c_int, C.POINTER(_lib.RlzPileupAddInfo)]
        lib.nolzss_rlz_pileup_close.argtypes = [vp]
        lib.nolzss_profile_enable.argtypes = [C.c_int, C.c_int]
        lib.nolzss_profile_reset.argtypes = [C.c_int]
        lib.nolzss_profile_report.argtypes = [C.c_int, C.c_char_p, sz]
        lib.nolzss_last_error.restype = C.c_char_p

    def check(self, rc):
        if rc:
            raise RuntimeError(f"parent library: status {rc}: {self.lib.nolzss_last_error().decode(errors='replace')}")

    def report(self):
        buf = C.create_string_buffer(1 << 16)
        self.check(self.lib.nolzss_profile_report(0, buf, len(buf)))
        return {name: (int(count), float(ms), float(nbytes))
                for name, count, ms, nbytes in (line.split() for line in buf.value.decode().splitlines())}


def profiled(fn, enable, reset, report):
    enable(True)
    try:
        reset()
        t, out = timed(fn)
        return t, out, report()
    finally:
        enable(False)
        reset()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=str(ROOT / "nolzss_amd" / "libnolzss_hip.parent.so"))
    ap.add_argument("--lg", type=int, default=24)
    ap.add_argument("--lgreads", type=int, default=18)
    ap.add_argument("--lgcontigs", type=int, default=12)
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "r17_rlz_index_consensus.txt"))
    a = ap.parse_args()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    lib = _lib.lib
    native.set_device(0)
    values = (20, 64, 5000, 31, 40, 16, 256)
    aparams = native._align_params(*values)
    ref_arr = gen.random_dna(1 << a.lg, 0x524C5A)
    ref = ref_arr.tobytes()
    B = len(ref)
    say(f"relative-LZ index consensus probe: reference 2^{a.lg} bases, reverse complement on, min_length 20, max_hits 64, "
        f"max_gap 5000, bandwidth 31, min_score 40, band 16, max_flank 256, primary_only")
    ix = native.RlzIndexHandle.open(ref, with_rc=True)
    parent = Parent(a.parent) if Path(a.parent).exists() else None
    p_ix = C.c_void_p()
    if parent:
        parent.check(parent.lib.nolzss_rlz_index_open(*native._seq_args([ref], "reference"), 1, 0, 0, C.byref(p_ix)))
        say(f"parent library: {Path(a.parent).name}, its own index handle on the same device")
    else:
        say(f"parent library {a.parent} not found: no comparison with the parent commit in this run")

    sets = (("reads", 1 << a.lgreads, 150, 0.01, 1), ("contigs", 1 << a.lgcontigs, 10_000, 0.001, 2))
    for label, k, length, rate, seed in sets:
        targets = [row.tobytes() for row in cuts(ref_arr, k, length, rate, seed)]
        args = native._seq_args(targets, "target")
        plain = native.RlzPileupHandle.open(ix, *values)
        normal = native.RlzPileupHandle.open(ix, *values, normalize_indels=True)
        p_pile = C.c_void_p()
        if parent:
            parent.check(parent.lib.nolzss_rlz_pileup_open(p_ix, C.byref(aparams), C.byref(p_pile)))

        def add_to(pile):
            def add():
                info = _lib.RlzPileupAddInfo()
                _lib.check(lib.nolzss_rlz_pileup_add(pile._handle(), *args, 1, C.byref(info)))
                return info.alignments
            return add

        def add_parent():
            info = _lib.RlzPileupAddInfo()
            parent.check(parent.lib.nolzss_rlz_pileup_add(p_pile, *args, 1, C.byref(info)))
            return info.alignments

        arms = ([("parent", add_parent)] if parent else []) + [("flags 0", add_to(plain)), ("normalize", add_to(normal))]
        say()
        say(f"---- {label}: {k} targets of {length} bases, substitution rate {rate}")
        kept = {name: fn() for name, fn in arms}  # warm-up of every arm
        assert len(set(kept.values())) == 1, kept
        say(f"alignments kept per add: {kept['flags 0']}; insertion events per add: {plain.info['insertion_events']} "
            f"({plain.info['log_bytes'] / 2**20:.2f} MiB of log after the first add)")
        times = {name: [] for name, _ in arms}
        for _ in range(a.pairs):
            for name, fn in arms:
                times[name].append(timed(fn)[0])
        for name, _ in arms:
            say(f"add {name:10s} median {statistics.median(times[name]):9.2f} ms   {['%.2f' % t for t in times[name]]}")
        if parent:
            for name in ("flags 0", "normalize"):
                diffs = [t - p for t, p in zip(times[name], times["parent"])]
                say(f"{name} - parent per round: {['%+.2f' % d for d in diffs]} ms; median {statistics.median(diffs):+.2f} ms, "
                    f"spread {max(diffs) - min(diffs):.2f} ms ({statistics.median(diffs) / statistics.median(times['parent']):+.4f} of the "
                    f"parent's median)")
            again = [timed(add_parent)[0] for _ in range(a.pairs)]
            say(f"parent against itself, {a.pairs} more adds: median {statistics.median(again):.2f} ms, "
                f"{statistics.median(again) - statistics.median(times['parent']):+.2f} ms from its median above")

        reports = {}
        for name, fn in arms:
            if name == "parent":
                _, _, reports[name] = profiled(fn, lambda on: parent.check(parent.lib.nolzss_profile_enable(0, 1 if on else 0)),
                                               lambda: parent.check(parent.lib.nolzss_profile_reset(0)), parent.report)
            else:
                _, _, reports[name] = profiled(fn, native.profile_enable, native.profile_reset, native.profile_report)
        say("scope rows of one add (launches, device ms): parent | flags 0 | normalize")
        for scope in sorted(set().union(*reports.values()), key=lambda s: -reports["flags 0"].get(s, (0, 0.0, 0))[1]):
            cells = ["%5d %9.3f" % reports[name][scope][:2] if scope in reports[name] else " " * 15 for name, _ in arms]
            added = "   <- added" if parent and scope not in reports["parent"] else ""
            say(f"  {scope:28s} " + " | ".join(cells) + added)
        span = reports["flags 0"].get("rlz_pileup_add", (0, 0.0, 0))[1]
        for scope in NEW_SCOPES:
            row = [reports[name].get(scope, (0, 0.0, 0))[1] for name, _ in arms]
            say(f"scope {scope:24s} " + " / ".join("%.3f" % v for v in row) + f" ms ({' / '.join(n for n, _ in arms)}); "
                f"flags 0: {row[-2] / max(span, 1e-9):.4f} of the add's device span ({span:.3f} ms)")

        t_ins, (found, rep_i) = timed(lambda: profiled(lambda: normal.insertions(2, (1, 2)), native.profile_enable,
                                                        native.profile_reset, native.profile_report)[1:])
        t_again, _ = timed(lambda: normal.insertions(2, (1, 2)))
        t_cons, (cons, rep_c) = timed(lambda: profiled(lambda: normal.consensus(1, (1, 2), "reference", False), native.profile_enable,
                                                        native.profile_reset, native.profile_report)[1:])
        say(f"insertions(2, 1, 2): {t_ins:.1f} ms with the resolve and the allele table of {normal.info['insertion_events']} events, "
            f"{t_again:.1f} ms from the kept table; {len(found)} records, {found.nbytes / 1e6:.3f} MB down")
        text_bytes = sum(len(r) for r in cons["records"])
        say(f"consensus(1, 1/2): {t_cons:.1f} ms; {text_bytes / 1e6:.2f} MB of text down against {32 * B / 1e6:.1f} MB that counts() of the "
            f"block would bring down ({text_bytes / (32 * B):.4f}); called {cons['called']}, low {cons['low_positions']}, substitutions "
            f"{cons['substitutions']}, deleted {cons['deleted']}, insertions {cons['insertions']} ({cons['inserted_bases']} bases)")
        for rep_r in (rep_i, rep_c):
            for scope in READ_SCOPES:
                if scope in rep_r:
                    say(f"read scope {scope:28s} {rep_r[scope][0]:5d} launches {rep_r[scope][1]:9.3f} ms")
        plain.close()
        normal.close()
        if parent:
            parent.check(parent.lib.nolzss_rlz_pileup_close(p_pile))
    if parent:
        parent.check(parent.lib.nolzss_rlz_index_close(p_ix))
    ix.close()
    say()
    say("no counter run was made")
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
