#!/usr/bin/env python3
"""Relative-LZ archive: what the compact container costs and saves beside the .npz.

    python tools/rlz_archive_pack_probe.py [--lg 20] [--targets 300] [--reps 5] [--dir DIR]
                                           [--out profiles/r19_rlz_archive_pack.txt]

One process, one device.  An index-built archive of a planted collection: one reference of 2^lg random bases and
--targets targets, each the reference with 0.1 % of its positions redrawn, two indels and, every eighth target, one
reverse-complemented segment.  Medians of --reps after a warm-up of every arm.
  (a) save(path, compact=True) and load of that file beside save(path) and load of the .npz.  The .npz arm IS the
      parent commit's code path, which this commit leaves as it was (export of the 24-byte records, numpy.savez;
      numpy.load, open_records), run in the same process on the same archive.  Wall times, and the bytes that cross PCIe.
  (b) the device time of the stages of both arms from nolzss_profile_report.
  (c) file sizes: compact against the .npz, against numpy.savez_compressed of the same arrays and against the targets
      at 2 bits per base; the share of the records in every nibble class.
Runs on the GPU machine only.  No figure is asserted: the byte-exact model test pins the size.  No counter run.
"""
import argparse
import os
import statistics
import sys
import tempfile
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
sys.path.insert(0, str(ROOT / "tools"))

import numpy as np  # noqa: E402

import gen  # noqa: E402
import rlz_model  # noqa: E402
from nolzss_amd import _noLZSS as native  # noqa: E402
from nolzss_amd.genomics import rlz  # noqa: E402
from rlz_probe import mutated, timed  # noqa: E402

PACK_SCOPES = ("rlz_archive_pack_all", "rlz_packed_plan", "rlz_packed_write", "rlz_archive_literal_index",
               "rlz_packed_literals", "rlz_packed_block", "packed_d2h")
OPEN_SCOPES = ("rlz_archive_open_packed", "packed_h2d", "rlz_unpack_block", "rlz_unpack_sizes", "rlz_unpack_records",
               "rlz_append_sample")
EXPORT_SCOPES = ("rlz_archive_export_all", "block_d2h", "rlz_archive_literal_index", "rlz_archive_export", "factors_d2h")
RECORDS_SCOPES = ("rlz_archive_open", "records_h2d", "rlz_archive_check", "rlz_archive_pack")


def planted(ref, j):
    t = mutated(ref, 7000 + j)
    r = np.random.default_rng(90_000 + j)
    a, b = sorted(int(x) for x in r.integers(1000, len(t) - 1000, 2))
    t = np.concatenate([t[:a], t[a + 7:b], gen.random_dna(11, 100 + j), t[b:]])  # a deletion of 7, an insertion of 11
    if j % 8 == 0:
        c = int(r.integers(1000, len(t) - 5000))
        t[c:c + 3000] = np.frombuffer(rlz_model.revcomp(t[c:c + 3000].tobytes()), dtype=np.uint8)
    return t.tobytes()


def profiled(fn):
    native.profile_enable(True)
    try:
        native.profile_reset()
        t, out = timed(fn)
        return t, out, native.profile_report()
    finally:
        native.profile_enable(False)
        native.profile_reset()


def arm(say, name, fn, reps, scopes, after=None):
    fn_out = fn()  # warm-up
    if after:
        after(fn_out)
    walls, reports = [], []
    for _ in range(reps):
        t, out, rep = profiled(fn)
        if after:
            after(out)
        walls.append(t)
        reports.append(rep)
    say(f"{name}: wall median {statistics.median(walls):.2f} ms {['%.2f' % t for t in walls]}")
    cells = [f"{s} {statistics.median(r.get(s, (0, 0.0, 0))[1] for r in reports):.3f}" for s in scopes]
    say(f"    device spans (ms, medians; a stage and the kernels inside it are separate scopes): " + ", ".join(cells))
    return statistics.median(walls)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lg", type=int, default=20)
    ap.add_argument("--targets", type=int, default=300)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--dir", default=None, help="where the files go (default: a temporary directory)")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "r19_rlz_archive_pack.txt"))
    a = ap.parse_args()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    def flush():
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text("\n".join(lines) + "\n")

    native.set_device(0)
    ref = gen.random_dna(1 << a.lg, 0x524C5A)
    targets = [planted(ref, j) for j in range(a.targets)]
    bases = sum(len(t) for t in targets)
    say(f"relative-LZ archive pack probe: reference 2^{a.lg} bases, {a.targets} targets ({bases / 1e6:.1f} M bases): 0.1 % of the "
        f"positions redrawn, two indels each, a reverse-complemented segment of 3000 in every eighth; medians of {a.reps} after a warm-up")
    tmp = tempfile.TemporaryDirectory(dir=a.dir)
    compact, npz = Path(tmp.name) / "a.rlz", Path(tmp.name) / "a.npz"
    with rlz.RlzIndex.build(ref.tobytes()) as ix:
        t_build, arc = timed(lambda: ix.archive_on_device(targets, ids=[f"t{j}" for j in range(a.targets)]))
        with arc:
            info = arc.info
            z, nlit, B = info["z"], info["n_literals"], info["block_length"]
            say(f"the archive: {z} records ({bases / z:.0f} bases each), {nlit} literals, block {B} bytes, resident "
                f"{info['device_bytes'] / 1e6:.1f} MB; built on the device in {t_build / 1e3:.2f} s")
            say()
            say("---- (a), (b) save and load; the .npz arm is the parent commit's code path, unchanged here")
            t_sc = arm(say, "save(compact=True)", lambda: arc.save(compact, compact=True), a.reps, PACK_SCOPES)
            t_sn = arm(say, "save()  [.npz]    ", lambda: arc.save(npz), a.reps, EXPORT_SCOPES)
            t_lc = arm(say, "load(compact file)", lambda: rlz.RlzArchive.load(compact), a.reps, OPEN_SCOPES, lambda x: x.close())
            t_ln = arm(say, "load(.npz)        ", lambda: rlz.RlzArchive.load(npz), a.reps, RECORDS_SCOPES, lambda x: x.close())
            say(f"save: compact / npz = {t_sc / t_sn:.2f}; load: compact / npz = {t_lc / t_ln:.2f}")
            s, lengths, _ = rlz.read_packed_archive(compact)
            sections = sum(len(s[k]) for k in ("block", "control", "data", "literals"))
            say(f"bytes across PCIe, each way: compact {sections} (block {len(s['block'])}, control {len(s['control'])}, data "
                f"{len(s['data'])}, literals {len(s['literals'])}); .npz path {B + 24 * z + nlit} (block {B}, records {24 * z}, "
                f"literals {nlit})")
            with rlz.RlzArchive.load(compact) as loaded:
                probe = [(j, 0, len(targets[j])) for j in (0, 8, a.targets - 1)]
                assert loaded.extract(probe) == [targets[j] for j, _, _ in probe] == arc.extract(probe)
            say("three whole targets of the loaded compact archive equal their inputs")
            flush()

            say()
            say("---- (c) sizes")
            block, records, literals = arc._live().export()
            arrays = rlz.archive_arrays(block, records, literals, arc._live().target_lengths, arc.ids)
            packed_npz = Path(tmp.name) / "c.npz"
            t_z, _ = timed(lambda: np.savez_compressed(packed_npz, **{k: arrays[k] for k in rlz.ARCHIVE_ARRAYS}))
            sc, sn, sz = (os.path.getsize(p) for p in (compact, npz, packed_npz))
            say(f"compact file {sc} bytes; .npz {sn} bytes ({sn / sc:.2f} x); numpy.savez_compressed of the same arrays {sz} bytes "
                f"({sz / sc:.2f} x, written in {t_z:.0f} ms); the targets at 2 bits per base {bases // 4} bytes ({bases / 4 / sc:.1f} x)")
            say(f"per record: compact {(len(s['control']) + len(s['data'])) / z:.2f} bytes of control and data, .npz 24; modes: block "
                f"{s['block_mode']} ({s['num_separators']} separators), literals {s['literal_mode']}")
            nib = np.frombuffer(s["control"], dtype=np.uint8)
            nib = np.stack([nib & 15, nib >> 4], axis=1).reshape(-1)[:z]
            share = np.bincount(nib, minlength=16) / z
            say("share of the records per nibble class (a: bytes of L, b: bytes of v):")
            for code in range(16):
                if share[code]:
                    what = "literal" if code == 0 else f"L in {(0, 1, 2, 4)[code & 3]}, v in {(0, 1, 3, 5)[code >> 2]}"
                    say(f"    a = {code & 3}, b = {code >> 2} ({what}): {100 * share[code]:.2f} %")
    tmp.cleanup()
    say()
    say("no counter run was made")
    flush()


if __name__ == "__main__":
    main()
