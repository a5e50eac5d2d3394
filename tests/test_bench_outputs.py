"""bench.py's plain line and --dump-outputs, on the CPU: the library is replaced by a stand-in that returns the oracle's
factors, so what is checked is the benchmark's own logic -- a plain run times exactly --steps steps and runs nothing
beside them, --full adds the side runs, and the dumped arrays are float64, bounded, seeded and describe every record."""
import importlib
import sys
import types

import numpy as np
import pytest

import oracle_lib as oracle


class _Parsed(Exception):
    pass


@pytest.fixture
def bench(monkeypatch):
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    return importlib.import_module("bench")


def parse(bench, monkeypatch, argv):
    """the namespace main() builds from argv (stopped before it touches torch or a device)"""
    monkeypatch.setattr(bench, "late_imports", lambda: None)
    monkeypatch.setattr(bench, "Job", lambda a: (_ for _ in ()).throw(_Parsed(a)))
    monkeypatch.setattr(sys, "argv", ["bench.py"] + argv)
    with pytest.raises(_Parsed) as e:
        bench.main()
    return e.value.args[0]


class FakeNative:
    """the entry points bench.py calls, answering with the oracle's result for the text"""

    def __init__(self, factors=None, batch_counts=None):
        self.factors, self.batch_counts, self.calls = factors, batch_counts, []

    def factorize_device(self, ptr, n, emit=2):
        self.calls.append(("factorize_device", emit))
        return len(self.factors), (self.factors if emit == 2 else None)

    def factorize_batch_device(self, ptrs, lens, emit=0):
        self.calls.append(("factorize_batch_device", emit))
        return list(self.batch_counts)

    def factorize_batch(self, recs, want_factors=True):
        self.calls.append(("factorize_batch", want_factors))
        return list(self.batch_counts), None

    def debug_lpt_plan(self, lens, world):
        return [0] * len(lens)

    def profile_enable(self, on):
        self.calls.append(("profile_enable", on))

    def profile_reset(self):
        pass

    def profile_report(self):
        return {}


def cpu_job():
    import torch
    cpu = torch.device("cpu")
    return types.SimpleNamespace(world=1, rank=0, local_rank=0, collectives=False, backend="gloo", dev=cpu, cdev=cpu,
                                 barrier=lambda: None, max_over_ranks=lambda s: s)


def single_sequence(bench, monkeypatch, argv, log2n=14):
    import torch
    a = parse(bench, monkeypatch, ["--log2n", str(log2n)] + argv)
    text = bench.make_text(a.workload, 1 << a.log2n, 0)
    fake = FakeNative(factors=oracle.factors_array(text.tobytes()))
    monkeypatch.setattr(bench, "torch", torch)
    monkeypatch.setattr(bench, "native", fake)
    monkeypatch.setattr(bench, "measure_copy_ceiling", lambda dev: 1.0)
    out, _, z = bench.run_single_sequence(cpu_job(), a)
    return a, out, z, fake


def test_defaults_are_a_plain_run(bench, monkeypatch):
    a = parse(bench, monkeypatch, ["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 2, False, None)
    a = parse(bench, monkeypatch, ["--steps", "1", "--full", "--dump-outputs", "d"])
    assert a.full and a.dump_outputs == "d"


def test_plain_run_times_the_steps_and_nothing_else(bench, monkeypatch):
    a, out, z, fake = single_sequence(bench, monkeypatch, ["--steps", "5", "--warmup", "2"])
    assert fake.calls == [("factorize_device", 1)] * 7
    for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert key in out
    assert out["steps"] == 5 and out["warmup"] == 2 and out["ms_per_step"] > 0
    assert out["value"] == pytest.approx((1 << a.log2n) / (out["ms_per_step"] * 1e-3))
    assert out["config"]["factors_per_sequence"] == z
    for key in ("roofline", "pcie_inclusive_bases_per_s", "stages_ms_per_step", "kernels_ms_per_step"):
        assert key not in out


def test_full_run_adds_the_side_measurements(bench, monkeypatch):
    _, out, _, fake = single_sequence(bench, monkeypatch, ["--steps", "3", "--warmup", "1", "--full"])
    assert fake.calls[0] == ("factorize_device", 1) and fake.calls.count(("factorize_device", 1)) == 4
    assert ("profile_enable", True) in fake.calls and fake.calls[-1] == ("factorize_device", 2)
    for key in ("roofline", "pcie_inclusive_bases_per_s", "stages_ms_per_step", "kernels_ms_per_step"):
        assert key in out


def test_dump_outputs_single_sequence(bench, monkeypatch, tmp_path):
    d = tmp_path / "out"
    a, out, z, fake = single_sequence(bench, monkeypatch, ["--steps", "2", "--warmup", "0", "--dump-outputs", str(d)])
    assert fake.calls == [("factorize_device", 1)] * 2 + [("factorize_device", 2)]
    n, f = 1 << a.log2n, fake.factors
    got = {p.stem: np.load(p) for p in d.glob("*.npy")}
    assert set(got) == {"factor_counts", "sample_positions", "factors_sample", "block_sums"}
    assert all(v.dtype == np.float64 for v in got.values())
    assert got["factor_counts"].tolist() == [z]
    pos, s = got["sample_positions"], got["factors_sample"]
    assert np.all(np.diff(pos) > 0) and pos[0] >= 0 and pos[-1] < n
    assert np.all(s[:, 0] <= pos) and np.all(pos < s[:, 0] + s[:, 1])  # the factor that covers the position
    rows = {int(x) for x in f["start"]}
    assert all(int(x) in rows for x in s[:, 0])
    b = got["block_sums"]
    assert b.shape == (bench.DUMP_BLOCKS, 3)
    assert b[:, 0].sum() == z and b[:, 1].sum() == n and b[:, 2].sum() == float(f["ref"].astype(np.float64).sum())
    # the same arguments write the same arrays
    again = bench.factor_outputs(f, n, [z])
    assert all(np.array_equal(np.asarray(again[k], dtype=np.float64), got[k]) for k in got)


def test_dump_outputs_stay_within_the_limit(bench, tmp_path):
    # at the headline size: 2^20 sample positions (8 B) and rows (24 B), the block sums and the counts of 8 ranks
    worst = bench.DUMP_SAMPLE * 4 * 8 + bench.DUMP_BLOCKS * 3 * 8 + 8 * 8
    assert worst <= bench.DUMP_LIMIT_BYTES
    with pytest.raises(SystemExit):
        bench.write_outputs(tmp_path, {"x": np.zeros(bench.DUMP_LIMIT_BYTES // 8 + 1)})


def test_fasta512_plain_run_and_dump(bench, monkeypatch, tmp_path):
    import torch
    d = tmp_path / "out"
    a = parse(bench, monkeypatch, ["--workload", "fasta512", "--steps", "3", "--warmup", "1", "--fasta-records", "4",
                                   "--fasta-record-log2", "10", "--dump-outputs", str(d)])
    a.fasta_steps, a.fasta_warmup = a.steps, a.warmup
    fake = FakeNative(batch_counts=[11, 12, 13, 14])
    monkeypatch.setattr(bench, "torch", torch)
    monkeypatch.setattr(bench, "native", fake)
    fa = bench.run_fasta_shard(cpu_job(), a, headline=True)
    assert fake.calls == [("factorize_batch_device", 1)] * 4  # no host-buffer run, no file path
    assert fa["steps"] == 3 and fa["ms_per_step"] > 0 and fa["total_factors"] == 50
    counts = np.load(d / "factor_counts.npy")
    assert counts.dtype == np.float64 and counts.tolist() == [11, 12, 13, 14]
