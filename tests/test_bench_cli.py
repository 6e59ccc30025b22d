"""bench.py's command line and output dump (no GPU): --steps sets the timed
steps, without --full the options of every pass beside them are switched
off, --dump-outputs writes exact float64 arrays within its size budget."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import bench  # noqa: E402


def _parse(monkeypatch, *argv):
    monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
    return bench.parse()


def test_steps_and_full_options(monkeypatch):
    a = _parse(monkeypatch, "--gpus", "1", "--steps", "7", "--warmup", "2")
    assert (a.gpus, a.steps, a.warmup) == (1, 7, 2)
    assert a.full is False and a.dump_outputs is None
    a = _parse(monkeypatch, "--full", "--dump-outputs", "somewhere")
    assert a.full is True and a.dump_outputs == "somewhere"
    assert a.steps == 1000  # the C2 default


def test_plain_run_switches_the_other_passes_off(monkeypatch):
    # whatever the pass options say, a run without --full has none of them
    for argv in ([], ["--profile-steps", "30", "--latency-steps", "9", "--index-stats"],
                 ["--workload", "c5"], ["--workload", "c3", "--cpu-seconds", "4"]):
        a = _parse(monkeypatch, *argv)
        assert a.no_cpu_baseline is True and a.index_stats is False
        assert a.profile_steps == 0 and a.latency_steps == 0
    # with --full they are what the command line says, else today's defaults
    a = _parse(monkeypatch, "--full")
    assert a.no_cpu_baseline is False and a.index_stats is False
    assert a.profile_steps == 10 and a.latency_steps is None
    assert _parse(monkeypatch, "--full", "--workload", "c5").profile_steps == 60
    a = _parse(monkeypatch, "--full", "--no-cpu-baseline", "--profile-steps", "0",
               "--latency-steps", "0", "--index-stats")
    assert a.no_cpu_baseline is True and a.index_stats is True
    assert a.profile_steps == 0 and a.latency_steps == 0


def test_dump_outputs_writes_exact_float64(tmp_path, monkeypatch):
    import torch
    vals = torch.tensor([0, 2, (1 << 53) - 1, 2 << 26], dtype=torch.int64)
    found = torch.tensor([0, 1, 1, 1], dtype=torch.uint8)
    d = str(tmp_path / "out")
    bench.dump_outputs(d, {"values": vals, "found": found}, "")
    v, f = np.load(os.path.join(d, "values.npy")), np.load(os.path.join(d, "found.npy"))
    assert v.dtype == np.float64 and f.dtype == np.float64
    assert v.astype(np.uint64).tolist() == vals.tolist() and f.tolist() == [0.0, 1.0, 1.0, 1.0]
    # the element budget is shared among the arrays of all ranks: each array
    # is cut to its leading elements; ranks get their own files
    monkeypatch.setattr(bench, "DUMP_MAX_VALUES", 12)
    bench.dump_outputs(d, {"values": vals, "found": found}, "_rank1", world=2)
    assert np.load(os.path.join(d, "values_rank1.npy")).tolist() == [0.0, 2.0, float((1 << 53) - 1)]
    assert np.load(os.path.join(d, "found_rank1.npy")).tolist() == [0.0, 1.0, 1.0]
    # a value float64 cannot hold is refused, not rounded (-1 is 2^64 - 1)
    with pytest.raises(ValueError):
        bench.dump_outputs(d, {"values": torch.tensor([-1], dtype=torch.int64)}, "")


def test_dump_budget_is_below_64_mb():
    # float64 elements plus a .npy header per array, at up to 8 ranks x 2 arrays
    assert bench.DUMP_MAX_VALUES * 8 + 16 * 128 <= 64 * 10**6
