"""Host checks of bench.py's command line and its --dump-outputs writer (no GPU)."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def test_plain_run_is_lean_by_default(monkeypatch):
    """--full and --dump-outputs are off unless given; --steps / --warmup set the step counts."""
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"])
    a = bench.parse()
    assert (a.gpus, a.steps, a.warmup) == (1, 7, 2)
    assert a.full is False and a.dump_outputs is None
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "d"])
    a = bench.parse()
    assert a.full is True and a.dump_outputs == "d"


def test_dump_outputs_writes_float32(tmp_path):
    """An fp16 output comes back as float32 with the same values and shape."""
    t = torch.randn(4, 4, 8, 8, generator=torch.Generator().manual_seed(0)).half()
    bench.dump_outputs(str(tmp_path / "o"), {"latents": t})
    a = np.load(tmp_path / "o" / "latents.npy")
    assert a.dtype == np.float32 and a.shape == (4, 4, 8, 8)
    assert np.array_equal(a, t.float().numpy())


def test_dump_outputs_samples_within_budget(tmp_path, monkeypatch):
    """Arrays above the size budget are cut to a fixed sample (same elements every run); the files
    of one dump stay within the budget in all."""
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 4096)
    g = torch.Generator().manual_seed(1)
    big, small = torch.randn(5000, generator=g), torch.randn(100, generator=g)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"big": big, "small": small})
    a, b = np.load(tmp_path / "a" / "big.npy"), np.load(tmp_path / "b" / "big.npy")
    assert a.dtype == np.float32 and a.size == 2048 // 4 and np.array_equal(a, b)
    assert np.isin(a, big.numpy()).all()
    s = np.load(tmp_path / "a" / "small.npy")
    assert np.array_equal(s, small.numpy())
    assert a.nbytes + s.nbytes <= 4096
