"""bench.py's command line and its output dump, without a GPU: a plain run times one block of exactly --steps steps, --full
restores the five blocks, and --dump-outputs writes float32 .npy files within 64 MB, sampled the same way in every run."""
import os

import numpy as np
import pytest
import torch

import bench


def test_plain_run_times_one_block_of_steps():
    a = bench.parse(["--gpus", "1", "--steps", "7", "--warmup", "3"])
    assert (a.steps, a.warmup, a.reps, a.full, a.dump_outputs) == (7, 3, 1, False, None)
    assert bench.parse(["--full"]).reps == 5
    assert bench.parse(["--full", "--reps", "2"]).reps == 2
    assert bench.parse(["--dump-outputs", "d"]).dump_outputs == "d"
    with pytest.raises(SystemExit):
        bench.parse(["--steps", "0"])


def test_dump_outputs_writes_everything_below_the_limit(tmp_path):
    x = torch.randn(4, 16, 3)
    bench.dump_outputs(str(tmp_path), {"poses": x, "logits": torch.ones(4, 1, dtype=torch.bfloat16)})
    assert sorted(os.listdir(tmp_path)) == ["logits.npy", "poses.npy"]
    p = np.load(tmp_path / "poses.npy")
    assert p.dtype == np.float32 and p.shape == (4, 16, 3) and np.array_equal(p, x.numpy())
    assert np.load(tmp_path / "logits.npy").dtype == np.float32


def test_dump_outputs_samples_large_outputs_reproducibly(tmp_path):
    arrays = {"a": torch.arange(3000.0), "b": torch.arange(1000.0)}
    limit = 4 * 400
    for d in ("r1", "r2"):
        bench.dump_outputs(str(tmp_path / d), arrays, limit_bytes=limit)
    a1, b1 = np.load(tmp_path / "r1" / "a.npy"), np.load(tmp_path / "r1" / "b.npy")
    assert a1.size + b1.size <= 400 and a1.size == 3 * b1.size
    assert np.array_equal(a1, np.load(tmp_path / "r2" / "a.npy")) and np.array_equal(b1, np.load(tmp_path / "r2" / "b.npy"))
    assert np.all(np.diff(a1) >= 0) and a1.max() < 3000
