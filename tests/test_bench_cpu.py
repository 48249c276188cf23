"""bench.py's command line and its --dump-outputs writer, without a GPU."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import bench  # noqa: E402


def test_steps_set_the_timed_steps_exactly():
    a = bench.parse(["--gpus", "1", "--steps", "7", "--warmup", "3"])
    assert a.steps == 7 and a.warmup == 3 and a.repeats == 1 and a.dump_outputs is None
    a = bench.parse(["--steps", "7", "--repeats", "3", "--dump-outputs", "out"])
    assert a.repeats == 3 and a.dump_outputs == "out"


def test_dump_outputs_writes_the_whole_state_under_the_limit(tmp_path):
    x = torch.arange(6 * 8, dtype=torch.float64).reshape(6, 8)
    shapes = bench.dump_outputs(str(tmp_path / "d"), x, 0.02)
    assert shapes == {"clock": [1], "state": [6, 8]}
    got = np.load(tmp_path / "d" / "state.npy")
    assert got.dtype == np.float64 and np.array_equal(got, x.numpy())
    assert np.load(tmp_path / "d" / "clock.npy").tolist() == [0.02]
    assert not (tmp_path / "d" / "state_rows.npy").exists()


def test_dump_outputs_samples_a_fixed_set_of_beams_over_the_limit(tmp_path):
    x = torch.arange(1000 * 16, dtype=torch.float32).reshape(1000, 16)
    limit = 4096 + 100 * (16 * 4 + 8)
    shapes = bench.dump_outputs(str(tmp_path / "a"), x, 1.0, limit=limit)
    bench.dump_outputs(str(tmp_path / "b"), x, 1.0, limit=limit)
    assert shapes["state"] == [100, 16] and shapes["state_rows"] == [100]
    rows = np.load(tmp_path / "a" / "state_rows.npy")
    state = np.load(tmp_path / "a" / "state.npy")
    assert state.dtype == np.float32 and rows.dtype == np.float64
    assert np.all(np.diff(rows) > 0) and np.array_equal(state, x.numpy()[rows.astype(np.int64)])
    assert np.array_equal(rows, np.load(tmp_path / "b" / "state_rows.npy"))     # the same sample every run
    total = sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a"))
    assert total <= limit
