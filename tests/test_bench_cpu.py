"""bench.py's host-side pieces that need no GPU: the --dump-outputs writer and the plain / --full defaults."""
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _arrays(torch, n):
    g = torch.Generator().manual_seed(3)
    return {"obs": torch.randn(n, 26, generator=g), "reward": torch.randn(n, generator=g),
            "done": torch.randint(0, 2, (n,), dtype=torch.uint8, generator=g), "loss": torch.tensor(0.25),
            "q_params": torch.randn(500, generator=g), "absent": None}


def test_dump_outputs_writes_float32_and_samples_envs_within_the_budget(tmp_path):
    """Every array lands as float32 <name>.npy; above the byte budget the per-env arrays keep the same fixed, seeded rows (env_index.npy) and
    the other arrays stay whole."""
    import torch
    import bench
    n = 1000
    arrays = _arrays(torch, n)
    bench.dump_outputs(str(tmp_path / "all"), arrays, n)
    names = sorted(os.listdir(tmp_path / "all"))
    assert names == ["done.npy", "loss.npy", "obs.npy", "q_params.npy", "reward.npy"]
    for k in ("obs", "reward", "done", "q_params"):
        a = np.load(tmp_path / "all" / f"{k}.npy")
        assert a.dtype == np.float32 and np.array_equal(a, arrays[k].float().numpy())
    assert np.load(tmp_path / "all" / "loss.npy") == np.float32(0.25)

    budget = 60_000
    for d in ("s1", "s2"):
        bench.dump_outputs(str(tmp_path / d), arrays, n, budget=budget)
    idx = np.load(tmp_path / "s1" / "env_index.npy")
    assert idx.dtype == np.float64 and np.array_equal(idx, np.load(tmp_path / "s2" / "env_index.npy"))
    rows = idx.astype(np.int64)
    assert 0 < len(rows) < n and np.all(np.diff(rows) > 0) and rows[-1] < n
    total = sum(np.load(tmp_path / "s1" / f).nbytes for f in os.listdir(tmp_path / "s1"))
    assert total <= budget
    assert np.array_equal(np.load(tmp_path / "s1" / "obs.npy"), arrays["obs"].numpy()[rows])
    assert np.array_equal(np.load(tmp_path / "s1" / "done.npy"), arrays["done"].float().numpy()[rows])
    assert np.array_equal(np.load(tmp_path / "s1" / "q_params.npy"), arrays["q_params"].numpy())


def test_bench_offers_full_and_dump_outputs():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    text = out.stdout + out.stderr      # (bench.py sends everything but its result line to stderr)
    assert "--full" in text and "--dump-outputs" in text
