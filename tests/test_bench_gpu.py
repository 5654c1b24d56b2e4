"""bench.py's plain line (headline keys only, --steps timed steps in one window) and --dump-outputs: what the last timed vector step
handed its caller, the same on every run with the same arguments."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")
FULL_ONLY = ("roofline", "roofline_env_step", "clock", "also", "learner_only", "cpu_baseline", "all_reduce_ms", "timeouts")


@pytest.fixture(scope="module")
def torch():
    import torch as t
    if not t.cuda.is_available():
        pytest.skip("no GPU")
    return t


def _bench(args, timeout=600):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1"] + args, capture_output=True, text=True, timeout=timeout, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    return json.loads(lines[0])


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_plain_line_and_dumped_outputs_repeat(torch, tmp_path):
    """A plain run times exactly --steps vector steps (one window) and carries the headline keys only; --dump-outputs writes obs / reward /
    done / info of the last timed step (4 096 envs), the loss of its last gradient step and the network's parameters, float32, and a
    second run with the same arguments writes the same arrays."""
    from distributional_rl_navigation_amd.iqn.fused_train import P_TOTAL
    n, steps = 4096, 16
    runs = []
    for r in range(2):
        d = str(tmp_path / f"run{r}")
        j = _bench(["--envs", str(n), "--steps", str(steps), "--warmup", "4", "--dump-outputs", d])
        assert all(k in j for k in HEADLINE) and not any(k in j for k in FULL_ONLY)
        assert j["steps"] == steps and j["windows"]["n"] == 1 and j["higher_is_better"] is True
        assert abs(j["value"] - n * 1e3 / j["ms_per_step"]) <= 2e-3 * j["value"]
        assert j["config"]["resets"] == "under_next_act" and j["grad_steps_per_sec"] > 0
        runs.append(_load(d))
    a, b = runs
    assert sorted(a) == ["done", "info", "loss", "obs", "q_params", "reward"]
    assert all(v.dtype == np.float32 for v in a.values())
    assert a["obs"].shape == (n, 26) and a["reward"].shape == a["done"].shape == a["info"].shape == (n,) and a["q_params"].shape == (P_TOTAL,)
    assert np.isfinite(a["obs"]).all() and np.isfinite(a["loss"]).all() and set(np.unique(a["done"])) <= {0.0, 1.0}
    for k in a:
        assert np.array_equal(a[k], b[k]), k


def test_rollout_dump_outputs(torch, tmp_path):
    """--no-learner --rollout T: the final observations and the last step of every trace the launch wrote."""
    n = 4096
    d = str(tmp_path / "roll")
    j = _bench(["--no-learner", "--envs", str(n), "--steps", "8", "--warmup", "4", "--rollout", "4", "--dump-outputs", d])
    assert j["steps"] == 8 and j["windows"]["n"] == 1 and "roofline" not in j
    o = _load(d)
    assert sorted(o) == ["done_last_step", "obs", "obs_last_step", "reward_last_step"]
    assert o["obs"].shape == o["obs_last_step"].shape == (n, 26) and o["reward_last_step"].shape == (n,)
