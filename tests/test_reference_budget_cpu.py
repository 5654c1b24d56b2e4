"""`plan_cadence(budget="reference")` / `train_dqn.make_plan(budget="reference")`: the reference's own experiment -- env-step budget, replay ratio,
cadences, evaluation timesteps -- cut into vector steps; the default budget is untouched; both drivers print the plan without a GPU."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from distributional_rl_navigation_amd import train_dqn
from distributional_rl_navigation_amd.train_iqn import plan_cadence, plan_eval_points

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN_CURVE = os.path.join(ROOT, "tests", "golden", "ref_iqn_seed3_greedy_curve.npz")


@pytest.mark.parametrize("N", [4, 80, 400])
def test_iqn_reference_plan(N):
    p = plan_cadence(3_000_000, 10_000, N, 32, budget="reference")
    assert p["vector_steps"] == 3_000_000 // N and p["vector_steps"] * N == 3_000_000 and p["env_steps"] == 3_000_000
    assert p["batch"] == 32 and p["grad_steps_per_vector_step"] == N // 4
    assert p["learning_starts"] == 10_000 and p["learning_starts_vector_steps"] * N == 10_000
    assert p["total_grad_steps"] == 747_500 == (p["vector_steps"] - p["learning_starts_vector_steps"]) * p["grad_steps_per_vector_step"]
    assert p["target_sync_grad_steps"] == 2_500
    assert p["replay_ratio"] == 8 == p["reference_replay_ratio"]
    assert p["timestep_scale"] == N      # the curriculum switches at 1 M and 2 M ENV steps
    assert p["exploration_timesteps"] == 300_000 and p["exploration_fraction"] == 0.1
    assert p["replay"] == 1_000_000 and p["report_timestep_scale"] == 1
    assert p["n_evals"] == 300 and p["eval_every_vector_steps"] * N == 10_000
    want = np.load(GOLDEN_CURVE)["timesteps"]
    assert len(want) == 300 and np.array_equal(np.array(p["eval_timesteps"]), want)
    assert np.array_equal(np.arange(10_000, 3_000_001, 10_000), want)
    # every evaluation follows a vector step of the run, in order, the last one the last step
    after = plan_eval_points(p, N)
    assert sorted(t for ts in after.values() for t in ts) == list(want) and max(after) == p["vector_steps"] - 1
    assert all(ts == sorted(ts) for ts in after.values()) and all(t in (it * N, 3_000_000) for it, ts in after.items() for t in ts)


def test_default_N_is_80():
    from distributional_rl_navigation_amd.train_iqn import REFERENCE_N_ENVS, resolve_budget_args
    assert REFERENCE_N_ENVS == 80 and resolve_budget_args("reference", None, None, None) == (80, 32, None)
    assert resolve_budget_args("learner", None, None, None) == (4096, 256, 100_000)
    p = plan_cadence(3_000_000, 10_000, 80, 32, budget="reference")
    assert p["grad_steps_per_vector_step"] == 20 and p["vector_steps"] == 37_500


@pytest.mark.parametrize("N", [64, 30])
def test_other_N_are_refused_with_the_nearest_valid_values(N):
    with pytest.raises(ValueError, match="nearest valid values") as e:
        plan_cadence(3_000_000, 10_000, N, 32, budget="reference")
    assert ("[40, 80]" if N == 64 else "[20, 40]") in str(e.value)


def test_contradicting_values_are_errors():
    with pytest.raises(ValueError, match="batch"):
        plan_cadence(3_000_000, 10_000, 80, 256, budget="reference")
    with pytest.raises(ValueError, match="grad_steps_per_vector_step"):
        plan_cadence(3_000_000, 10_000, 80, 32, budget="reference", grad_steps_per_vector_step=1)
    with pytest.raises(ValueError, match="n_evals"):
        plan_cadence(3_000_000, 10_000, 80, 32, budget="reference", n_evals=30)
    assert plan_cadence(3_000_000, 10_000, 80, 32, budget="reference", grad_steps_per_vector_step=20, n_evals=300)["total_grad_steps"] == 747_500
    with pytest.raises(ValueError):
        plan_cadence(3_000_000, 10_000, 80, 32, budget="other")
    with pytest.raises(ValueError, match="unknown keys"):
        plan_cadence(3_000_000, 10_000, 80, 32, budget="reference", reference=dict(learning_start=1))


def test_reference_overrides_give_the_toy_plan():
    p = plan_cadence(4_000, 400, 16, 32, budget="reference", reference=dict(learning_starts=400, target_update_interval=400))
    assert p["vector_steps"] == 250 and p["total_grad_steps"] == 900 and p["target_sync_grad_steps"] == 100
    assert p["eval_timesteps"] == list(range(400, 4_001, 400))


def test_dqn_reference_plan():
    params = dict(total_timesteps=3_000_000, eval_freq=10_000)
    for N in (4, 80, 400):
        p = train_dqn.make_plan(params, N, 32, budget="reference")
        assert p["grad_steps_per_vector_step"] == N and p["total_grad_steps"] == 2_990_000 and p["target_sync_grad_steps"] == 10_000
        assert p["learning_starts"] == 10_000 and p["vector_steps"] * N == 3_000_000
        # the loop trains behind vector step `it` once it + 1 >= learning_starts_vector_steps: (vector_steps - first) x N gradient steps
        first = p["learning_starts_vector_steps"] - 1
        assert first * N == 10_000 and (p["vector_steps"] - first) * N == 2_990_000
        assert np.array_equal(np.array(p["eval_timesteps"]), np.load(GOLDEN_CURVE)["timesteps"])
        assert p["exploration_vector_steps"] * N == 300_000
        assert train_dqn.exploration_rate(p["vector_steps"] - 1, p) == 0.05 and train_dqn.exploration_rate(0, p) == 1.0


def test_learner_budget_is_the_call_without_the_argument():
    for args, kw in (((3_000_000, 10_000, 65536, 256), {}), ((3_000_000, 10_000, 8 * 65536, 256), {}), ((3_000_000, 10_000, 1024, 256), {}),
                     ((3_000_000, 10_000, 65536, 256), dict(grad_steps_per_vector_step=4, total_grad_steps=1000, n_evals=5))):
        assert plan_cadence(*args, budget="learner", **kw) == plan_cadence(*args, **kw)
    params = dict(total_timesteps=3_000_000, eval_freq=10_000)
    assert train_dqn.make_plan(params, 4096, 256, budget="learner") == train_dqn.make_plan(params, 4096, 256)


@pytest.mark.parametrize("driver", ["train_iqn", "train_dqn"])
def test_dry_run_prints_the_reference_plan_without_a_gpu(driver, tmp_path):
    cfg = tmp_path / "config.json"
    cfg.write_text(json.dumps(dict(agent="IQN" if driver == "train_iqn" else "DQN", seed=[0, 1], total_timesteps=3_000_000, eval_freq=10_000, save_dir=str(tmp_path / "out"))))
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", CUDA_VISIBLE_DEVICES="")      # no GPU, whatever the machine has
    run = lambda *extra: subprocess.run([sys.executable, "-m", f"distributional_rl_navigation_amd.{driver}", "-C", str(cfg), "--dry-run", "--env-budget", "reference", *extra],
                                        cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    r = run()
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
    assert [l["seed"] for l in lines] == [0, 1]
    for l in lines:
        assert l["n_envs"] == 80 and l["batch"] == 32 and l["replay"] == 1_000_000 and l["eval_deferred"] is True and l["episode_log"] is True
        want = plan_cadence(3_000_000, 10_000, 80, 32, budget="reference") if driver == "train_iqn" else \
            train_dqn.make_plan(dict(total_timesteps=3_000_000, eval_freq=10_000), 80, 32, budget="reference")
        assert l["plan"] == json.loads(json.dumps(want))
    assert not (tmp_path / "out").exists()
    # a contradicting explicit value is an error, not ignored
    for extra in (("--batch", "256"), ("--n-envs", "64"), ("--replay", "100000"), ("--grad-steps", "1")):
        r = run(*extra)
        assert r.returncode != 0 and "reference" in r.stderr, (extra, r.stderr[-500:])
