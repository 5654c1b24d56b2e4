"""`--env-budget reference` at toy size through both drivers' `run_trial`: the reference's cadence (one batch-32 gradient step per 4 env steps for
IQN, per env step for DQN, from learning_starts on), its evaluation timesteps, the training-episode log beside it, and run-to-run determinism."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOTAL, EVAL_FREQ, N = 4_000, 400, 16
REFERENCE = dict(learning_starts=400, target_update_interval=400)
POINTS = list(range(400, 4_001, 400))


@pytest.fixture(scope="module")
def torch():
    import torch as t
    if not t.cuda.is_available():
        pytest.skip("no GPU")
    return t


@pytest.fixture(scope="module")
def eval_config(torch):
    from distributional_rl_navigation_amd.train_iqn import create_eval_configs
    cfg = create_eval_configs(DEV)
    return {k: cfg[k] for k in list(cfg)[:3]}      # three evaluation worlds


def params(tmp, name, agent="IQN"):
    return dict(agent=agent, seed=3, total_timesteps=TOTAL, eval_freq=EVAL_FREQ, save_dir=str(tmp), training_time=name)


class DoneCounter:
    """`on_step` hook: the run's `done` flags summed on the device, read once at the end; the exploration rate of the last step."""

    def __init__(self, torch):
        self.total, self.eps, self.steps = torch.zeros((), dtype=torch.int64, device=DEV), None, 0

    def __call__(self, it, stats):
        self.total += (stats["last"]["done"] != 0).sum()
        self.eps, self.steps = stats["last"]["eps"], self.steps + 1


@pytest.fixture(scope="module")
def iqn_runs(torch, eval_config, tmp_path_factory):
    """The toy reference-budget IQN trial, twice with the same seed."""
    from distributional_rl_navigation_amd.train_iqn import run_trial
    tmp = tmp_path_factory.mktemp("reference_budget")
    out = []
    for name in ("a", "b"):
        counter = DoneCounter(torch)
        d, agent = run_trial(DEV, params(tmp, name), N, verbose=False, env_budget="reference", reference=REFERENCE, eval_config=eval_config, max_eval_steps=60,
                             episode_log="full", eval_deferred=dict(verbose=False), on_step=counter, return_agent=True)
        flat = torch.cat([p.detach().reshape(-1) for p in agent.qnetwork_local.parameters()]).cpu().numpy()
        out.append(dict(dir=d, grad_steps=agent.grad_steps, ring=len(agent.memory), params=flat, dones=int(counter.total.cpu()), eps=counter.eps, steps=counter.steps))
    return out


def test_batch_32_takes_the_one_launch_gradient_step(torch):
    from distributional_rl_navigation_amd import _capi
    torch.zeros(1, device=DEV)
    MN_TRAIN_ONE_LAUNCH = 4      # include/marinenav_hip.h
    assert _capi.lib().mn_iqn_train_plan(32, MN_TRAIN_ONE_LAUNCH, 0) == 1


def test_iqn_cadence_ring_and_exploration(iqn_runs):
    r = iqn_runs[0]
    assert r["steps"] == TOTAL // N
    assert r["grad_steps"] == 900          # (4 000 - 400) / 4
    assert r["ring"] == 4_000              # every env step of the run, nothing evicted from the reference's 1 M-row ring
    assert r["eps"] == 0.05


def test_iqn_evaluation_timesteps_are_the_reference_points(iqn_runs):
    d = iqn_runs[0]["dir"]
    greedy = np.load(os.path.join(d, "greedy_evaluations.npz"), allow_pickle=True)
    adaptive = np.load(os.path.join(d, "adaptive_evaluations.npz"), allow_pickle=True)
    assert greedy["timesteps"].tolist() == POINTS and adaptive["timesteps"].tolist() == POINTS
    assert greedy["rewards"].shape == (10, 3)


def test_iqn_training_log(iqn_runs):
    r = iqn_runs[0]
    log = np.load(os.path.join(r["dir"], "training_log.npz"))
    assert log["timesteps"].tolist() == POINTS and len(log["episodes"]) == 10
    assert r["dones"] > 0 and int(log["episodes"].sum()) == r["dones"]
    assert int(log["info_counts"].sum()) == r["dones"]
    eps = np.load(os.path.join(r["dir"], "training_episodes.npz"))
    assert len(eps["step"]) == r["dones"] and np.all(np.diff(eps["step"]) >= 0) and eps["step"].max() < TOTAL // N and eps["env"].max() < N


def test_iqn_second_run_is_bit_equal(iqn_runs):
    a, b = iqn_runs
    assert np.array_equal(a["params"].view(np.int32), b["params"].view(np.int32))
    ea, eb = (np.load(os.path.join(r["dir"], "training_episodes.npz")) for r in (a, b))
    assert set(ea.files) == set(eb.files) and len(ea["step"]) > 0
    for k in ea.files:
        assert ea[k].tobytes() == eb[k].tobytes(), k


def test_dqn_driver_at_the_same_toy_size(torch, eval_config, tmp_path):
    from distributional_rl_navigation_amd.train_dqn import run_trial
    counter = DoneCounter(torch)
    d, agent = run_trial(DEV, params(tmp_path, "dqn", "DQN"), N, verbose=False, env_budget="reference", reference=REFERENCE, eval_config=eval_config, max_eval_steps=60,
                         on_step=counter, return_agent=True)
    assert agent.n_updates == 3_600          # 4 000 - 400: one batch-32 step per env step from learning_starts on
    assert len(agent.memory) == 4_000 and counter.eps == 0.05
    assert np.load(os.path.join(d, "evaluations.npz"), allow_pickle=True)["timesteps"].tolist() == POINTS
    log = np.load(os.path.join(d, "training_log.npz"))
    assert log["timesteps"].tolist() == POINTS and int(log["episodes"].sum()) == int(counter.total.cpu()) > 0
    assert not os.path.exists(os.path.join(d, "training_episodes.npz"))      # (only with "full")


def test_learner_budget_without_the_flag_writes_no_training_log(torch, eval_config, tmp_path):
    from distributional_rl_navigation_amd.train_iqn import run_trial
    d = run_trial(DEV, params(tmp_path, "learner"), N, verbose=False, batch=32, total_grad_steps=200, eval_config=eval_config, max_eval_steps=60,
                  eval_deferred=dict(verbose=False))
    assert os.path.exists(os.path.join(d, "greedy_evaluations.npz"))
    assert not os.path.exists(os.path.join(d, "training_log.npz")) and not os.path.exists(os.path.join(d, "training_episodes.npz"))
