"""Captured experiment episodes from the episode launches: the sub-step trajectory trace of mn_rollout_policy / mn_rollout_iqn_rows / mn_rollout_dqn
(C-ABI `mn_set_trajectory_trace`), the IQN episode launch that acts as act_eval does and records the quantile values and taus it chose from (C-ABI
`mn_rollout_iqn_eval`, `rollout_iqn(want_quantiles=True)`), and `run_experiment(capture=True, one_launch=True)`.

Claim under test: every launch records, bit for bit, what the per-step loop collects -- (mn_iqn_act_rng with quantiles_dev, mn_step with
mn_enable_trajectory, mn_get_trajectory) per step --; attaching the trajectory trace changes no other output; and the captured sweep built from the
launches' traces equals the captured sweep of the loop, `ep_data` included.  Every comparison is bitwise (floats viewed as integers)."""
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DEV = "cuda:0"
N_ENVS, T_STEPS = 96, 60


@pytest.fixture(scope="module")
def torch():
    import torch as t
    if not t.cuda.is_available():
        pytest.skip("no GPU")
    return t


def _agent(seed=2):
    from distributional_rl_navigation_amd.iqn.agent import IQNAgent
    agent = IQNAgent(26, 9, device=DEV, seed=seed, BUFFER_SIZE=1024)
    agent.load_model(os.path.join(G, "pretrained_IQN_seed3"), DEV)
    return agent


def _dqn():
    from distributional_rl_navigation_amd.dqn import DQNPolicy
    return DQNPolicy.load(os.path.join(G, "pretrained_DQN_seed3", "q_net.npz"), device=DEV)


def _bits(x):
    import torch as t
    return x.view(t.int32) if x.dtype == t.float32 else x.view(t.int64) if x.dtype == t.float64 else x


def _live(torch, done):
    """[T][n]: the steps up to and including each env's first done."""
    dn = done.bool()
    return ~(torch.cumsum(dn.int(), 0) - dn.int() > 0)


def _envs(k, precision="f64", seed=4, N=5):
    from distributional_rl_navigation_amd.marinenav_env.vec_env import VecMarineNavEnv
    out = []
    for _ in range(k):
        e = VecMarineNavEnv(N_ENVS, seed=seed, device=DEV, precision=precision)
        e.set_attrs(N=N)
        e.reset()
        out.append(e)
    return out


def _loop(torch, env, act, keys):
    """T_STEPS x (act, step with the trajectory recorded, get_trajectory), every step on every row: the stacked per-step results.  `obs`: the observations
    each step returns -- without reset_done, a finished env's row at its terminal step is its terminal observation."""
    env.enable_trajectory()
    ref = {k: [] for k in keys + ("reward", "done", "info", "action", "traj", "obs")}
    for _ in range(T_STEPS):
        got = act(env.obs.contiguous())
        _, r, d, i = env.step(got["action"])
        got.update(reward=r, done=d, info=i, traj=torch.from_numpy(env.get_trajectory()).to(DEV), obs=env.obs)
        for k in ref:
            ref[k].append(got[k].clone())
    return {k: torch.stack(v) for k, v in ref.items()}


def _compare(torch, one, ref, keys, filled):
    """`one` (a launch's traces) against `ref` (the loop's) on every live entry; the entries the launch never writes still hold their fill; the final
    observation of EVERY env is what the loop's step returned at the env's last live step: the terminal observation where the episode ended."""
    live = _live(torch, ref["done"])
    assert 0 < int(live[-1].sum()) < N_ENVS      # some episodes ended, some run past the launch
    for k in keys:
        assert one[k].shape == ref[k].shape and one[k].dtype == ref[k].dtype, k
        assert torch.equal(_bits(one[k])[live], _bits(ref[k])[live]), k
    for k in filled:
        assert bool(torch.isnan(one[k][~live]).all()), k
    assert (one["action"][~live] == -1).all() and (one["done"][~live] == 1).all() and (one["reward"][~live] == 0).all()
    last = live.sum(0) - 1
    assert torch.equal(_bits(one["final_obs"]), _bits(ref["obs"][last, torch.arange(N_ENVS, device=last.device)]))
    return live


def _same_but(torch, a, b, skip):
    """Two launches' results, equal in everything but the traces `skip` (NaN fills compared as bits)."""
    assert set(a) - set(skip) == set(b) - set(skip)
    for k in set(a) - set(skip):
        if torch.is_tensor(a[k]):
            assert torch.equal(_bits(a[k]), _bits(b[k])), k
        else:
            assert a[k] == b[k], k


@pytest.mark.parametrize("network", ["random", "shipped"])
def test_iqn_eval_launch_equals_act_eval_step_loop(torch, network):
    from distributional_rl_navigation_amd.iqn.agent import IQNAgent
    from distributional_rl_navigation_amd.iqn.fused_act import ActRng, fused_act, rollout_iqn
    from distributional_rl_navigation_amd.iqn.model import ObsEncoder
    agent = _agent()
    net = ObsEncoder(26, 9, seed=11, device=DEV) if network == "random" else agent.qnetwork_local
    net.eval()
    envs = _envs(3)
    # per-row cvar and adaptive flag, all five settings of the sweep side by side
    gen = torch.Generator().manual_seed(3)
    setting = torch.randint(0, 5, (N_ENVS,), generator=gen)
    assert len(set(setting.tolist())) == 5
    fixed = torch.tensor([1.0, 0.25, 0.5, 0.75, 1.0])[setting].to(DEV)
    adaptive = (setting == 0).to(DEV)
    rng_l = ActRng(77, DEV)

    def act(obs):
        cv = torch.where(adaptive, agent.adjust_cvar_batch(obs), fixed)
        a, quant, taus, q = fused_act(net, obs, 0.0, cv, rng=rng_l, want_quantiles=True, want_qvals=True)
        return dict(action=a, cvar=cv, q=q, quantiles=quant, taus=taus[:, :, 0])
    ref = _loop(torch, envs[0], act, ("cvar", "q", "quantiles", "taus"))
    keys = ("reward", "done", "info", "action", "cvar", "q", "quantiles", "taus", "traj")
    rng_1 = ActRng(77, DEV)
    one = rollout_iqn(net, envs[1], T_STEPS, rng_1, cvar_rows=fixed, adaptive_rows=adaptive, want_quantiles=True,
                      trace=("reward", "done", "info", "action", "cvar", "q", "traj"))
    assert one is not None and one["quantiles"].shape == (T_STEPS, N_ENVS, 32, 9) and one["taus"].shape == (T_STEPS, N_ENVS, 32)
    live = _compare(torch, one, ref, keys, ("cvar", "q", "quantiles", "taus", "traj"))
    # Q is the mean of the recorded quantile values and the action its first maximum
    assert torch.equal(one["q"][live].argmax(1).int(), one["action"][live])
    steps = int(live.any(1).nonzero().max()) + 1
    assert one["steps_run"] == steps and int(rng_1.state[1]) == steps == int(rng_l.state[1])
    # the same launch without the trajectory trace: everything else unchanged
    rng_2 = ActRng(77, DEV)
    bare = rollout_iqn(net, envs[2], T_STEPS, rng_2, cvar_rows=fixed, adaptive_rows=adaptive, want_quantiles=True,
                       trace=("reward", "done", "info", "action", "cvar", "q"))
    _same_but(torch, one, bare, ("traj",))
    assert rng_1.state.tolist() == rng_2.state.tolist()
    for e in envs:
        e.close()


def test_iqn_acting_launch_trajectory_trace(torch):
    """mn_rollout_iqn_rows (the acting form) with the trajectory trace: the loop's positions, nothing else changed."""
    from distributional_rl_navigation_amd.iqn.fused_act import ActRng, fused_act, rollout_iqn
    net = _agent().qnetwork_local
    net.eval()
    envs = _envs(3)
    rng_l = ActRng(5, DEV)
    ref = _loop(torch, envs[0], lambda obs: dict(action=fused_act(net, obs, 0.0, 0.75, rng=rng_l)), ())
    one = rollout_iqn(net, envs[1], T_STEPS, ActRng(5, DEV), cvar=0.75, trace=("reward", "done", "info", "action", "q", "traj"))
    bare = rollout_iqn(net, envs[2], T_STEPS, ActRng(5, DEV), cvar=0.75, trace=("reward", "done", "info", "action", "q"))
    _compare(torch, one, ref, ("reward", "done", "info", "action", "traj"), ("traj", "q"))
    _same_but(torch, one, bare, ("traj",))
    for e in envs:
        e.close()


@pytest.mark.parametrize("policy", ["APF", "BA", "DQN"])
def test_trajectory_trace_of_planner_and_dqn_launches(torch, policy):
    from distributional_rl_navigation_amd.planners import planner_act_batch
    envs = _envs(3)
    dqn = _dqn()
    p = envs[0].params
    if policy == "DQN":
        act = lambda obs: dict(action=dqn.act_batch(obs))
        launch = lambda env, trace: dqn.rollout(env, T_STEPS, trace=trace)
    else:
        act = lambda obs: dict(action=planner_act_batch(obs, policy, p.a[:], p.w[:]))
        launch = lambda env, trace: env.rollout_policy(T_STEPS, policy, trace=trace)
    ref = _loop(torch, envs[0], act, ())
    one = launch(envs[1], ("reward", "done", "info", "action", "traj"))
    bare = launch(envs[2], ("reward", "done", "info", "action"))
    assert one is not None and one["traj"].shape == (T_STEPS, N_ENVS, 5, 2) and one["traj"].dtype == torch.float64
    _compare(torch, one, ref, ("reward", "done", "info", "action", "traj"), ("traj",))
    _same_but(torch, one, bare, ("traj",))
    # the attachment was consumed: the next launch records nothing into the old buffer
    before = one["traj"].clone()
    launch(envs[1], ("reward", "done", "info", "action"))
    torch.cuda.synchronize()
    assert torch.equal(_bits(one["traj"]), _bits(before))
    for e in envs:
        e.close()


def test_mixed_precision_handle_refuses_the_trajectory_trace(torch):
    from distributional_rl_navigation_amd import _capi
    from distributional_rl_navigation_amd.iqn.fused_act import ActRng, rollout_iqn
    env = _envs(1, precision="mixed")[0]
    buf = torch.zeros(4, N_ENVS, 5, 2, dtype=torch.float64, device=DEV)
    rc = _capi.lib().mn_set_trajectory_trace(env.h, buf.data_ptr(), 4, 5)
    assert rc == -1 and b"MN_PRECISION_F64" in _capi.lib().mn_last_error(env.h)
    with pytest.raises(_capi.MarineNavHipError):
        env.rollout_policy(4, "APF", trace=("done", "traj"))
    with pytest.raises(_capi.MarineNavHipError):
        rollout_iqn(_agent().qnetwork_local, env, 4, ActRng(1, DEV), trace=("done", "traj"))
    # the launches themselves still run on it, and a float64 handle refuses a trace sized for another N or a shorter one than the launch
    assert env.rollout_policy(4, "APF") is not None
    env.close()
    env = _envs(1)[0]
    assert _capi.lib().mn_set_trajectory_trace(env.h, buf.data_ptr(), 4, 7) == -1
    assert _capi.lib().mn_set_trajectory_trace(env.h, buf.data_ptr(), 4, 5) == 0
    with pytest.raises(_capi.MarineNavHipError):
        env.rollout(8, trace=("done",))                              # mn_rollout records none and says so
    assert _capi.lib().mn_rollout_policy(env.h, 8, 1, env.obs.data_ptr(), None, None, None, None, None, env._stream()) == -1      # 8 steps > 4
    assert env.rollout_policy(8, "APF") is not None                # ... and the refused launch detached it
    torch.cuda.synchronize()
    assert bool((buf == 0).all())
    env.close()


def _capture_sweep(policies, n_obs, n_cores, num, one_launch, prepare=None):
    from distributional_rl_navigation_amd.experiments import run_experiment
    agent = _agent()
    if prepare is not None:
        prepare(agent)
    res, _ = run_experiment(agent, n_obs, n_cores, num=num, policies=policies, dqn=_dqn(), capture=True, one_launch=one_launch)
    return res


def _records_equal(loop, one, policies):
    assert list(one) == list(loop) == list(policies)
    for name in policies:
        assert set(one[name]) == set(loop[name]) and "ep_data" in one[name], name
        for k in one[name]:
            if k == "computation_times":      # built differently by design: checked as test_experiment_capture_schema does
                for r in (one, loop):
                    ct = r[name][k]
                    assert len(ct) == sum(len(a) for a in r[name]["actions"]) and all(0.0 < v < 1.0 for v in ct), name
                continue
            assert one[name][k] == loop[name][k], (name, k)
        assert json.dumps(one[name]["ep_data"]) == json.dumps(loop[name]["ep_data"]), name
        for i, ep in enumerate(one[name]["ep_data"]):
            L = len(one[name]["actions"][i])
            assert ep["robot"]["action_history"] == one[name]["actions"][i] and len(ep["robot"]["trajectory"]) == 5 * L
            iqn_keys = {"actions_cvars", "actions_quantiles", "actions_taus"} & set(ep["robot"])
            assert len(iqn_keys) == (3 if "IQN" in name else 0), name
            if iqn_keys:
                assert np.array(ep["robot"]["actions_quantiles"]).shape == (L, 1, 32, 9) and np.array(ep["robot"]["actions_taus"]).shape == (L, 1, 32, 1)


@pytest.mark.parametrize("n_obs,n_cores", [(10, 8), (6, 4)])
def test_captured_sweep_from_four_launches_equals_the_loop(torch, monkeypatch, n_obs, n_cores):
    from distributional_rl_navigation_amd import experiments
    from distributional_rl_navigation_amd.experiments import ALL_POLICIES
    loop = _capture_sweep(ALL_POLICIES, n_obs, n_cores, 6, False)

    def no_loop(*a, **k):
        raise AssertionError("the per-step loop was entered")
    monkeypatch.setattr(experiments, "loop_episodes", no_loop)
    one = _capture_sweep(ALL_POLICIES, n_obs, n_cores, 6, True)
    monkeypatch.undo()
    _records_equal(loop, one, ALL_POLICIES)


def test_captured_sweep_falls_back_to_the_loop_on_the_exact_variant(torch):
    """An agent on the exact-f32 act variant has no one-launch form: with capture=True, one_launch=True its policies run in the loop (the others as
    launches), with equal results."""
    from distributional_rl_navigation_amd.iqn.fused_act import act_context
    policies = ("adaptive_IQN", "IQN_0.5", "DQN", "APF")
    exact = lambda a: act_context(a.qnetwork_local).set_variant(0)
    loop = _capture_sweep(policies, 6, 4, 6, False, prepare=exact)
    one = _capture_sweep(policies, 6, 4, 6, True, prepare=exact)
    _records_equal(loop, one, policies)
