"""IQN evaluation episodes in one launch (C-ABI `mn_rollout_iqn`, csrc/mn_rollout_iqn.hip; `IQNAgent.evaluation_vec(one_launch=True)`).

Claim under test: the launch computes, bit for bit, what the per-step loop of (mn_iqn_act_rng at eps = 0, mn_step) computes -- observations,
rewards, done / info codes, actions, Q-values, the adaptive cvar and the act call counter -- and the evaluation built from its traces equals
the loop's evaluation (returned dict, logged npz, ActRng state)."""
import ctypes as C
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DEV = "cuda:0"


@pytest.fixture(scope="module")
def torch():
    import torch as t
    if not t.cuda.is_available():
        pytest.skip("no GPU")
    return t


def _cfg():
    with open(os.path.join(G, "eval_config_seed3.json")) as f:
        return json.load(f)


def _pretrained_agent():
    from distributional_rl_navigation_amd.iqn.agent import IQNAgent
    agent = IQNAgent(26, 9, device=DEV, seed=3)
    agent.load_model(os.path.join(G, "pretrained_IQN_seed3"), DEV)
    return agent


def _npz_equal(a, b):
    za, zb = np.load(a, allow_pickle=True), np.load(b, allow_pickle=True)
    assert sorted(za.files) == sorted(zb.files)
    for k in za.files:
        x, y = za[k], zb[k]
        if x.dtype == object:
            assert x.shape == y.shape and all(list(u) == list(v) for u, v in zip(x.reshape(-1), y.reshape(-1))), k
        else:
            assert np.array_equal(x, y), k


def _evaluations_agree(greedy, tmp_path, prepare=None):
    from distributional_rl_navigation_amd.marinenav_env.vec_env import VecMarineNavEnv
    cfg = _cfg()
    agents, envs, dirs = [], [], []
    for i in range(2):
        a = _pretrained_agent()
        if prepare is not None:
            prepare(a)
        agents.append(a)
        envs.append(VecMarineNavEnv(len(cfg), seed=0, device=DEV, precision="f64"))
        d = tmp_path / f"run{i}"
        d.mkdir()
        dirs.append(str(d))
    for _ in range(2):      # the second evaluation continues from the act counter the first one left
        loop = agents[0].evaluation_vec(envs[0], cfg, greedy=greedy, eval_log_path=dirs[0])
        one = agents[1].evaluation_vec(envs[1], cfg, greedy=greedy, eval_log_path=dirs[1], one_launch=True)
        assert one == loop
        name = "greedy_evaluations.npz" if greedy else "adaptive_evaluations.npz"
        _npz_equal(os.path.join(dirs[0], name), os.path.join(dirs[1], name))
        r0, r1 = agents[0]._act_rng, agents[1]._act_rng
        assert r0 is not None and r1 is not None and r0.state.tolist() == r1.state.tolist()
    for e in envs:
        e.close()
    return agents


def test_pretrained_greedy_equals_loop(torch, tmp_path):
    _evaluations_agree(True, tmp_path)


def test_pretrained_adaptive_equals_loop_and_cvar_is_adjust_cvar(torch, tmp_path):
    _evaluations_agree(False, tmp_path)
    # the cvar each step's taus were drawn with = IQNAgent.adjust_cvar_batch of the row the step acted on, bitwise
    from distributional_rl_navigation_amd.iqn.fused_act import ActRng, rollout_iqn
    from distributional_rl_navigation_amd.marinenav_env.vec_env import VecMarineNavEnv
    cfg = _cfg()
    agent = _pretrained_agent()
    env = VecMarineNavEnv(len(cfg), seed=0, device=DEV, precision="f64")
    r0 = list(cfg.values())[0]["robot"]
    env.set_attrs(N=r0["N"], dt=r0["dt"])
    obs0 = env.load_worlds([VecMarineNavEnv.world_from_eval_config(c) for c in cfg.values()]).clone()
    tr = rollout_iqn(agent.qnetwork_local, env, 1000, ActRng(5, DEV), adaptive=True, trace=("obs", "done", "cvar"))
    T = tr["steps_run"]
    before = torch.cat([obs0[None], tr["obs"][:T - 1]], 0)
    alive = torch.ones(len(cfg), dtype=torch.bool, device=DEV)
    checked = 0
    for t in range(T):
        want = agent.adjust_cvar_batch(before[t])
        got = tr["cvar"][t]
        assert torch.equal(got[alive].view(torch.int32), want[alive].view(torch.int32)), t
        checked += int(alive.sum())
        alive &= ~tr["done"][t].bool()
    assert checked > 100
    env.close()


@pytest.mark.parametrize("precision", ["f64", "mixed"])
@pytest.mark.parametrize("cvar", [1.0, 0.25])
def test_seeded_network_traces_equal_act_step_loop(torch, precision, cvar):
    from distributional_rl_navigation_amd.iqn.fused_act import ActRng, fused_act, rollout_iqn
    from distributional_rl_navigation_amd.iqn.model import ObsEncoder
    from distributional_rl_navigation_amd.marinenav_env.vec_env import VecMarineNavEnv
    n, T = 1024, 300
    net = ObsEncoder(26, 9, seed=11, device=DEV)
    envs = []
    for _ in range(3):
        e = VecMarineNavEnv(n, seed=4, device=DEV, precision=precision)
        e.reset()
        envs.append(e)
    # the loop: mn_iqn_act_rng (+ Q) and mn_step, every step on every row
    rng_l = ActRng(77, DEV)
    ref = {k: [] for k in ("obs", "reward", "done", "info", "action", "q")}
    for t in range(T):
        a, q = fused_act(net, envs[0].obs.contiguous(), 0.0, cvar, rng=rng_l, want_qvals=True)
        obs, r, d, i = envs[0].step(a)
        for k, v in zip(("obs", "reward", "done", "info", "action", "q"), (obs, r, d, i, a, q)):
            ref[k].append(v.clone())
    ref = {k: torch.stack(v) for k, v in ref.items()}
    # one launch
    rng_1 = ActRng(77, DEV)
    one = rollout_iqn(net, envs[1], T, rng_1, cvar=cvar, trace=("obs", "reward", "done", "info", "action", "q", "cvar"))
    # two launches of 150
    rng_2 = ActRng(77, DEV)
    h1 = rollout_iqn(net, envs[2], T // 2, rng_2, cvar=cvar, trace=("obs", "reward", "done", "info", "action", "q"))
    h1 = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in h1.items()}
    h2 = rollout_iqn(net, envs[2], T // 2, rng_2, cvar=cvar, trace=("obs", "reward", "done", "info", "action", "q"))
    # live rows: steps up to and including each env's first done
    dn = ref["done"].bool()
    ended_before = torch.cumsum(dn.int(), 0) - dn.int() > 0      # [T][n]: the env finished at an earlier step
    live = ~ended_before
    for k in ("obs", "reward", "done", "info", "action", "q"):
        x, y = one[k], ref[k]
        if x.dtype == torch.float32:
            x, y = x.view(torch.int32), y.view(torch.int32)
        assert torch.equal(x[live], y[live]), k
    assert (one["action"][~live] == -1).all() and (one["done"][~live] == 1).all() and (one["reward"][~live] == 0).all()
    assert torch.equal(one["cvar"][live], torch.full_like(one["cvar"][live], cvar))
    steps = int(live.any(1).nonzero().max()) + 1
    assert one["steps_run"] == steps and int(rng_1.state[1]) == steps
    assert 0 < int(live[-1].sum()) < n      # some episodes ended, some run past the launch
    # two launches of 150 = one of 300 (envs still running after the first half; the second launch takes up every env's state)
    go_on = live[T // 2 - 1] & ~dn[T // 2 - 1]
    for k in ("obs", "reward", "done", "info", "action", "q"):
        x = torch.cat([h1[k], h2[k]], 0)
        y = one[k]
        if x.dtype == torch.float32:
            x, y = x.view(torch.int32), y.view(torch.int32)
        assert torch.equal(x[:T // 2][live[:T // 2]], y[:T // 2][live[:T // 2]]), k
        assert torch.equal(x[T // 2:][live[T // 2:] & go_on], y[T // 2:][live[T // 2:] & go_on]), k
    assert h1["steps_run"] == T // 2
    assert int(rng_2.state[1]) == T // 2 + h2["steps_run"]
    assert torch.equal(envs[1].obs[go_on & live[-1]], envs[2].obs[go_on & live[-1]])
    for e in envs:
        e.close()


def test_refusals_and_fallback(torch, tmp_path):
    from distributional_rl_navigation_amd import _capi
    from distributional_rl_navigation_amd.iqn.fused_act import ActRng, _p, act_context
    from distributional_rl_navigation_amd.iqn.model import ObsEncoder
    from distributional_rl_navigation_amd.marinenav_env.vec_env import VecMarineNavEnv
    lib = _capi.lib()
    net = ObsEncoder(26, 9, seed=2, device=DEV)
    env = VecMarineNavEnv(64, seed=1, device=DEV, precision="f64")
    env.reset()
    ctx = act_context(net)
    rng = ActRng(1, DEV)
    w = ctx.weights(net)
    s = env._stream()

    def call(h=env.h, c=ctx.h, weights=w, n_steps=4, state=rng.state, obs=env.obs):
        return lib.mn_rollout_iqn(h, c, weights, n_steps, _p(state) if state is not None else None, C.c_float(1.0), 0,
                                  _p(obs) if obs is not None else None, None, None, None, None, None, None, None, None, s)
    assert call(n_steps=0) != 0 and call(n_steps=-3) != 0
    assert call(h=None) != 0 and call(c=None) != 0 and call(weights=None) != 0 and call(state=None) != 0 and call(obs=None) != 0
    ctx.set_tau_mode(1)
    assert call() != 0
    ctx.set_tau_mode(0)
    ctx.set_variant(0)
    assert call() != 0
    ctx.set_variant(2)
    assert int(rng.state[1]) == 0
    assert call() == 0
    torch.cuda.synchronize()
    assert 1 <= int(rng.state[1]) <= 4
    env.close()
    # the agent falls back to the loop where the launch refuses: same results
    for sub, prep in (("shared", lambda a: setattr(a, "shared_taus", True)), ("exact", lambda a: act_context(a.qnetwork_local).set_variant(0))):
        (tmp_path / sub).mkdir()
        _evaluations_agree(True, tmp_path / sub, prepare=prep)


def test_train_driver_eval_one_launch(torch, tmp_path):
    """train_iqn.run_trial with eval_one_launch: the same evaluation files as without (first: two runs without the flag agree)."""
    from distributional_rl_navigation_amd import train_iqn
    runs = []
    for i, flag in enumerate((False, False, True)):
        params = dict(agent="IQN", seed=2, total_timesteps=20_000, eval_freq=10_000, save_dir=str(tmp_path / f"r{i}"), training_time="test")
        runs.append(train_iqn.run_trial("cuda:0", params, n_envs=1024, batch=64, replay=20_000, verbose=False, eval_one_launch=flag))
    names = ("greedy_evaluations.npz", "adaptive_evaluations.npz")

    def same(a, b):
        try:
            for nm in names:
                _npz_equal(os.path.join(a, nm), os.path.join(b, nm))
            return True
        except AssertionError:
            return False
    if same(runs[0], runs[1]):
        for nm in names:
            _npz_equal(os.path.join(runs[0], nm), os.path.join(runs[2], nm))
    else:      # training itself is not reproducible run to run: compare the evaluations of one saved network instead
        from distributional_rl_navigation_amd.iqn.agent import IQNAgent
        from distributional_rl_navigation_amd.marinenav_env.vec_env import VecMarineNavEnv
        cfg = _cfg()
        out = []
        for one in (False, True):
            a = IQNAgent(26, 9, device=DEV, seed=2)
            a.load_model(runs[2], DEV)
            env = VecMarineNavEnv(len(cfg), seed=0, device=DEV, precision="f64")
            out.append((a.evaluation_vec(env, cfg, greedy=True, one_launch=one), a.evaluation_vec(env, cfg, greedy=False, one_launch=one)))
            env.close()
        assert out[0] == out[1]
