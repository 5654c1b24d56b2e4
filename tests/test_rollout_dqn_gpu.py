"""DQN evaluation episodes in one launch (C-ABI `mn_rollout_dqn`, csrc/mn_rollout_dqn.hip; `DQNPolicy.rollout`, `train_dqn.evaluate(one_launch=True)`).

Claim under test: the launch computes, bit for bit, what the per-step loop of (mn_dqn_act, mn_step) computes -- observations, rewards, done / info
codes, actions, Q-values, the final state -- and the evaluation built from its traces equals the loop's evaluation.  Every comparison is exact."""
import ctypes as C
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DEV = "cuda:0"
KEYS = ("obs", "reward", "done", "info", "action", "q")


@pytest.fixture(scope="module")
def torch():
    import torch as t
    if not t.cuda.is_available():
        pytest.skip("no GPU")
    return t


def _cfg():
    with open(os.path.join(G, "eval_config_seed3.json")) as f:
        return json.load(f)


class _Agent:      # what train_dqn.evaluate reads of a DQNAgent
    def __init__(self, policy):
        self.policy, self.device = policy, policy.device


def _shipped():
    from distributional_rl_navigation_amd.dqn import DQNPolicy
    return DQNPolicy.load(os.path.join(G, "pretrained_DQN_seed3", "q_net.npz"), device=DEV)


def _seeded(torch, seed):
    from distributional_rl_navigation_amd.dqn import DQNPolicy
    torch.manual_seed(seed)
    return DQNPolicy(device=DEV)


def _dicts_equal(a, b):
    assert sorted(a) == sorted(b) == ["actions", "energies", "rewards", "successes", "times"]
    for k in ("rewards", "successes", "times", "energies"):
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and a[k].tolist() == b[k].tolist(), k
    assert a["actions"] == b["actions"]


def _evaluate_both(policy, max_steps=1000):
    from distributional_rl_navigation_amd.marinenav_env.vec_env import VecMarineNavEnv
    from distributional_rl_navigation_amd.train_dqn import evaluate
    cfg = _cfg()
    out = []
    for one in (False, True):
        env = VecMarineNavEnv(len(cfg), device=DEV, precision="f64")
        out.append(evaluate(_Agent(policy), env, cfg, max_steps=max_steps, one_launch=one))
        env.close()
    _dicts_equal(out[0], out[1])
    return out[0]


def test_shipped_weights_evaluation_equals_loop(torch):
    ev = _evaluate_both(_shipped())
    assert len(ev["actions"]) == 30 and min(len(a) for a in ev["actions"]) >= 1
    assert ev["successes"].any()      # the shipped network reaches some goals: episodes of different lengths end inside the launch


def _bits(x):
    import torch as t
    return x.view(t.int32) if x.dtype == t.float32 else x


def _loop(torch, pol, env, T):
    """T x (mn_dqn_act with Q and actions, mn_step) on every row; the state after every step."""
    ref = {k: [] for k in KEYS}
    states = []
    for _ in range(T):
        q, a = pol._fused(env.obs.contiguous(), True, True)
        obs, r, d, i = env.step(a)
        for k, v in zip(KEYS, (obs, r, d, i, a, q)):
            ref[k].append(v.clone())
        states.append(env.get_state())
    return {k: torch.stack(v) for k, v in ref.items()}, states


def _live(torch, done):
    dn = done.bool()
    return ~(torch.cumsum(dn.int(), 0) - dn.int() > 0)      # [T][n]: steps up to and including each env's first done


@pytest.mark.parametrize("precision", ["f64", "mixed"])
@pytest.mark.parametrize("n", [1, 30, 37, 500])
def test_seeded_network_traces_equal_act_step_loop(torch, precision, n):
    from distributional_rl_navigation_amd.marinenav_env.vec_env import VecMarineNavEnv
    T = 150
    pol = _seeded(torch, 11)
    envs = []
    for _ in range(2):
        e = VecMarineNavEnv(n, seed=4, device=DEV, precision=precision)
        e.reset()
        envs.append(e)
    assert torch.equal(envs[0].obs, envs[1].obs)
    ref, states = _loop(torch, pol, envs[0], T)
    one = pol.rollout(envs[1], T, trace=KEYS)
    assert one is not None
    live = _live(torch, ref["done"])
    for k in KEYS:
        assert torch.equal(_bits(one[k])[live], _bits(ref[k])[live]), k
    dead = ~live
    assert (one["action"][dead] == -1).all() and (one["done"][dead] == 1).all() and (one["reward"][dead] == 0).all()
    assert torch.isnan(one["q"][dead]).all() and (one["obs"][dead] == 0).all()      # not written once an env has finished
    # terminal info code repeats; final observation and state: the terminal step's for a finished env, the last step's otherwise
    last = (live.int().sum(0) - 1)                       # [n] index of each env's last live step
    idx = torch.arange(n, device=DEV)
    assert torch.equal(one["info"][-1], ref["info"][last, idx])
    assert torch.equal(_bits(one["final_obs"]), _bits(ref["obs"][last, idx]))
    s1, ep1, tot1 = envs[1].get_state()
    last_h = last.cpu().numpy()
    for i in range(n):
        s0, ep0, tot0 = states[last_h[i]]
        assert s1[i].tobytes() == s0[i].tobytes() and ep1[i] == ep0[i] and tot1[i] == tot0[i], i
    if n == 500:
        assert 0 < int(live[-1].sum()) < n      # some episodes ended, some run past the launch
    for e in envs:
        e.close()


@pytest.mark.parametrize("precision", ["f64", "mixed"])
def test_two_launches_of_40_equal_one_of_80(torch, precision):
    from distributional_rl_navigation_amd.marinenav_env.vec_env import VecMarineNavEnv
    n = 500
    pol = _seeded(torch, 11)
    envs = []
    for _ in range(2):
        e = VecMarineNavEnv(n, seed=4, device=DEV, precision=precision)
        e.reset()
        envs.append(e)
    one = pol.rollout(envs[0], 80, trace=KEYS)
    h1 = {k: v.clone() for k, v in pol.rollout(envs[1], 40, trace=KEYS).items()}
    h2 = pol.rollout(envs[1], 40, trace=KEYS)
    live = _live(torch, one["done"])
    go_on = live[39] & ~one["done"][39].bool()      # envs the second launch continues
    assert 0 < int(go_on.sum())
    for k in KEYS:
        x, y = _bits(torch.cat([h1[k], h2[k]], 0)), _bits(one[k])
        assert torch.equal(x[:40][live[:40]], y[:40][live[:40]]), k
        assert torch.equal(x[40:][live[40:] & go_on], y[40:][live[40:] & go_on]), k
    assert torch.equal(_bits(envs[0].obs)[go_on], _bits(envs[1].obs)[go_on])
    s0, ep0, tot0 = envs[0].get_state()
    s1, ep1, tot1 = envs[1].get_state()
    m = go_on.cpu().numpy()
    assert s0[m].tobytes() == s1[m].tobytes() and (ep0[m] == ep1[m]).all() and (tot0[m] == tot1[m]).all()
    for e in envs:
        e.close()


def test_rollout_acts_on_changed_weights(torch):
    """An in-place write through PyTorch (version counters) and a write behind PyTorch's back + weights_changed() both reach the next launch."""
    from distributional_rl_navigation_amd.marinenav_env.vec_env import VecMarineNavEnv
    n, T = 37, 20
    pol = _seeded(torch, 5)

    def both():
        envs = []
        for _ in range(2):
            e = VecMarineNavEnv(n, seed=9, device=DEV, precision="f64")
            e.reset()
            envs.append(e)
        one = pol.rollout(envs[0], T, trace=("action", "q", "done"))
        fresh = _seeded(torch, 5)      # a policy whose image is built from scratch from the same weights
        fresh.load_state_dict(pol.state_dict())
        ref, _ = _loop(torch, fresh, envs[1], T)
        live = _live(torch, ref["done"])
        assert torch.equal(one["action"][live], ref["action"][live]) and torch.equal(_bits(one["q"])[live], _bits(ref["q"])[live])
        for e in envs:
            e.close()
        return one["q"][0].clone()

    q0 = both()
    with torch.no_grad():
        pol.q_net.q_net[4].bias.add_(torch.linspace(-1.0, 1.0, 9, device=DEV))      # bumps the version counter
    q1 = both()
    assert not torch.equal(q0, q1)
    w = pol.q_net.features_extractor.hidden_layer.weight
    v = w._version
    w.data.mul_(0.5)      # `.data` has its own version counter: a write behind the parameter's back, like a HIP kernel's
    assert w._version == v
    pol.weights_changed()
    q2 = both()
    assert not torch.equal(q1, q2)


def test_refusals_and_fallback(torch):
    from distributional_rl_navigation_amd import _capi
    from distributional_rl_navigation_amd.marinenav_env.vec_env import VecMarineNavEnv
    lib = _capi.lib()
    pol = _seeded(torch, 2)
    env = VecMarineNavEnv(64, seed=1, device=DEV, precision="f64")
    env.reset()
    st, _ = pol._image(env.device)
    s = env._stream()
    p = lambda t: C.c_void_p(t.data_ptr())

    def call(h=env.h, weights=st["ptrs"], image=p(st["image"]), n_steps=4, obs=p(env.obs)):
        return lib.mn_rollout_dqn(h, weights, image, 1, n_steps, obs, None, None, None, None, None, None, s)
    INVALID = -1      # MN_ERR_INVALID
    assert call(n_steps=0) == INVALID and call(n_steps=-3) == INVALID
    assert call(h=None) == INVALID and call(weights=None) == INVALID and call(image=None) == INVALID and call(obs=None) == INVALID
    holes = (C.c_void_p * 18)(*[st["ptrs"][i] for i in range(18)])
    holes[7] = None
    assert call(weights=holes) == INVALID
    assert call() == 0
    torch.cuda.synchronize()
    env.close()
    # a policy that does not act through the fused kernel has no one-launch form: rollout returns None, evaluate runs the loop
    shipped = _shipped()
    _evaluate_both(shipped, max_steps=200)
    shipped.use_fused_act = False
    env = VecMarineNavEnv(30, device=DEV, precision="f64")
    assert shipped.rollout(env, 10) is None
    env.close()
    _evaluate_both(shipped, max_steps=200)      # (one_launch=True ran the loop: both dicts equal)


def test_train_driver_eval_one_launch(torch, tmp_path):
    from distributional_rl_navigation_amd import train_dqn
    from distributional_rl_navigation_amd.dqn import DQNAgent
    from distributional_rl_navigation_amd.marinenav_env.vec_env import VecMarineNavEnv
    cfg = tmp_path / "config_DQN.json"
    cfg.write_text(json.dumps({"agent": "DQN", "seed": [1], "total_timesteps": 3_000_000, "eval_freq": 10_000, "save_dir": str(tmp_path / "runs")}))
    train_dqn.main(["-C", str(cfg), "--n-envs", "1024", "--total-grad-steps", "300", "--n-evals", "2", "--eval-one-launch"])
    (stamp,) = os.listdir(tmp_path / "runs")
    d = tmp_path / "runs" / stamp / "seed_1"
    for f in ("evaluations.npz", "latest_model.zip", "best_model.zip"):
        assert (d / f).exists(), f
    ev = np.load(d / "evaluations.npz", allow_pickle=True)
    assert ev["rewards"].shape == (2, 30) and ev["rewards"].dtype == np.float64 and ev["successes"].dtype == bool
    assert ev["actions"].dtype == object and len(ev["actions"][0]) == 30
    ag = DQNAgent(device=DEV, buffer_size=64, seed=9)
    ag.load(str(d / "latest_model.zip"))
    ec = _cfg()
    out = []
    for one in (False, True):
        env = VecMarineNavEnv(len(ec), device=DEV, precision="f64")
        out.append(train_dqn.evaluate(ag, env, ec, one_launch=one))
        env.close()
    _dicts_equal(out[0], out[1])
