"""The experiment sweep as four launches (`run_experiment(one_launch=True)`) and what it needs of the IQN episode launch: per-env cvar and adaptive
flag (C-ABI `mn_rollout_iqn_rows`, `rollout_iqn(cvar_rows=, adaptive_rows=)`).

Claim under test: the rows form with NULL rows is mn_rollout_iqn; with rows it computes, bit for bit, what the per-step loop's ONE act call on all
rows computes (taus keyed by the row index, cvar = adjust_cvar of the row where the flag is set); and the sweep's records equal the loop's."""
import ctypes as C
import os

import pytest

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DEV = "cuda:0"
RECORD_KEYS = ("success", "out_of_area", "time", "energy", "reward", "actions")


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
    return x.view(t.int32) if x.dtype == t.float32 else x


def _live(torch, done):
    dn = done.bool()
    return ~(torch.cumsum(dn.int(), 0) - dn.int() > 0)


def test_rows_form_with_null_rows_is_mn_rollout_iqn(torch):
    from distributional_rl_navigation_amd import _capi
    from distributional_rl_navigation_amd.iqn.fused_act import ActRng, _p, act_context
    from distributional_rl_navigation_amd.iqn.model import ObsEncoder
    from distributional_rl_navigation_amd.marinenav_env.vec_env import VecMarineNavEnv
    lib = _capi.lib()
    n, T = 96, 60
    net = ObsEncoder(26, 9, seed=11, device=DEV)
    ctx = act_context(net)
    ctx.set_tau_mode(0)
    out = []
    for rows in (False, True):
        env = VecMarineNavEnv(n, seed=4, device=DEV, precision="f64")
        env.reset()
        rng = ActRng(77, DEV)
        tr = dict(obs=torch.zeros(T, n, 26, device=DEV), reward=torch.empty(T, n, device=DEV), done=torch.empty(T, n, dtype=torch.uint8, device=DEV),
                  info=torch.empty(T, n, dtype=torch.uint8, device=DEV), action=torch.empty(T, n, dtype=torch.int32, device=DEV),
                  cvar=torch.full((T, n), float("nan"), device=DEV), q=torch.full((T, n, 9), float("nan"), device=DEV))
        steps = torch.zeros(1, dtype=torch.int32, device=DEV)
        head = (env.h, ctx.h, ctx.weights(net), T, _p(rng.state), C.c_float(0.5), 1)
        tail = (_p(env.obs), _p(tr["obs"]), _p(tr["reward"]), _p(tr["done"]), _p(tr["info"]), _p(tr["action"]), _p(tr["cvar"]), _p(tr["q"]), _p(steps),
                env._stream())
        rc = lib.mn_rollout_iqn_rows(*head, None, None, *tail) if rows else lib.mn_rollout_iqn(*head, *tail)
        assert rc == 0
        torch.cuda.synchronize()
        out.append((tr, int(steps), rng.state.tolist(), env.obs.clone()))
        env.close()
    (a, sa, ca, oa), (b, sb, cb, ob) = out
    assert sa == sb and ca == cb and ca[1] == sa and torch.equal(_bits(oa), _bits(ob))
    for k in a:
        x, y = _bits(a[k]), _bits(b[k])
        assert torch.equal(x, y), k      # (NaN fill compared as bits)


@pytest.mark.parametrize("precision", ["f64", "mixed"])
def test_mixed_rows_equal_one_act_call_per_step_loop(torch, precision):
    from distributional_rl_navigation_amd.iqn.fused_act import ActRng, fused_act, rollout_iqn
    from distributional_rl_navigation_amd.marinenav_env.vec_env import VecMarineNavEnv
    agent = _agent()
    net = agent.qnetwork_local
    n, T = 250, 120
    envs = []
    for _ in range(2):
        e = VecMarineNavEnv(n, seed=6, device=DEV, precision=precision)
        e.reset()
        envs.append(e)
    gen = torch.Generator().manual_seed(3)
    fixed = torch.tensor([0.25, 0.5, 0.75, 1.0])[torch.randint(0, 4, (n,), generator=gen)].to(DEV)
    adaptive = (torch.rand(n, generator=gen) < 0.4).to(DEV)
    assert 0 < int(adaptive.sum()) < n
    # the loop: what run_experiment does per step for its IQN rows -- agent.act_batch's launch (here with Q), env.step
    rng_l = ActRng(77, DEV)
    ref = {k: [] for k in ("done", "action", "cvar", "q")}
    for _ in range(T):
        obs = envs[0].obs.contiguous()
        cv = torch.where(adaptive, agent.adjust_cvar_batch(obs), fixed)
        a, q = fused_act(net, obs, 0.0, cv, rng=rng_l, want_qvals=True, shared_taus=agent.shared_taus)
        _, _, d, _ = envs[0].step(a)
        for k, v in zip(("done", "action", "cvar", "q"), (d, a, cv, q)):
            ref[k].append(v.clone())
    ref = {k: torch.stack(v) for k, v in ref.items()}
    rng_1 = ActRng(77, DEV)
    one = rollout_iqn(net, envs[1], T, rng_1, cvar_rows=fixed, adaptive_rows=adaptive, trace=("done", "action", "cvar", "q"))
    assert one is not None
    live = _live(torch, ref["done"])
    for k in ("done", "action", "cvar", "q"):
        assert torch.equal(_bits(one[k])[live], _bits(ref[k])[live]), k
    assert torch.equal(one["cvar"][0][~adaptive], fixed[~adaptive])
    steps = int(live.any(1).nonzero().max()) + 1
    assert one["steps_run"] == steps and int(rng_1.state[1]) == steps
    for e in envs:
        e.close()


def _sweep_both(policies, num, with_agent=True, with_dqn=True, prepare=None):
    from distributional_rl_navigation_amd.experiments import run_experiment
    out, agents = [], []
    for one in (False, True):
        agent = _agent() if with_agent else None
        if prepare is not None:
            prepare(agent)
        res, _ = run_experiment(agent, 6, 4, num=num, policies=policies, dqn=_dqn() if with_dqn else None, one_launch=one)
        out.append(res)
        agents.append(agent)
    loop, one = out
    assert list(one) == list(loop) == list(policies)
    for name in policies:
        for k in RECORD_KEYS:
            assert one[name][k] == loop[name][k], (name, k)
        assert len(one[name]["success"]) == num
        assert len(one[name]["computation_times"]) == sum(len(a) for a in one[name]["actions"]), name
        assert all(t > 0 for t in one[name]["computation_times"])
    return loop, one, agents


def test_sweep_all_policies_equals_loop(torch):
    from distributional_rl_navigation_amd.experiments import ALL_POLICIES
    loop, one, agents = _sweep_both(ALL_POLICIES, 24)
    # the documented difference: the act-call counter ends at + the longest IQN episode (loop: + the longest episode of any policy in the loop)
    iqn = [p for p in ALL_POLICIES if "IQN" in p]
    assert int(agents[1]._act_rng.state[1]) == max(len(a) for p in iqn for a in one[p]["actions"])
    assert int(agents[0]._act_rng.state[1]) == max(len(a) for p in iqn + ["DQN"] for a in loop[p]["actions"])
    assert any(one["DQN"]["success"]) and any(one["IQN_1.0"]["success"])


def test_sweep_dqn_only_without_agent(torch):
    _sweep_both(("DQN",), 24, with_agent=False)


def test_sweep_iqn_subset_in_other_order(torch):
    _sweep_both(("IQN_0.5", "adaptive_IQN", "IQN_1.0"), 24, with_dqn=False)


def test_sweep_falls_back_where_the_library_refuses(torch):
    """An agent on the exact-f32 act variant has no one-launch form: its policies run in the loop (DQN / APF / BA still as launches); a DQN policy
    that does not act through the fused kernel likewise."""
    from distributional_rl_navigation_amd.experiments import ALL_POLICIES, run_experiment
    from distributional_rl_navigation_amd.iqn.fused_act import act_context
    _sweep_both(ALL_POLICIES, 12, prepare=lambda a: act_context(a.qnetwork_local).set_variant(0))
    out = []
    for one in (False, True):
        pol = _dqn()
        pol.use_fused_act = False
        out.append(run_experiment(None, 6, 4, num=12, policies=("DQN", "APF"), dqn=pol, one_launch=one)[0])
    for name in ("DQN", "APF"):
        for k in RECORD_KEYS:
            assert out[0][name][k] == out[1][name][k], (name, k)
