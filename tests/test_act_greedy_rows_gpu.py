"""The act launch that runs the network only on the rows that do not explore (C-ABI mn_iqn_set_greedy_rows, `fused_act(greedy_rows=...)`,
`IQNAgent.act_greedy_rows_only`; csrc/iqn_act_common.h `draw_block<true>`, iqn_act_split.h `iqn_qvals_split_kernel<.., ROWS = true>`): the preparation
launch writes an exploring row's action and lists every other row, the act kernel deals the list out.  Two yardsticks, both bit for bit:
  * the same call with `want_qvals=True`, which evaluates every row in the full kernel (pinned by tests/test_rng_draws_gpu.py);
  * the numpy twin tests/rng_twin.py (`act_draws`, `explore_action`).
Then the things a list adds: its count re-armed from call to call and its buffer grown, a per-row cvar, late rows (resets under the act kernel)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import rng_twin as T      # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS = (1.0, 0.9997, 0.5, 0.05, 1e-9)


@pytest.fixture(scope="module")
def torch():
    import torch as t
    if not t.cuda.is_available():
        pytest.skip("no GPU")
    return t


def _net(seed=7):
    from distributional_rl_navigation_amd.iqn.model import ObsEncoder
    return ObsEncoder(26, 9, seed=seed, device=DEV)      # (seeded random weights)


@pytest.fixture(scope="module")
def net(torch):
    return _net()


def _obs(torch, n, seed=11):
    g = torch.Generator(device=DEV); g.manual_seed(seed)
    return (torch.randn(n, 26, device=DEV, generator=g) * 5.0).contiguous()


def _rng(torch, seed, ctr=0):
    from distributional_rl_navigation_amd.iqn.fused_act import ActRng
    rng = ActRng(0, DEV)
    rng.state.copy_(torch.tensor([seed, ctr], dtype=torch.int64, device=DEV))
    return rng


def _act(torch, net, obs, eps, cvar, seed, ctr=0, **kw):
    """One fused_act call from the generator state {seed, ctr}: (outputs, a copy of the call's draw buffer, the state afterwards)."""
    from distributional_rl_navigation_amd.iqn.fused_act import fused_act
    rng = _rng(torch, seed, ctr)
    out = fused_act(net, obs, eps, cvar, rng=rng, **kw)
    return out, rng.draws(obs.shape[0], 32).clone(), rng.state.clone()


def _sizes(torch):
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    return [1, 7, 4096 + 37, 2 * 8 * 64 * cus - 3]      # one row; one block's waves; 17 of 256 CUs' worth and an odd tail; two rounds of 64 rows per wavefront


@pytest.mark.parametrize("k", range(4))
def test_actions_equal_the_full_kernel_and_the_twin(torch, net, k):
    n = _sizes(torch)[k]
    obs = _obs(torch, n)
    seed = 1000 + k
    want = T.act_draws(seed, 0, n, 1.0)
    u = want[-n:]
    for eps in EPS:
        (a_ref, q), d_ref, s_ref = _act(torch, net, obs, eps, 1.0, seed, want_qvals=True)
        a_on, d_on, s_on = _act(torch, net, obs, eps, 1.0, seed, greedy_rows=True)
        a_off, d_off, s_off = _act(torch, net, obs, eps, 1.0, seed, greedy_rows=False)
        where = (n, eps)
        assert torch.equal(a_on, a_ref) and torch.equal(a_off, a_ref), where
        assert torch.equal(d_on, d_ref) and torch.equal(d_off, d_ref), where
        assert np.array_equal(d_on.cpu().numpy().view(np.uint32), want.view(np.uint32)), where      # taus of EVERY row, and the uniforms
        assert torch.equal(s_on, s_ref) and torch.equal(s_off, s_ref) and s_on.tolist() == [seed, 1], where
        a = a_on.cpu().numpy()
        greedy = u > np.float32(eps)
        with np.errstate(invalid="ignore"):      # (the twin forms u / eps x 9 for the greedy rows too and discards it: past int32 at eps = 1e-9)
            assert np.array_equal(a, T.explore_action(u, eps, q.cpu().numpy().argmax(1))), where
        assert np.array_equal(a[~greedy], T.explore_action(u[~greedy], eps, np.full(int((~greedy).sum()), -1))), where      # exploring rows: the twin alone
        if eps == 1.0:
            assert not greedy.any()                             # 24-bit uniforms in [0, 1): the list is empty
        if eps == 1e-9:
            assert np.array_equal(greedy, u != 0)               # ... and here it holds every row but those that drew exactly 0


def test_consecutive_calls_rearm_the_count_and_grow_the_buffer(torch):
    """Five calls on one ActRng, n alternating between two sizes (the second larger: the context's list grows on its first launch), on a network
    of its own (a fresh context).  The list's count is re-armed by the launches themselves: every call's actions and the final state equal those of
    the full kernel."""
    from distributional_rl_navigation_amd.iqn.fused_act import fused_act
    ns = (1000, 9001, 1000, 9001, 1000)
    obs = {n: _obs(torch, n, seed=n) for n in set(ns)}
    runs = []
    for kw in (dict(want_qvals=True), dict(greedy_rows=True), dict(greedy_rows=False)):
        net = _net(seed=3)
        rng = _rng(torch, 77)
        acts = []
        for n in ns:
            out = fused_act(net, obs[n], 0.5, 1.0, rng=rng, **kw)
            acts.append((out[0] if isinstance(out, tuple) else out).clone())
        runs.append((acts, rng.state.clone()))
    for acts, state in runs[1:]:
        for a, b in zip(acts, runs[0][0]):
            assert torch.equal(a, b)
        assert torch.equal(state, runs[0][1]) and state.tolist() == [77, 5]
    for i, n in enumerate(ns):      # (and the twin, so that the three cannot agree on something else)
        u = T.act_draws(77, i, n, 1.0)[-n:]
        a = runs[1][0][i].cpu().numpy()
        assert np.array_equal(a[u <= np.float32(0.5)], T.explore_action(u[u <= np.float32(0.5)], 0.5, np.zeros(int((u <= np.float32(0.5)).sum()))))


def test_per_row_cvar(torch, net):
    n, eps = 513, 0.3
    obs = _obs(torch, n, seed=2)
    cv = torch.rand(n, device=DEV, generator=torch.Generator(device=DEV).manual_seed(9)) * 0.9 + 0.1
    (a_ref, q), d_ref, s_ref = _act(torch, net, obs, eps, cv, 31, 4, want_qvals=True)
    a_on, d_on, s_on = _act(torch, net, obs, eps, cv, 31, 4, greedy_rows=True)
    a_off, d_off, s_off = _act(torch, net, obs, eps, cv, 31, 4, greedy_rows=False)
    assert torch.equal(a_on, a_ref) and torch.equal(a_off, a_ref)
    assert torch.equal(d_on, d_ref) and torch.equal(s_on, s_ref) and torch.equal(d_off, d_ref) and torch.equal(s_off, s_ref)
    want = T.act_draws(31, 4, n, cv.cpu().numpy())
    assert np.array_equal(d_on.cpu().numpy().view(np.uint32), want.view(np.uint32))
    assert np.array_equal(a_on.cpu().numpy(), T.explore_action(want[-n:], eps, q.cpu().numpy().argmax(1)))


def _loop(torch, under_act, greedy_rows, eps, n=8192, T_=10):
    """The shape of tests/test_reset_under_act_gpu.py `_loop` with every row late (max_episode_steps = 3), no training, and the actions recorded."""
    from distributional_rl_navigation_amd.iqn.agent import IQNAgent
    from distributional_rl_navigation_amd.iqn.fused_act import late_timeouts
    from distributional_rl_navigation_amd.marinenav_env.vec_env import VecMarineNavEnv
    env = VecMarineNavEnv(n, seed=3, device=DEV, precision="f64")
    env.params.max_episode_steps = 3
    env.set_attrs(num_cores=8, num_obs=10, min_start_goal_dis=40.0)
    agent = IQNAgent(26, 9, BATCH_SIZE=64, BUFFER_SIZE=3 * n, device=DEV, seed=11, learning_starts=0, UPDATE_EVERY=10 ** 9)
    agent.reset_under_act = under_act
    agent.act_greedy_rows_only = greedy_rows
    env.set_reset_under_act_max(2 ** 31 - 1)
    acts, inner = [], agent.act_batch

    def recording(*a, **kw):
        out = inner(*a, **kw)
        acts.append(out.clone())
        return out
    agent.act_batch = recording
    obs = env.reset()
    dones = 0
    for t in range(T_):
        obs, reward, done, info, loss = agent.vec_step(env, obs, eps)
        assert (env.late_rows is not None) == under_act
        dones += int(done.sum())
    env.join_reset()
    assert late_timeouts(agent.qnetwork_local) == 0
    out = dict(actions=torch.stack(acts), obs=obs.clone(), state=env.get_state(), dones=dones)
    env.close()
    return out


@pytest.mark.parametrize("eps", [0.5, 0.9997])
def test_every_row_late(torch, eps):
    """Resets under the act kernel == resets in front of it, with the listed rows; and both == the launch that evaluates every row.  An exploring
    late row is not in the list: nobody waits for its reset or reads its observation."""
    front = _loop(torch, False, True, eps)
    under = _loop(torch, True, True, eps)
    full = _loop(torch, True, False, eps)
    assert front["dones"] >= 2 * 8192
    for other in (under, full):
        assert torch.equal(front["actions"], other["actions"]) and torch.equal(front["obs"], other["obs"])
        for x, y in zip(front["state"], other["state"]):
            assert np.array_equal(x, y)


def _learn_vec_run(torch, under, greedy_rows=True, steps=40):
    from distributional_rl_navigation_amd.iqn.agent import IQNAgent
    from distributional_rl_navigation_amd.iqn.fused_act import late_timeouts
    from distributional_rl_navigation_amd.marinenav_env.vec_env import VecMarineNavEnv
    env = VecMarineNavEnv(4096, seed=2, device=DEV, precision="f64")
    env.params.max_episode_steps = 5
    env.set_attrs(num_cores=8, num_obs=10, min_start_goal_dis=40.0)
    agent = IQNAgent(26, 9, BATCH_SIZE=64, BUFFER_SIZE=3 * 4096, device=DEV, seed=5, learning_starts=0, UPDATE_EVERY=2)
    agent.act_greedy_rows_only = greedy_rows
    agent.learn_vec(total_vector_steps=steps, train_env=env, verbose=False, reset_under_act=under)
    out = dict(params=torch.cat([p.detach().reshape(-1).clone() for p in agent.qnetwork_local.parameters()]), obs=env.obs.clone(), state=env.get_state(),
               launches=list(env.reset_launches), fallback=agent.under_act_fallback, timeouts=late_timeouts(agent.qnetwork_local))
    env.close()
    return out


def test_training_loop_with_late_rows(torch):
    """4 096 envs, 40 vector steps of learn_vec with a gradient step every second one (as test_learn_vec_preflight_healthy_box): resets in front and
    under the act kernel, and the launch that evaluates every row, learn the same parameters from the same observations; no wait ran out."""
    front = _learn_vec_run(torch, False)
    under = _learn_vec_run(torch, True)
    full = _learn_vec_run(torch, True, greedy_rows=False)
    assert under["launches"][1] == 40 and front["launches"] == [0, 0]
    for r in (front, under, full):
        assert r["fallback"] is None and r["timeouts"] == 0
    for other in (under, full):
        assert torch.equal(front["params"], other["params"]) and torch.equal(front["obs"], other["obs"])
        for x, y in zip(front["state"], other["state"]):
            assert np.array_equal(x, y)
