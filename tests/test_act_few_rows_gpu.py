"""The act launch of a SHORT list of greedy rows (csrc/iqn_act_few.h `sp::iqn_act_few_kernel`; C-ABI mn_iqn_set_few_rows_max, `ActContext.set_few_rows_max`): two
wavefronts per listed row that read the weight image from global memory instead of an LDS copy of it.  The kernel is forced on (threshold 2^31 - 1) or off
(-1) through the setter, and everything a call leaves -- actions, the draw buffer, the generator state -- is compared bit for bit with the listed form of
`iqn_qvals_split_kernel` and with the full kernel (`greedy_rows=False`).  `ActContext.few_rows_launches` says which kernel a call really took."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import rng_twin as T      # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ALWAYS, NEVER = 2 ** 31 - 1, -1


@pytest.fixture(scope="module")
def torch():
    import torch as t
    if not t.cuda.is_available():
        pytest.skip("no GPU")
    return t


def _net(seed=7):
    from distributional_rl_navigation_amd.iqn.model import ObsEncoder
    return ObsEncoder(26, 9, seed=seed, device=DEV)


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


def _act(torch, net, obs, eps, cvar, seed, ctr=0, few=None, grid=0):
    """One fused_act call from the generator state {seed, ctr}.  few = True / False: the listed rows through the few-rows kernel / the listed form;
    None: every row through the full kernel.  Returns (actions, a copy of the draw buffer, the state afterwards); asserts the kernel the call took."""
    from distributional_rl_navigation_amd.iqn.fused_act import act_context, fused_act
    ctx = act_context(net)
    ctx.set_few_rows_max(ALWAYS if few else NEVER)
    ctx.set_grid(grid)
    before = ctx.few_rows_launches()
    rng = _rng(torch, seed, ctr)
    try:
        a = fused_act(net, obs, eps, cvar, rng=rng, greedy_rows=few is not None)
    finally:
        ctx.set_few_rows_max(None)
        ctx.set_grid(0)
    assert ctx.few_rows_launches() - before == (1 if few else 0)
    return a, rng.draws(obs.shape[0], 32).clone(), rng.state.clone()


# n, eps, workgroup cap (0: one per CU): the smallest sizes; a list longer than the grid, so that a workgroup loops over positions (capped at 37 workgroups
# as well: eight or nine positions each whatever the chip); the headline regime, about four rows of 4 133; an empty list
CASES = [(1, 0.5, 0), (1, 1e-9, 0), (7, 0.5, 0), (7, 1e-9, 0), (300, 1e-9, 0), (300, 1e-9, 37), (4096 + 37, 0.999, 0), (4096 + 37, 1.0, 0)]


@pytest.mark.parametrize("n,eps,grid", CASES)
def test_equal_to_the_listed_form_and_the_full_kernel(torch, net, n, eps, grid):
    obs = _obs(torch, n)
    seed = 2000 + n
    a_few, d_few, s_few = _act(torch, net, obs, eps, 1.0, seed, few=True, grid=grid)
    a_lst, d_lst, s_lst = _act(torch, net, obs, eps, 1.0, seed, few=False, grid=grid)
    a_all, d_all, s_all = _act(torch, net, obs, eps, 1.0, seed, few=None)
    assert torch.equal(a_few, a_lst) and torch.equal(a_few, a_all)
    assert torch.equal(d_few, d_lst) and torch.equal(d_few, d_all)
    assert torch.equal(s_few, s_lst) and torch.equal(s_few, s_all) and s_few.tolist() == [seed, 1]
    want = T.act_draws(seed, 0, n, 1.0)
    assert np.array_equal(d_few.cpu().numpy().view(np.uint32), want.view(np.uint32))      # the taus of EVERY row, and the uniforms
    greedy = want[-n:] > np.float32(eps)
    if n == 300:
        assert greedy.sum() > torch.cuda.get_device_properties(0).multi_processor_count or grid      # longer than the grid
        assert greedy.sum() >= 290
    if eps == 0.999:
        assert 1 <= greedy.sum() <= 20
    if eps == 1.0:
        assert not greedy.any()
    a = a_few.cpu().numpy()
    assert np.array_equal(a[~greedy], T.explore_action(want[-n:][~greedy], eps, np.full(int((~greedy).sum()), -1)))      # exploring rows: the twin alone


def test_per_row_cvar(torch, net):
    n, eps = 513, 0.3
    obs = _obs(torch, n, seed=2)
    cv = torch.rand(n, device=DEV, generator=torch.Generator(device=DEV).manual_seed(9)) * 0.9 + 0.1
    a_few, d_few, s_few = _act(torch, net, obs, eps, cv, 31, 4, few=True)
    a_lst, d_lst, s_lst = _act(torch, net, obs, eps, cv, 31, 4, few=False)
    a_all, d_all, s_all = _act(torch, net, obs, eps, cv, 31, 4, few=None)
    assert torch.equal(a_few, a_lst) and torch.equal(a_few, a_all)
    assert torch.equal(d_few, d_lst) and torch.equal(d_few, d_all) and torch.equal(s_few, s_lst) and torch.equal(s_few, s_all)
    want = T.act_draws(31, 4, n, cv.cpu().numpy())
    assert np.array_equal(d_few.cpu().numpy().view(np.uint32), want.view(np.uint32))


def test_consecutive_calls_alternating_kernels_rearm_the_count(torch):
    """Five calls on one ActRng, the few-rows kernel and the listed form in turn, n alternating between 1 000 and 9 001 (the list grows on the second call):
    both kernels leave the count slots as the other expects them; every call's actions and the final state equal the full kernel's."""
    from distributional_rl_navigation_amd.iqn.fused_act import act_context, fused_act
    ns = (1000, 9001, 1000, 9001, 1000)
    obs = {n: _obs(torch, n, seed=n) for n in set(ns)}
    runs = []
    for mixed in (False, True):
        net = _net(seed=3)
        ctx = act_context(net)
        rng = _rng(torch, 77)
        acts = []
        for i, n in enumerate(ns):
            ctx.set_few_rows_max(ALWAYS if i % 2 == 0 else NEVER)
            acts.append(fused_act(net, obs[n], 0.5, 1.0, rng=rng, greedy_rows=mixed).clone())
        assert ctx.few_rows_launches() == (3 if mixed else 0)
        runs.append((acts, rng.state.clone()))
    for a, b in zip(runs[0][0], runs[1][0]):
        assert torch.equal(a, b)
    assert torch.equal(runs[0][1], runs[1][1]) and runs[1][1].tolist() == [77, 5]


def test_weight_change_between_two_calls(torch):
    """The second call finds a stale image, which its preparation launch packs: the few-rows kernel reads the new one -- its actions equal the listed
    form's, and those of a network that never had other weights."""
    from distributional_rl_navigation_amd.iqn.fused_act import act_context, fused_act
    n, eps = 64, 1e-9
    obs = _obs(torch, n, seed=5)

    def change(net):
        with torch.no_grad():
            net.output_layer.weight.copy_(net.output_layer.weight.flip(0))
            net.hidden_layer.bias.mul_(-1.5)

    second = []
    for few in (True, False):
        net = _net(seed=3)
        ctx = act_context(net)
        ctx.set_few_rows_max(ALWAYS if few else NEVER)
        rng = _rng(torch, 5)
        first = fused_act(net, obs, eps, 1.0, rng=rng).clone()
        change(net)
        second.append((first, fused_act(net, obs, eps, 1.0, rng=rng).clone()))
        assert ctx.few_rows_launches() == (2 if few else 0)
    fresh = _net(seed=3)
    change(fresh)
    a_fresh, _, _ = _act(torch, fresh, obs, eps, 1.0, 5, 1, few=False)
    assert torch.equal(second[0][0], second[1][0]) and torch.equal(second[0][1], second[1][1]) and torch.equal(second[0][1], a_fresh)
    assert not torch.equal(second[0][0], second[0][1])      # (the change moves actions: a stale image would show)


def _training_loop(torch, few, n=4096, steps=40, eps=0.999):
    """`steps` vector steps of IQNAgent.vec_step at eps with every reset owed to the next act call (its preparation launch runs it) and a gradient step every
    fourth step; the episode clocks staggered so that a fifth of the envs finishes at every step.  Everything the loop leaves, as host arrays."""
    from test_reset_in_prep_gpu import _everything
    from distributional_rl_navigation_amd import _capi
    from distributional_rl_navigation_amd.iqn.agent import IQNAgent
    from distributional_rl_navigation_amd.iqn.fused_act import act_context
    from distributional_rl_navigation_amd.marinenav_env.vec_env import VecMarineNavEnv
    env = VecMarineNavEnv(n, seed=3, device=DEV, precision="f64")
    env.params.max_episode_steps = 5
    env.set_attrs(num_cores=8, num_obs=10, min_start_goal_dis=40.0)
    agent = IQNAgent(26, 9, BATCH_SIZE=64, BUFFER_SIZE=3 * n, device=DEV, seed=11, learning_starts=0, UPDATE_EVERY=4)
    agent.reset_under_act = True
    env.set_reset_owed_max_rows(ALWAYS)
    ctx = act_context(agent.qnetwork_local)
    ctx.set_few_rows_max(ALWAYS if few else NEVER)
    acts, inner = [], agent.act_batch

    def recording(*a, **kw):
        out = inner(*a, **kw)
        acts.append(out.clone())
        return out
    agent.act_batch = recording
    obs = env.reset()
    env.set_state(episode_timesteps=np.arange(n) % 5)
    losses, owed = 0, 0
    for t in range(steps):
        obs, reward, done, info, loss = agent.vec_step(env, obs, eps)
        owed += int(_capi.lib().mn_reset_is_owed(env.h))
        losses += loss is not None
    env.join_reset()
    agent.check_learner()
    out = dict(actions=torch.stack(acts).cpu().numpy(), end=_everything(torch, env, agent, obs), losses=losses, owed=owed, few=ctx.few_rows_launches())
    env.close()
    return out


def test_training_loop_few_rows_on_against_off(torch):
    from test_reset_in_prep_gpu import _equal
    on = _training_loop(torch, True)
    off = _training_loop(torch, False)
    assert on["few"] == 40 and off["few"] == 0
    assert on["owed"] == 40 and on["losses"] >= 9 and on["losses"] == off["losses"]
    _equal(on["actions"], off["actions"], "actions")
    _equal(on["end"], off["end"], "end")      # env state of every kind, RNG rows, observations, the replay ring, the generator state, the parameters
