"""The exploring DQN act launch (C-ABI mn_dqn_act_rng, csrc/dqn_collect.hip) and `DQNAgent(fused_collect=True)`: the actions against the host twin
(tests/dqn_rng_twin.py) given mn_dqn_act's greedy actions, the uniforms against the twin, the Q-values against mn_dqn_act's -- all bit for bit --, the weight
image's repack switch, the argument checks, and the agent's collect through `step_append` against `step` + `add_vector_step`."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import dqn_rng_twin as D      # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "pretrained_DQN_seed3", "q_net.npz")
SENT = 0x7FC0DEAD    # (a NaN with a payload, as float)
PAD = 8              # rows behind the n of a call in every output buffer
INVALID = -1         # MN_ERR_INVALID
SEED = 0xC0FFEE12345
NS = (1, 15, 16, 17, 129, 2051)      # below, at and above one tile; more than one workgroup of 8 tiles (2 051 rows: 129 tiles, 17 workgroups)
EPS = (0.0, 0.05, 0.5, 1.0)
CALLS = (0, 1, 2 ** 32 + 5)


@pytest.fixture(scope="module")
def torch():
    import torch as t
    if not t.cuda.is_available():
        pytest.skip("no GPU")
    return t


@pytest.fixture(scope="module")
def L(torch):
    from distributional_rl_navigation_amd import _capi
    return _capi.lib()


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _stream(torch):
    from distributional_rl_navigation_amd import _capi
    return _capi.stream_ptr(torch.device(DEV))


def _bits(t):
    import torch
    return t.detach().contiguous().view(-1).view({1: torch.uint8, 4: torch.int32, 8: torch.int64}[t.element_size()]).cpu()


def _sentinels(torch, shape, dtype):
    return torch.full(shape, SENT, dtype=torch.int32, device=DEV).view(dtype)


class Net:
    """A policy with a weight image of the test's own and the 18 weight pointers; `reference(n)`: mn_dqn_act's Q-values and greedy actions of the first n
    rows of `obs`, computed once per n."""

    def __init__(self, torch, L, policy):
        self.torch, self.L, self.policy = torch, L, policy
        st, _ = policy._image(torch.device(DEV))
        self.ptrs = st["ptrs"]
        self.image = torch.empty(int(L.mn_dqn_image_floats()), dtype=torch.float32, device=DEV)
        self.obs = torch.randn(max(NS) + PAD, 26, generator=torch.Generator().manual_seed(26)).to(DEV)
        self._ref = {}

    def reference(self, n):
        if n not in self._ref:
            torch = self.torch
            q = torch.empty(n, 9, dtype=torch.float32, device=DEV)
            a = torch.empty(n, dtype=torch.int32, device=DEV)
            image = torch.empty_like(self.image)
            assert self.L.mn_dqn_act(_p(self.obs), self.ptrs, _p(image), 1, _p(q), _p(a), n, _stream(torch)) == 0
            self._ref[n] = (q.cpu(), a.cpu())
        return self._ref[n]


def _random_policy(torch, seed):
    """A seeded random init with every weight matrix scaled by 3: under nn.Linear's own init the biases decide, and every row chooses one action."""
    from distributional_rl_navigation_amd.dqn import DQNPolicy
    torch.manual_seed(seed)
    pol = DQNPolicy(device=DEV)
    with torch.no_grad():
        for p in pol.parameters():
            if p.dim() == 2:
                p.mul_(3.0)
    return pol


@pytest.fixture(scope="module", params=["golden", "random"])
def net(request, torch, L):
    from distributional_rl_navigation_amd.dqn import DQNPolicy
    if request.param == "golden":
        return Net(torch, L, DQNPolicy.load(GOLDEN, device=DEV))
    return Net(torch, L, _random_policy(torch, 77))


def _act(torch, L, net, n, eps, ctr, want_u, want_q, repack=1, seed=SEED):
    a = _sentinels(torch, (n + PAD,), torch.int32)
    u = _sentinels(torch, (n + PAD,), torch.float32) if want_u else None
    q = _sentinels(torch, (n + PAD, 9), torch.float32) if want_q else None
    rc = L.mn_dqn_act_rng(_p(net.obs), net.ptrs, _p(net.image), repack, seed, ctr, C.c_float(eps), _p(u), _p(q), _p(a), n, _stream(torch))
    assert rc == 0
    return a, u, q


@pytest.mark.parametrize("n", NS)
def test_actions_uniforms_and_qvalues(torch, L, net, n):
    q_ref, greedy = net.reference(n)
    if n >= 129:
        assert len(set(greedy.tolist())) > 1      # (the rows do not all choose one action)
    for ctr in CALLS:
        u_twin = D.dqn_act_uniforms(SEED, ctr, n)
        for eps in EPS:
            want = D.dqn_actions(SEED, ctr, eps, greedy.numpy())
            if 0 < eps < 1 and n >= 129:
                assert 0 < (want != greedy.numpy()).sum() < n
            # every output; the uniforms alone (rows that explore skip the network); no optional output
            for want_u, want_q in ((True, True), (True, False), (False, False)):
                a, u, q = _act(torch, L, net, n, eps, ctr, want_u, want_q)
                assert np.array_equal(a[:n].cpu().numpy(), want), (n, eps, ctr, want_u, want_q)
                assert (a[n:] == SENT).all()
                if want_u:
                    assert np.array_equal(u[:n].cpu().numpy().view(np.uint32), u_twin.view(np.uint32)), (n, eps, ctr)
                    assert (u[n:].view(torch.int32) == SENT).all()
                if want_q:      # every row, the exploring ones included
                    assert torch.equal(_bits(q[:n]), _bits(q_ref)), (n, eps, ctr)
                    assert (q[n:].view(torch.int32) == SENT).all()


def test_a_launch_with_two_greedy_rows(torch, L, net):
    """eps just below the two largest uniforms of the call: two rows are greedy, every other tile skips the network and the workgroups without a greedy
    row do not load the image."""
    n, ctr = 2051, 9
    u = D.dqn_act_uniforms(SEED, ctr, n)
    eps = float(np.sort(u)[-3])
    greedy_rows = np.nonzero(u > np.float32(eps))[0]
    assert len(greedy_rows) == 2 and 0 < eps < 1
    _, greedy = net.reference(n)
    want = D.dqn_actions(SEED, ctr, eps, greedy.numpy())
    assert np.array_equal(want[greedy_rows], greedy.numpy()[greedy_rows])
    a, _, _ = _act(torch, L, net, n, eps, ctr, False, False)
    assert np.array_equal(a[:n].cpu().numpy(), want) and (a[n:] == SENT).all()


def test_repack_switch(torch, L):
    net = Net(torch, L, _random_policy(torch, 5))
    n = 40
    _, greedy = net.reference(n)
    a0, _, _ = _act(torch, L, net, n, 0.0, 0, False, False, repack=1)
    assert torch.equal(a0[:n].cpu(), greedy)
    with torch.no_grad():
        net.policy.q_net.q_net[4].bias[5] += 1.0e3      # now action 5 wins everywhere
    a1, _, _ = _act(torch, L, net, n, 0.0, 1, False, False, repack=0)      # the old image
    assert torch.equal(a1[:n].cpu(), greedy) and not (greedy == 5).all()
    a2, _, _ = _act(torch, L, net, n, 0.0, 2, False, False, repack=1)      # the new one
    assert (a2[:n] == 5).all()
    a3, _, q3 = _act(torch, L, net, n, 0.3, 3, False, True, repack=0)      # ... which stays
    assert np.array_equal(a3[:n].cpu().numpy(), D.dqn_actions(SEED, 3, 0.3, np.full(n, 5, np.int32)))
    assert (q3[:n, 5] > 500).all()


def test_bad_arguments_launch_nothing(torch, L, net):
    n = 33
    a = _sentinels(torch, (n + PAD,), torch.int32)
    u = _sentinels(torch, (n + PAD,), torch.float32)
    q = _sentinels(torch, (n + PAD, 9), torch.float32)
    image = _sentinels(torch, (int(L.mn_dqn_image_floats()),), torch.float32)
    s = _stream(torch)
    holed = (C.c_void_p * 18)(*[net.ptrs[i] for i in range(18)])
    holed[11] = None
    call = lambda obs, w, im, act, rows: L.mn_dqn_act_rng(obs, w, im, 1, SEED, 0, C.c_float(0.5), _p(u), _p(q), act, rows, s)
    assert call(None, net.ptrs, _p(image), _p(a), n) == INVALID
    assert call(_p(net.obs), None, _p(image), _p(a), n) == INVALID
    assert call(_p(net.obs), holed, _p(image), _p(a), n) == INVALID
    assert call(_p(net.obs), net.ptrs, None, _p(a), n) == INVALID
    assert call(_p(net.obs), net.ptrs, _p(image), None, n) == INVALID
    assert call(_p(net.obs), net.ptrs, _p(image), _p(a), 0) == INVALID
    assert call(_p(net.obs), net.ptrs, _p(image), _p(a), -4) == INVALID
    torch.cuda.synchronize()
    for t in (a, u, q, image):      # not even the pack ran
        assert (t.view(torch.int32) == SENT).all()


# ---- the agent ----------------------------------------------------------------------------------------------------------------------------------------
def _agent(seed=11, **kw):
    from distributional_rl_navigation_amd.dqn import DQNAgent
    return DQNAgent(device=DEV, seed=seed, **dict(dict(buffer_size=48, batch_size=8, learning_starts=10 ** 9), **kw))


def test_agent_act_batch_equals_the_twin_and_counts_its_calls(torch):
    ag = _agent(fused_collect=True)
    assert ag.uses_fused_collect() and ag.act_seed == 11 + 4321 and ag.act_calls == 0
    obs = torch.randn(131, 26, generator=torch.Generator().manual_seed(3)).to(DEV)
    greedy = ag.policy.act_batch(obs).cpu().numpy()
    for k, eps in enumerate((1.0, 0.4, 0.0)):      # a falling rate; the counter advances at eps = 0 too
        a = ag.act_batch(obs, eps)
        assert a.dtype == torch.int32 and a.shape == (131,)
        assert np.array_equal(a.cpu().numpy(), D.dqn_actions(11 + 4321, k, eps, greedy)), (k, eps)
        assert ag.act_calls == k + 1
    a = ag.act_batch(obs, 0.4)      # call 3 draws other rows than call 1 did
    assert np.array_equal(a.cpu().numpy(), D.dqn_actions(11 + 4321, 3, 0.4, greedy))
    assert not np.array_equal(D.dqn_actions(11 + 4321, 3, 0.4, greedy), D.dqn_actions(11 + 4321, 1, 0.4, greedy))


def test_agent_without_the_switch_draws_from_the_torch_generator(torch):
    ag = _agent()
    assert not ag.fused_collect and not ag.uses_fused_collect()
    obs = torch.randn(70, 26, generator=torch.Generator().manual_seed(4)).to(DEV)
    greedy = ag.policy.act_batch(obs)
    gen = torch.Generator(device=DEV)
    gen.manual_seed(11 + 4321)
    for eps in (1.0, 0.3):      # dqn/agent.py's act_batch as it was, written out
        u = torch.rand(70, device=DEV, generator=gen)
        rnd = torch.randint(0, 9, (70,), device=DEV, dtype=torch.int32, generator=gen)
        assert torch.equal(ag.act_batch(obs, eps), torch.where(u < eps, rnd, greedy))
    assert torch.equal(ag.act_batch(obs, 0.0), greedy)
    assert ag.act_calls == 0


def test_collect_through_step_append_equals_step_and_add_vector_step(torch):
    """Three vector steps of `learn_vec` with the switch on (ring of 48 rows, 20 envs: the third step wraps) against the same actions through `step` and
    `add_vector_step` on an env made from the same seeds."""
    from distributional_rl_navigation_amd.marinenav_env.vec_env import VecMarineNavEnv
    n, steps, total = 20, 3, 100
    fused, plain, actor = _agent(fused_collect=True), _agent(), _agent(fused_collect=True)      # equal seeds: equal networks, equal draws
    env_a, env_b = (VecMarineNavEnv(n, seed=5, device=DEV, precision="f64") for _ in range(2))
    seen = []
    out = fused.learn_vec(steps, env_a, total_timesteps=total, callback=lambda ag, it: seen.append((it, ag.act_calls, ag.memory.ptr)))
    assert out["n_updates"] == 0 and seen == [(0, 1, 20), (1, 2, 40), (2, 3, 12)]
    obs = env_b.reset()
    for it in range(steps):
        eps = actor.exploration_rate(total)
        assert 0.0 < eps <= 1.0
        a = actor.act_batch(obs, eps)
        nxt, reward, done, info = env_b.step(a)
        plain.memory.add_vector_step(obs, a, reward, nxt, done)
        obs = env_b.reset_done()
        actor.num_timesteps += n
    ma, mb = fused.memory, plain.memory
    assert (ma.ptr, ma.size, len(ma)) == (mb.ptr, mb.size, len(mb)) == (12, 48, 48)
    for k in ("states", "next_states", "actions", "rewards", "dones"):
        assert torch.equal(_bits(getattr(ma, k)), _bits(getattr(mb, k))), k
    assert len(set(ma.actions.view(-1).tolist())) > 1 and fused.num_timesteps == steps * n
    env_a.close()
    env_b.close()
