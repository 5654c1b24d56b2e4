"""Every in-kernel random draw against its host twin (tests/rng_twin.py), bit for bit: the act call's taus and exploration uniforms in all five
kernel forms (csrc/iqn_act_common.h `draw_block`, iqn_act_split.h's shared-tau prep), the epsilon-greedy epilogue, `mn_iqn_sample`'s replay batch
and taus (csrc/mn_train_shared.h `perm_row`, csrc/iqn_train.hip `sample_tau`) and `mn_random_actions` (csrc/mn_rollout.hip `draw_action`).  What
the twin's streams are worth statistically is tests/test_rng_twin_cpu.py's subject; here draw number i of call c under seed s IS the twin's value.
The in-launch draws of the IQN and DQN gradient steps are pinned to `mn_iqn_sample` by their own tests.

Last, greedy actions at EXACT ties: output-layer rows copied onto others make Q-values bit-equal, and all act epilogues (the IQN forms,
`mn_dqn_act`, the two episode launches) must return the lowest tied index -- `first maximum wins`, like np.argmax."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import rng_twin as T      # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
# (name, kernel variant, shared_taus argument of fused_act)
FORMS = [("exact", 0, False), ("split", 2, False), ("shared", 2, True), ("wave", 2, "wave"), ("tiled", 2, "tiled")]
FORM_IDS = [f[0] for f in FORMS]
STATES = [(123, 0), (123, 2**32 - 1), (123, 2**32), (2**63 - 1, 0)]      # (seed, call counter) before the call


@pytest.fixture(scope="module")
def torch():
    import torch as t
    if not t.cuda.is_available():
        pytest.skip("no GPU")
    return t


@pytest.fixture(scope="module")
def net(torch):
    from distributional_rl_navigation_amd.iqn.model import ObsEncoder
    return ObsEncoder(26, 9, seed=7, device=DEV)


def _i64(x):
    x &= 2**64 - 1
    return x - 2**64 if x >= 2**63 else x


def _state(torch, seed, ctr):
    return torch.tensor([_i64(seed), _i64(ctr)], dtype=torch.int64, device=DEV)


def _obs(torch, n, seed=11):
    g = torch.Generator(device=DEV); g.manual_seed(seed)
    return (torch.randn(n, 26, device=DEV, generator=g) * 5.0).contiguous()


def _act(torch, net, form, obs, eps, cvar, seed, ctr, **kw):
    """One fused_act call of `form` from the generator state {seed, ctr}: (outputs, the call's draw buffer, the state afterwards)."""
    from distributional_rl_navigation_amd.iqn.fused_act import ActRng, act_context, fused_act
    _, variant, shared = form
    ctx = act_context(net)
    rng = ActRng(0, DEV)
    rng.state.copy_(_state(torch, seed, ctr))
    try:
        ctx.set_variant(variant)
        out = fused_act(net, obs, eps, cvar, rng=rng, shared_taus=shared, **kw)
    finally:
        ctx.set_variant(ctx.DEFAULT_VARIANT)
    return out, rng.draws(obs.shape[0], 32).cpu().numpy(), rng.state.cpu().numpy()


@pytest.mark.parametrize("form", FORMS, ids=FORM_IDS)
def test_act_draws_equal_the_twin(torch, net, form):
    """n = 1, 2, 3, 5: the scalar tail of `draw_block` after 33 n mod 4 = 1, 2, 3, 1 values; 4 and 64: the exact multiple of the float4 path."""
    is_shared = bool(form[2])
    for n in (1, 2, 3, 4, 5, 63, 64, 65, 1000):
        obs = _obs(torch, n)
        cv_rows = torch.rand(n, device=DEV, generator=torch.Generator(device=DEV).manual_seed(n)) * 0.9 + 0.1
        for ci, cvar in enumerate((1.0, 0.25) if is_shared else (1.0, 0.25, cv_rows)):
            for si, (seed, ctr) in enumerate(STATES):
                quant = (ci + si) % 2 == 1
                out, draws, state = _act(torch, net, form, obs, 0.3, cvar, seed, ctr, want_quantiles=quant)
                want = T.act_draws(seed, ctr, n, cvar.cpu().numpy() if torch.is_tensor(cvar) else cvar, shared=is_shared)
                where = (form[0], n, ci, seed, ctr)
                assert np.array_equal(draws[:want.size].view(np.uint32), want.view(np.uint32)), where
                assert state.view(np.uint64).tolist() == [seed, ctr + 1], where
                if quant:      # act_eval's `taus` [n, 32, 1]: the call's draws x cvar
                    taus = out[2].cpu().numpy().reshape(n, 32)
                    want_t = np.broadcast_to(want[:32], (n, 32)) if is_shared else want[:32 * n].reshape(n, 32)
                    assert np.array_equal(taus, want_t), where
                    lim = cvar.cpu().numpy().reshape(n, 1) if torch.is_tensor(cvar) else np.float32(cvar)
                    assert (taus <= lim).all() and (taus >= 0).all()


@pytest.mark.parametrize("quant", [False, True], ids=["act", "act_eval"])
@pytest.mark.parametrize("form", FORMS, ids=FORM_IDS)
def test_exploration_epilogue_equals_the_twin(torch, net, form, quant):
    """Every row's action is `explore_action(twin uniform, eps, first argmax of the row's own returned Q)` -- with no row excluded."""
    n = 4096
    obs = _obs(torch, n, seed=5)
    for k, eps in enumerate((1.0, 0.3, 0.05)):
        seed, ctr = STATES[k]
        out, draws, _ = _act(torch, net, form, obs, eps, 1.0, seed, ctr, want_qvals=True, want_quantiles=quant)
        a, q = out[0].cpu().numpy(), out[-1].cpu().numpy()
        want = T.act_draws(seed, ctr, n, 1.0, shared=bool(form[2]))
        assert np.array_equal(draws[:want.size], want)
        u = want[-n:]
        expect = T.explore_action(u, eps, q.argmax(1))
        bad = np.flatnonzero(a != expect)
        assert bad.size == 0, (form[0], eps, bad.size, bad[:5], u[bad[:5]], a[bad[:5]], expect[bad[:5]])


SAMPLE_CASES = [(1, 1), (2, 2), (3, 3), (5, 5), (17, 16), (64, 64), (65, 64), (1024, 1024), (1025, 1024), (100_000, 256), (2**31 - 1, 64)]


@pytest.mark.parametrize("ring,batch", SAMPLE_CASES)
def test_mn_iqn_sample_equals_the_twin(torch, ring, batch):
    from distributional_rl_navigation_amd import _capi
    L = _capi.lib()
    p = lambda t: C.c_void_p(t.data_ptr())
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    max_taus = 2 * 1024 * 8
    for n_taus in (0, 1, 2 * batch * 8, max_taus):
        for seed, ctr in STATES + [(2**64 - 1, 1)]:
            st = _state(torch, seed, ctr)
            idx = torch.full((1024 + 8,), -7, dtype=torch.int64, device=DEV)
            taus = torch.full((max_taus + 8,), -7.0, device=DEV)
            assert L.mn_iqn_sample(ring, batch, p(st), p(idx), p(taus), n_taus, stream) == 0
            idx, taus = idx.cpu().numpy(), taus.cpu().numpy()
            base = T.sample_base(seed, ctr)
            where = (ring, batch, n_taus, seed, ctr)
            want_idx = T.perm_row(base, ring, np.arange(batch))
            assert np.array_equal(idx[:batch], want_idx) and (idx[batch:] == -7).all(), where      # ... and nothing written behind the batch
            assert np.array_equal(taus[:n_taus], T.sample_taus(base, n_taus)) and (taus[n_taus:] == -7.0).all(), where
            assert st.cpu().numpy().view(np.uint64).tolist() == [seed, ctr + 1], where
            assert idx[:batch].min() >= 0 and idx[:batch].max() < ring and np.unique(idx[:batch]).size == batch
            if batch == ring:
                assert np.array_equal(np.sort(idx[:batch]), np.arange(ring)), where


@pytest.mark.parametrize("n", [1, 63, 64, 65, 1000])
def test_mn_random_actions_equal_the_twin(torch, n):
    from distributional_rl_navigation_amd import _capi
    L = _capi.lib()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def launch(seed, step, env0, count):
        out = torch.full((count + 8,), -7, dtype=torch.int32, device=DEV)
        assert L.mn_random_actions(seed, step, env0, count, C.c_void_p(out.data_ptr()), stream) == 0
        out = out.cpu().numpy()
        assert (out[count:] == -7).all()
        return out[:count]
    e = np.arange(n, dtype=np.uint64)
    for seed in (0, 42, 2**64 - 1):
        for step in (0, 7, 2**32, 2**64 - 2):
            for env0 in (0, 65536, 2**32 + 5):
                got = launch(seed, step, env0, n)
                assert np.array_equal(got, T.random_action(seed, step, T.u64(env0) + e)), (n, seed, step, env0)
            whole = launch(seed, step, 0, 1000 + n)      # a shard (env0 = k, n) is the slice [k : k + n] of the launch at env0 = 0
            for k in (1, 37, 1000):
                assert np.array_equal(launch(seed, step, k, n), whole[k:k + n]), (n, seed, step, k)


def test_vec_env_random_actions_are_the_twins(torch):
    from distributional_rl_navigation_amd.marinenav_env.vec_env import VecMarineNavEnv
    env = VecMarineNavEnv(65, seed=0, device=DEV, first_index=1000)
    try:
        for seed, step in ((42, 0), (42, 9), (2**63 - 1, 2**32)):
            got = env.random_actions(seed, step).cpu().numpy()
            assert np.array_equal(got, T.random_action(seed, step, np.arange(1000, 1065, dtype=np.uint64))), (seed, step)
    finally:
        env.close()


# ---- greedy action at exact ties ------------------------------------------------------------------------------------------------------------------
TIES = [(2, 5), (0, 8), (3, 4, 7), tuple(range(9))]
DQN_TIES = TIES + [(3, 8), (3, 4)]      # dqn_argmax: lane group g holds actions 4 g .. 4 g + 3, so these pairs meet in the cross-lane reduction


def _tie(torch, layer, tied, lift):
    """Copies the output layer's row and bias of tied[0] onto the other tied actions and raises the tied biases by `lift`."""
    with torch.no_grad():
        for a in tied[1:]:
            layer.weight[a] = layer.weight[tied[0]]
            layer.bias[a] = layer.bias[tied[0]]
        for a in tied:
            layer.bias[a] += lift


def _check_ties(q, a, tied, where):
    """At least 90 % of the rows have bit-equal maxima at exactly the tied actions; on each of them the action is the lowest tied index."""
    q, a = np.asarray(q), np.asarray(a)
    top = q.max(1, keepdims=True)
    is_max = q == top
    want = np.zeros(9, dtype=bool); want[list(tied)] = True
    rows = (is_max == want).all(1) & (q[:, list(tied)].view(np.uint32) == q[:, [tied[0]]].view(np.uint32)).all(1)
    assert rows.mean() >= 0.9, (where, rows.mean())
    assert (a[rows] == min(tied)).all(), (where, np.unique(a[rows]))


@pytest.mark.parametrize("tied", TIES, ids=lambda t: "-".join(map(str, t)))
@pytest.mark.parametrize("form", FORMS, ids=FORM_IDS)
def test_iqn_greedy_action_at_exact_ties(torch, form, tied):
    from distributional_rl_navigation_amd.iqn.fused_act import weights_changed
    from distributional_rl_navigation_amd.iqn.model import ObsEncoder
    net = ObsEncoder(26, 9, seed=7, device=DEV)
    obs = _obs(torch, 1000, seed=3)
    (_, q0), _, _ = _act(torch, net, form, obs, 0.0, 1.0, 9, 0, want_qvals=True)
    _tie(torch, net.output_layer, tied, 2.0 * float(q0.max() - q0.min()) + 1.0)
    weights_changed(net)
    (a, q), _, _ = _act(torch, net, form, obs, 0.0, 1.0, 9, 0, want_qvals=True)
    _check_ties(q.cpu().numpy(), a.cpu().numpy(), tied, form[0])
    # act_eval's kernel of the form: the output layer per tau, Q = their mean
    (a, _, _, q), _, _ = _act(torch, net, form, obs, 0.0, 1.0, 9, 0, want_qvals=True, want_quantiles=True)
    _check_ties(q.cpu().numpy(), a.cpu().numpy(), tied, form[0] + " act_eval")


@pytest.mark.parametrize("tied", DQN_TIES, ids=lambda t: "-".join(map(str, t)))
def test_dqn_greedy_action_at_exact_ties(torch, tied):
    from distributional_rl_navigation_amd.dqn.policy import DQNPolicy
    torch.manual_seed(5)
    pol = DQNPolicy(device=DEV)
    obs = _obs(torch, 1000, seed=3)
    q0 = pol.q_values(obs)
    _tie(torch, pol.q_net.q_net[4], tied, 2.0 * float(q0.max() - q0.min()) + 1.0)
    pol.weights_changed()
    q, a = pol._fused(obs, True, True)
    _check_ties(q.cpu().numpy(), a.cpu().numpy(), tied, "mn_dqn_act")
    assert torch.equal(a, pol.act_batch(obs))


def test_episode_launches_take_the_lowest_tied_action(torch):
    """One step of `mn_rollout_dqn` and of `mn_rollout_iqn` at n = 37 with tied output rows: the rollout copies of the two epilogues."""
    from distributional_rl_navigation_amd.dqn.policy import DQNPolicy
    from distributional_rl_navigation_amd.iqn.fused_act import ActRng, rollout_iqn, weights_changed
    from distributional_rl_navigation_amd.iqn.model import ObsEncoder
    from distributional_rl_navigation_amd.marinenav_env.vec_env import VecMarineNavEnv
    n = 37
    for tied in ((3, 8), (0, 8), (3, 4, 7)):
        torch.manual_seed(5)
        pol = DQNPolicy(device=DEV)
        env = VecMarineNavEnv(n, seed=2, device=DEV)
        try:
            env.reset()
            q0 = pol.q_values(env.obs.contiguous())
            _tie(torch, pol.q_net.q_net[4], tied, 2.0 * float(q0.max() - q0.min()) + 1.0)
            pol.weights_changed()
            out = pol.rollout(env, 1, trace=("action", "q"))
            _check_ties(out["q"][0].cpu().numpy(), out["action"][0].cpu().numpy(), tied, "mn_rollout_dqn")
        finally:
            env.close()
        net = ObsEncoder(26, 9, seed=7, device=DEV)
        env = VecMarineNavEnv(n, seed=2, device=DEV)
        try:
            env.reset()
            (_, q0), _, _ = _act(torch, net, FORMS[1], env.obs.contiguous(), 0.0, 1.0, 9, 0, want_qvals=True)
            _tie(torch, net.output_layer, tied, 2.0 * float(q0.max() - q0.min()) + 1.0)
            weights_changed(net)
            out = rollout_iqn(net, env, 1, ActRng(9, DEV), trace=("action", "q"))
            assert out is not None
            _check_ties(out["q"][0].cpu().numpy(), out["action"][0].cpu().numpy(), tied, "mn_rollout_iqn")
        finally:
            env.close()
