"""The DQN baseline's multi-step gradient call (`mn_dqn_train_steps`, csrc/dqn_train.hip) on the GPU: bit for bit the loop of single
`mn_dqn_train_step` launches -- parameters, Adam state, counters, the last gradient, EVERY step's loss and rows (a stale parameter read between
steps shows from the second loss on) -- in draw mode and with given rows, at every tile shape, however a run is split into calls; a float64
yardstick for the last step of a call; the argument checks; `DQNAgent.train_many` and the train_dqn driver either way."""
import copy
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LR = 1e-4
RING = 2048


@pytest.fixture(scope="module")
def torch():
    import torch as t
    if not t.cuda.is_available():
        pytest.skip("no GPU")
    return t


def _agent(torch, batch=32, buffer_size=RING, seed=3):
    from distributional_rl_navigation_amd.dqn import DQNAgent
    return DQNAgent(device=DEV, buffer_size=buffer_size, batch_size=batch, seed=seed, fused_train=True)


@pytest.fixture(scope="module")
def ring(torch):
    """A replay ring filled from a small rollout of the HIP env (random actions, auto-reset): 256 envs x 8 steps."""
    from distributional_rl_navigation_amd.marinenav_env.vec_env import VecMarineNavEnv
    env = VecMarineNavEnv(256, seed=5, device=DEV)
    ag = _agent(torch)
    obs = env.reset()
    for _ in range(8):
        a = ag.act_batch(obs, 1.0)
        nxt, r, d, _ = env.step(a)
        ag.memory.add_vector_step(obs, a, r, nxt, d)
        obs = env.reset_done()
    env.close()
    m = ag.memory
    assert m.size == RING
    return tuple(t.clone() for t in (m.states, m.actions, m.rewards, m.next_states, m.dones))


@pytest.fixture(scope="module")
def rig(torch, ring):
    """One fused agent whose state the tests restore, with a target network that differs from the local one and a non-zero Adam state."""
    ag = _agent(torch)
    _load_ring(ag, ring)
    ft = ag._fused_trainer()
    for _ in range(3):
        ft.step(ring, RING, 32)
    ag._train_path = "hip"
    ft.rng_state.copy_(torch.tensor([99991, 17], dtype=torch.int64))
    return ag, _State(ag)


def _load_ring(ag, ring):
    m = ag.memory
    n = ring[0].shape[0]
    for dst, src in zip((m.states, m.actions, m.rewards, m.next_states, m.dones), ring):
        dst[:n].copy_(src)
    m.size, m.ptr = n, n % m.capacity


class _State:
    """Snapshot / restore of a fused agent's whole training state (parameters, target, Adam moments, step and draw counters)."""

    def __init__(self, ag):
        ft = ag._fused_trainer()
        self.ag, self.t = ag, [x.clone() for x in self._tensors(ft)]

    @staticmethod
    def _tensors(ft):
        return (ft.local, ft.target, ft.exp_avg, ft.exp_avg_sq, ft.step_dev, ft.rng_state)

    def restore(self):
        for d, s in zip(self._tensors(self.ag._fused), self.t):
            d.copy_(s)
        self.ag._train_path = "hip"      # the device counter is authoritative: the next eager step takes it over
        self.ag.policy.weights_changed()


def _bits(t):
    """The tensor's bytes: `==` on these tells -0 from +0 and equal NaNs from different ones."""
    import torch
    return t.detach().contiguous().view(-1).view({4: torch.int32, 8: torch.int64}[t.element_size()]).cpu()


def _outcome(torch, ft, losses, rows):
    return dict(params=_bits(ft.local), exp_avg=_bits(ft.exp_avg), exp_avg_sq=_bits(ft.exp_avg_sq), step=_bits(ft.step_dev), rng=_bits(ft.rng_state),
                grad=_bits(ft.grad), losses=_bits(losses), rows=_bits(rows))


def _same(torch, got, want):
    for k in want:
        assert got[k].shape == want[k].shape and torch.equal(got[k], want[k]), k


def _loop(torch, ag, state, ring, ring_size, batch, K, idx=None):
    """K single launches from `state`; checks that the first one already moved the parameters."""
    ft = ag._fused
    state.restore()
    losses, rows = [], []
    for k in range(K):
        losses.append(ft.step(ring, ring_size, batch, None if idx is None else idx[k]).clone())
        rows.append(ft.last_idx.clone())
        if k == 0:
            assert not torch.equal(ft.local, state.t[0])      # or the comparison proves nothing
    return _outcome(torch, ft, torch.stack(losses), torch.stack(rows))


def _call(torch, ag, state, ring, ring_size, batch, cuts, idx=None):
    """The same steps as multi-step calls of `cuts` steps each, from `state`."""
    ft = ag._fused
    state.restore()
    losses, rows, k0 = [], [], 0
    for K in cuts:
        losses.append(ft.steps(ring, ring_size, batch, K, None if idx is None else idx[k0:k0 + K]).clone())
        rows.append(ft.last_idx.clone())
        k0 += K
    return _outcome(torch, ft, torch.cat(losses), torch.cat(rows))


@pytest.mark.parametrize("batch,K", [(32, 3), (32, 1), (17, 3), (16, 3), (5, 4), (1, 2)])
def test_bitwise_against_the_loop_draw_mode(torch, ring, rig, batch, K):
    """Batch 17: the second tile with one live slot; 16: one tile; 5 and 1: a partly filled tile.  A ring size that is no power of two."""
    ag, state = rig
    want = _loop(torch, ag, state, ring, 1000, batch, K)
    got = _call(torch, ag, state, ring, 1000, batch, [K])
    _same(torch, got, want)
    assert int(ag._fused.step_dev.item()) == int(state.t[4].item()) + K and ag._fused.rng_state.tolist() == [99991, 17 + K]
    assert got["rows"].shape == (K * batch,) and int(got["rows"].max()) < 1000


@pytest.mark.parametrize("ring_size", [32, RING])
def test_smallest_legal_ring_and_full_ring(torch, ring, rig, ring_size):
    ag, state = rig
    want = _loop(torch, ag, state, ring, ring_size, 32, 3)
    _same(torch, _call(torch, ag, state, ring, ring_size, 32, [3]), want)
    if ring_size == 32:      # every step draws the whole ring, each in its own order
        assert all(sorted(r.tolist()) == list(range(32)) for r in want["rows"].view(3, 32))


def test_given_rows(torch, ring, rig):
    """idx [K][batch] with a row repeated inside a batch and the same row in two steps."""
    ag, state = rig
    gen = torch.Generator(device=DEV).manual_seed(11)
    for batch, K in ((32, 3), (17, 4)):
        idx = torch.randint(0, RING, (K, batch), device=DEV, generator=gen)
        idx[0, 1] = idx[0, 0]
        idx[1, batch - 1] = idx[1, 0]
        idx[2, 0] = idx[0, 0]
        want = _loop(torch, ag, state, ring, RING, batch, K, idx)
        got = _call(torch, ag, state, ring, RING, batch, [K], idx)
        _same(torch, got, want)
        assert torch.equal(got["rows"], _bits(idx)) and got["rng"].tolist() == [99991, 17]      # the draw counter is left alone


def test_splitting_is_invisible(torch, ring, rig):
    ag, state = rig
    one = _call(torch, ag, state, ring, RING, 32, [6])
    _same(torch, _call(torch, ag, state, ring, RING, 32, [2, 4]), one)
    _same(torch, _call(torch, ag, state, ring, RING, 32, [1, 5]), one)
    _same(torch, one, _loop(torch, ag, state, ring, RING, 32, 6))


def _f64_step(torch, ag, batch):
    """Loss and clipped gradient of DQN.train in float64 from the agent's current networks."""
    import torch.nn.functional as F
    q = copy.deepcopy(ag.q_net).double()
    t = copy.deepcopy(ag.q_net_target).double()
    obs, act, rew, nxt, done = (x.double() if x.dtype == torch.float32 else x for x in batch)
    with torch.no_grad():
        y = rew + (1 - done) * ag.gamma * t(nxt).max(dim=1)[0].reshape(-1, 1)
    loss = F.smooth_l1_loss(torch.gather(q(obs), 1, act.long()), y)
    loss.backward()
    torch.nn.utils.clip_grad_norm_(q.parameters(), ag.max_grad_norm)
    return float(loss.detach()), np.concatenate([p.grad.cpu().numpy().ravel() for p in q.parameters()])


def _flat(ag, what="param"):
    ps = list(ag.q_net.parameters())
    return np.concatenate([(p.grad if what == "grad" else p).detach().double().cpu().numpy().ravel() for p in ps])


def test_last_step_against_float64(torch, ring, rig):
    """Step 3 of a 3-step call against DQN.train in float64 from the state after step 2, with the eager float32 step's own error as the bar
    (1.5 x that + 1e-6): ties the call to the arithmetic, not only to its twin."""
    ag, state = rig
    m = ag.memory
    gen = torch.Generator(device=DEV).manual_seed(23)
    for batch in (32, 17):
        idx = torch.stack([torch.randperm(RING, device=DEV, generator=gen)[:batch] for _ in range(3)])
        state.restore()
        ag._fused.steps(ring, RING, batch, 2, idx[:2])
        rows = tuple(t[idx[2]] for t in (m.states, m.actions, m.rewards, m.next_states, m.dones))
        loss64, g64 = _f64_step(torch, ag, rows)
        loss_e = float(ag.train(rows))
        g_e, p_e = _flat(ag, "grad"), _flat(ag)
        ag._enter_train_path("hip")
        state.restore()      # (the eager step moved the shared parameters and moments)
        losses = ag._fused.steps(ring, RING, batch, 3, idx)
        loss_f, g_f, p_f = float(losses[2]), ag._fused.grad.double().cpu().numpy(), ag._fused.local.double().cpu().numpy()
        lbar = 1.5 * abs(loss_e - loss64) + 1e-6
        assert abs(loss_f - loss64) <= lbar, (loss_f, loss_e, loss64)
        gbar = 1.5 * np.abs(g_e - g64).max() + 1e-6
        assert np.abs(g_f - g64).max() <= gbar, (np.abs(g_f - g64).max(), np.abs(g_e - g64).max())
        big = np.abs(g64) > 100 * gbar
        assert np.abs(p_f - p_e)[big].max(initial=0) <= 2e-6
        assert np.abs(p_f - p_e).max() <= 2 * LR


def test_arguments(torch, ring, rig):
    from distributional_rl_navigation_amd import _capi
    ag, state = rig
    state.restore()
    ft = ag._fused
    L = _capi.lib()
    p = lambda t: C.c_void_p(t.data_ptr())
    ws = torch.zeros(L.mn_dqn_train_steps_workspace_floats(32, 4), dtype=torch.float32, device=DEV)
    losses = torch.zeros(4, dtype=torch.float32, device=DEV)
    out = torch.zeros(4 * 33, dtype=torch.int64, device=DEV)
    idx = torch.zeros(4 * 33, dtype=torch.int64, device=DEV)
    states, actions, rewards, next_states, dones = ring

    def call(batch=32, n_steps=4, ring_size=RING, rng=ft.rng_state, rows=None):
        return L.mn_dqn_train_steps(p(states), p(next_states), p(actions), p(rewards), p(dones), ring_size, p(rng) if rng is not None else None,
                                    p(rows) if rows is not None else None, p(out), p(ft.local), p(ft.target), p(ws), p(ft.grad), p(losses), p(ft.exp_avg),
                                    p(ft.exp_avg_sq), p(ft.step_dev), batch, n_steps, C.c_float(0.99), C.c_double(LR), C.c_double(0.9), C.c_double(0.999),
                                    C.c_double(1e-8), C.c_double(10.0), _capi.stream_ptr(torch.device(DEV)))

    INVALID = -1      # MN_ERR_INVALID
    assert call(batch=33) == INVALID and call(batch=33, rng=None, rows=idx) == INVALID
    assert call(n_steps=0) == INVALID and call(n_steps=-1) == INVALID
    assert call(ring_size=31) == INVALID
    assert call(rng=None, rows=None) == INVALID
    torch.cuda.synchronize()
    for d, s in zip(_State._tensors(ft), state.t):
        assert torch.equal(d, s)
    assert call() == 0 and call(rng=None, rows=idx, batch=32) == 0      # the same buffers are fine with legal arguments
    torch.cuda.synchronize()
    assert not torch.equal(ft.local, state.t[0])
    state.restore()


def test_agent_train_many(torch, ring):
    many, loop = _agent(torch, seed=21), _agent(torch, seed=21)
    for ag in (many, loop):
        _load_ring(ag, ring)
    obs = ring[0][:64].contiguous()
    many.policy.act_batch(obs)      # builds the act kernel's weight image BEFORE the steps: a stale image would act on these weights
    losses = many.train_many(7)
    want = torch.stack([loop.train() for _ in range(7)])
    assert many.n_updates == loop.n_updates == 7 and losses.shape == (7,) and torch.equal(_bits(losses), _bits(want))
    a, b = many._fused, loop._fused
    for x, y in ((a.local, b.local), (a.exp_avg, b.exp_avg), (a.exp_avg_sq, b.exp_avg_sq), (a.step_dev, b.step_dev), (a.rng_state, b.rng_state), (a.grad, b.grad)):
        assert torch.equal(_bits(x), _bits(y))
    assert a.last_idx.shape == (7, 32) and torch.equal(a.last_idx[6], b.last_idx)
    with torch.no_grad():
        q_eager = many.q_net(obs)
    assert torch.equal(many.policy.act_batch(obs).long(), q_eager.argmax(dim=1))
    # the eager step afterwards continues the one Adam state
    m = many.memory
    rows = torch.arange(32, device=DEV)
    many.train(tuple(t[rows] for t in (m.states, m.actions, m.rewards, m.next_states, m.dones)))
    p0 = next(iter(many.q_net.parameters()))
    assert float(many.optimizer.state[p0]["step"]) == 8 and many.optimizer.state[p0]["exp_avg"].data_ptr() == a.exp_avg.data_ptr()
    assert many.n_updates == 8
    # above batch 32 train_many is the loop of single launches
    big = _agent(torch, batch=64, seed=21)
    _load_ring(big, ring)
    assert big.train_many(2).shape == (2,) and big.n_updates == 2 and int(big._fused.step_dev.item()) == 2


def _nested_equal(a, b):
    """Equality of ragged nests (object arrays / lists of arrays), leaf by leaf."""
    if isinstance(a, (list, tuple)) or (isinstance(a, np.ndarray) and a.dtype == object):
        return isinstance(b, (list, tuple, np.ndarray)) and len(a) == len(b) and all(_nested_equal(x, y) for x, y in zip(a, b))
    return np.array_equal(np.asarray(a), np.asarray(b))


def test_driver_files_are_equal_either_way(torch, tmp_path):
    """The toy reference-budget run of tests/test_reference_budget_gpu.py with the gradient steps as multi-step calls and as single launches."""
    from distributional_rl_navigation_amd.train_dqn import run_trial
    from distributional_rl_navigation_amd.train_iqn import create_eval_configs
    TOTAL, N = 4_000, 16
    REFERENCE = dict(learning_starts=400, target_update_interval=400)
    cfg = create_eval_configs(DEV)
    eval_config = {k: cfg[k] for k in list(cfg)[:3]}      # three evaluation worlds
    runs = []
    for name, per_call in (("multi", "multi"), ("single", 1)):
        params = dict(agent="DQN", seed=3, total_timesteps=TOTAL, eval_freq=400, save_dir=str(tmp_path), training_time=name)
        d, agent = run_trial(DEV, params, N, verbose=False, env_budget="reference", reference=REFERENCE, eval_config=eval_config, max_eval_steps=60,
                             return_agent=True, train_steps_per_call=per_call)
        assert agent.n_updates == 3_600
        runs.append((d, _bits(agent._fused.local), _bits(agent._fused.target)))
    (da, pa, ta), (db, pb, tb) = runs
    assert torch.equal(pa, pb) and torch.equal(ta, tb)
    for f in ("evaluations.npz", "training_log.npz"):
        za, zb = (np.load(os.path.join(d, f), allow_pickle=True) for d in (da, db))
        assert sorted(za.files) == sorted(zb.files) and len(za.files) > 0
        for k in za.files:
            if za[k].dtype == object:
                assert _nested_equal(za[k], zb[k]), (f, k)      # (actions: per evaluation point a list of per-world arrays of different lengths)
            else:
                assert np.array_equal(za[k], zb[k], equal_nan=za[k].dtype.kind == "f"), (f, k)
