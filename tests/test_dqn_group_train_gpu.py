"""Many DQN learners per launch (`mn_dqn_group_train_step` / `mn_dqn_group_train_steps`, csrc/dqn_train.hip; dqn/group_train.py; `run_trials_together`)
on the GPU: every learner of a grouped launch is BYTE for byte what the single calls leave from the same state -- parameters, both moments, step and draw
counters, gradient, every loss, every row -- at every tile shape, in draw mode and with given rows, for a group of one and at the limit of 64; nothing is
written outside a learner's own buffers (guard words); group and single calls interleave on one agent; the argument checks; the driver's files.

The learners of the kernel-level cases live in ONE int32 arena: per learner local | target | grad | exp_avg | exp_avg_sq | step | draw state, then the
grouped workspace, with guard words in front of every buffer and behind the last.  Comparing the arena in front of the workspace compares every field of
every learner and every guard at once."""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LR, GAMMA = 1e-4, 0.99
RING = 2048
P_TOTAL = 27650
VEC = 27652          # a vector's slot: its 27 650 floats and two guard words
GUARD = 4
SENT = 0x7FC0DEAD    # (a NaN with a payload, as float)
INVALID = -1         # MN_ERR_INVALID
FIELDS = ("local", "target", "grad", "exp_avg", "exp_avg_sq")


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


def _agent(torch, batch=32, seed=3, buffer_size=RING):
    from distributional_rl_navigation_amd.dqn import DQNAgent
    return DQNAgent(device=DEV, buffer_size=buffer_size, batch_size=batch, seed=seed, fused_train=True)


@pytest.fixture(scope="module")
def rings(torch):
    """Three replay rings of 2 048 rows, each from its own 256-env, 8-step rollout of the HIP env (random actions, auto-reset)."""
    from distributional_rl_navigation_amd.marinenav_env.vec_env import VecMarineNavEnv
    out = []
    for seed in (5, 6, 7):
        env = VecMarineNavEnv(256, seed=seed, device=DEV)
        ag = _agent(torch, seed=seed)
        obs = env.reset()
        for _ in range(8):
            a = ag.act_batch(obs, 1.0)
            nxt, r, d, _ = env.step(a)
            ag.memory.add_vector_step(obs, a, r, nxt, d)
            obs = env.reset_done()
        env.close()
        m = ag.memory
        assert m.size == RING
        out.append(tuple(t.clone() for t in (m.states, m.actions, m.rewards, m.next_states, m.dones)))
    assert not torch.equal(out[0][0], out[1][0])
    return out


@pytest.fixture(scope="module")
def base_params(torch):
    """Two freshly initialised networks as flat vectors (local, target)."""
    flat = lambda ag: torch.cat([p.detach().reshape(-1) for p in ag.q_net.parameters()]).clone()
    a, b = flat(_agent(torch, seed=11)), flat(_agent(torch, seed=12))
    assert a.numel() == P_TOTAL
    return a, b


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _stream(torch):
    from distributional_rl_navigation_amd import _capi
    return _capi.stream_ptr(torch.device(DEV))


HYPER = (C.c_float(GAMMA), C.c_double(LR), C.c_double(0.9), C.c_double(0.999), C.c_double(1e-8), C.c_double(10.0))


class Arena:
    """G learners and the grouped workspace as slices of one allocation, with guard words between them."""

    def __init__(self, torch, L, G, rings, base_params, ws_floats):
        self.torch, self.L, self.G = torch, L, G
        self.rings = [rings[g % len(rings)] for g in range(G)]
        per = len(FIELDS) * (GUARD + VEC) + 2 * (GUARD + 4)
        self.ws_off = G * per + GUARD
        n = self.ws_off + ws_floats + GUARD
        self.mem = torch.full((n,), SENT, dtype=torch.int32, device=DEV)
        self.guard = torch.ones(n, dtype=torch.bool, device=DEV)
        self.learners = []
        gen = torch.Generator(device=DEV).manual_seed(1234)
        o = 0
        for g in range(G):
            ln = {}
            for f in FIELDS:
                o += GUARD
                ln[f] = self.mem[o:o + P_TOTAL].view(torch.float32)
                self.guard[o:o + P_TOTAL] = False
                o += VEC
            o += GUARD
            ln["step"] = self.mem[o:o + 1]
            self.guard[o:o + 1] = False
            o += 4 + GUARD
            ln["rng"] = self.mem[o:o + 4].view(torch.int64)
            self.guard[o:o + 4] = False
            o += 4
            for f, base in zip(("local", "target"), base_params):      # each learner its own networks, the target unlike the local one
                ln[f].copy_(base * (1 + 0.1 * torch.randn(P_TOTAL, device=DEV, generator=gen)))
            for f in ("grad", "exp_avg", "exp_avg_sq"):
                ln[f].zero_()
            ln["step"].zero_()
            self.learners.append(ln)
        assert o + GUARD == self.ws_off
        self.ws = self.mem[self.ws_off:self.ws_off + ws_floats].view(torch.float32)
        self.guard[self.ws_off:self.ws_off + ws_floats] = False
        self.ws.zero_()
        assert self.ws.data_ptr() % 16 == 0
        # a non-zero Adam state: three single steps each, then a draw state of its own
        ws1, loss1 = self.single_ws(32), torch.zeros(1, device=DEV)
        for g, ln in enumerate(self.learners):
            for k in range(3):
                idx = torch.randint(0, RING, (32,), device=DEV, generator=gen)
                assert self.single_step(g, RING, 32, ws1, loss1, None, idx) == 0
            ln["rng"].copy_(torch.tensor([99991 + 7 * g, 17 + g], dtype=torch.int64))
        torch.cuda.synchronize()
        self.snap = self.mem.clone()
        assert bool((self.snap[self.guard] == SENT).all()) and int(self.guard.sum()) >= GUARD * (G * 7 + 2)
        self.handle = self.create()

    def restore(self):
        self.mem.copy_(self.snap)

    def head(self):
        """Every learner's every field, and the guards among them, as bytes."""
        return self.mem[:self.ws_off].clone().cpu()

    def moved(self, g):
        """Whether learner g's parameters differ from the snapshot's."""
        ln = self.learners[g]["local"]
        o = (ln.data_ptr() - self.mem.data_ptr()) // 4
        return not self.torch.equal(ln.view(self.torch.int32), self.snap[o:o + P_TOTAL])

    def guards_intact(self):
        return bool((self.mem[self.guard] == SENT).all())

    def table(self, n=None):
        from distributional_rl_navigation_amd import _capi
        n = self.G if n is None else n
        tab = (_capi.MnDqnLearner * max(n, 1))()
        for g in range(n):
            ln, ring = self.learners[g % self.G], self.rings[g % self.G]
            row = tab[g]
            row.ring_states, row.ring_actions, row.ring_rewards, row.ring_next_states, row.ring_dones = (t.data_ptr() for t in ring)
            row.rng_state, row.params_local, row.params_target = ln["rng"].data_ptr(), ln["local"].data_ptr(), ln["target"].data_ptr()
            row.grad, row.exp_avg, row.exp_avg_sq, row.step = ln["grad"].data_ptr(), ln["exp_avg"].data_ptr(), ln["exp_avg_sq"].data_ptr(), ln["step"].data_ptr()
        return tab

    def create(self, tab=None, n=None):
        h = C.c_void_p()
        rc = self.L.mn_dqn_group_create(self.table() if tab is None else tab, self.G if n is None else n, C.byref(h))
        if rc:
            assert not h.value
            return rc
        return h

    def single_ws(self, batch):
        return self.torch.zeros(self.L.mn_dqn_train_workspace_floats(batch), dtype=self.torch.float32, device=DEV)

    def _single_args(self, g, ring_size, draw, idx, out, ws, loss):
        ln = self.learners[g]
        states, actions, rewards, next_states, dones = self.rings[g]
        return (_p(states), _p(next_states), _p(actions), _p(rewards), _p(dones), ring_size, _p(ln["rng"]) if draw else None, _p(idx), _p(out),
                _p(ln["local"]), _p(ln["target"]), _p(ws), _p(ln["grad"]), _p(loss), _p(ln["exp_avg"]), _p(ln["exp_avg_sq"]), _p(ln["step"]))

    def single_step(self, g, ring_size, batch, ws, loss, out, idx=None):
        return self.L.mn_dqn_train_step(*self._single_args(g, ring_size, idx is None, idx, out, ws, loss), batch, *HYPER, _stream(self.torch))

    def single_steps(self, g, ring_size, batch, K, ws, losses, out, idx=None):
        return self.L.mn_dqn_train_steps(*self._single_args(g, ring_size, idx is None, idx, out, ws, losses), batch, K, *HYPER, _stream(self.torch))

    # ---- the three ways to run K steps of every learner from the snapshot; each returns (head bytes, losses [G][K], rows [G][K][batch]) ----------------
    def by_single_launches(self, ring_size, batch, K, idx=None):
        torch = self.torch
        self.restore()
        ws, loss = self.single_ws(batch), torch.zeros(1, device=DEV)
        losses, rows = torch.zeros((self.G, K), device=DEV), torch.zeros((self.G, K, batch), dtype=torch.int64, device=DEV)
        for g in range(self.G):
            for k in range(K):
                assert self.single_step(g, ring_size, batch, ws, loss, rows[g, k], None if idx is None else idx[g, k]) == 0
                losses[g, k] = loss[0]
        torch.cuda.synchronize()
        return self.head(), losses.cpu(), rows.cpu()

    def by_single_multi_calls(self, ring_size, batch, K, idx=None):
        torch = self.torch
        self.restore()
        ws = torch.zeros(self.L.mn_dqn_train_steps_workspace_floats(batch, K), device=DEV)
        losses, rows = torch.zeros((self.G, K), device=DEV), torch.zeros((self.G, K, batch), dtype=torch.int64, device=DEV)
        for g in range(self.G):
            assert self.single_steps(g, ring_size, batch, K, ws, losses[g], rows[g], None if idx is None else idx[g]) == 0
        torch.cuda.synchronize()
        return self.head(), losses.cpu(), rows.cpu()

    def group_step(self, ring_size, batch, losses, rows, idx=None, ws=None, handle=None):
        return self.L.mn_dqn_group_train_step(handle or self.handle, ring_size, _p(idx), _p(rows), _p(self.ws if ws is None else ws), _p(losses), batch,
                                              *HYPER, _stream(self.torch))

    def group_steps(self, ring_size, batch, K, losses, rows, idx=None, ws=None, handle=None):
        return self.L.mn_dqn_group_train_steps(handle or self.handle, ring_size, _p(idx), _p(rows), _p(self.ws if ws is None else ws), _p(losses), batch, K,
                                               *HYPER, _stream(self.torch))

    def by_group_launches(self, ring_size, batch, K, idx=None):
        torch = self.torch
        self.restore()
        losses, rows = torch.zeros((K, self.G), device=DEV), torch.zeros((K, self.G, batch), dtype=torch.int64, device=DEV)
        for k in range(K):
            assert self.group_step(ring_size, batch, losses[k], rows[k], None if idx is None else idx[:, k].contiguous()) == 0
            if k == 0:      # the first launch must already have moved every learner's parameters, or the comparison proves nothing
                assert all(self.moved(g) for g in range(self.G))
        torch.cuda.synchronize()
        assert self.guards_intact()
        return self.head(), losses.t().contiguous().cpu(), rows.transpose(0, 1).contiguous().cpu()

    def by_group_multi_calls(self, ring_size, batch, cuts, idx=None):
        torch = self.torch
        self.restore()
        losses, rows, k0 = [], [], 0
        for K in cuts:
            lo, ro = torch.zeros((self.G, K), device=DEV), torch.zeros((self.G, K, batch), dtype=torch.int64, device=DEV)
            assert self.group_steps(ring_size, batch, K, lo, ro, None if idx is None else idx[:, k0:k0 + K].contiguous()) == 0
            losses.append(lo)
            rows.append(ro)
            k0 += K
        torch.cuda.synchronize()
        assert self.guards_intact()
        return self.head(), torch.cat(losses, dim=1).cpu(), torch.cat(rows, dim=1).cpu()

    def same(self, got, want):
        """Bytes of every field of every learner (named, for the message), of the whole head (guards included), of the losses and the rows."""
        torch = self.torch
        per = len(FIELDS) * (GUARD + VEC) + 2 * (GUARD + 4)
        for g in range(self.G):
            o = g * per
            for f in FIELDS:
                o += GUARD
                assert torch.equal(got[0][o:o + P_TOTAL], want[0][o:o + P_TOTAL]), (g, f)
                o += VEC
            assert torch.equal(got[0][o:o + per - len(FIELDS) * (GUARD + VEC)], want[0][o:o + per - len(FIELDS) * (GUARD + VEC)]), (g, "step / draw state")
        assert torch.equal(got[0], want[0])
        assert got[1].shape == want[1].shape and torch.equal(got[1].view(torch.int32), want[1].view(torch.int32)), "losses"
        assert got[2].shape == want[2].shape and torch.equal(got[2], want[2]), "rows"


def _ws_floats(L, G, shapes):
    """Floats of a grouped workspace that serves every (batch, n_steps) of `shapes` (n_steps 0: the single step)."""
    r4 = lambda n: (n + 3) // 4 * 4
    return G * max(r4(L.mn_dqn_train_steps_workspace_floats(b, k) if k else L.mn_dqn_train_workspace_floats(b)) for b, k in shapes)


@pytest.fixture(scope="module")
def three(torch, L, rings, base_params):
    return Arena(torch, L, 3, rings, base_params, _ws_floats(L, 3, [(48, 0), (32, 5), (32, 3), (32, 2)]))


def _rows(torch, G, K, batch, seed):
    """Given rows with a repeat inside a batch and the same row in two steps and two learners."""
    gen = torch.Generator(device=DEV).manual_seed(seed)
    idx = torch.randint(0, RING, (G, K, batch), device=DEV, generator=gen)
    idx[0, 0, 1] = idx[0, 0, 0]
    idx[G - 1, K - 1, 0] = idx[0, 0, 0]
    return idx


@pytest.mark.parametrize("draw", [True, False], ids=["draw", "rows"])
@pytest.mark.parametrize("batch", [32, 20, 48])
def test_grouped_step_equals_single_launches(torch, three, batch, draw):
    """Batch 32: two full tiles; 20: 16 + 4, a partial tile; 48: three tiles.  Four consecutive grouped launches against four single launches per learner.
    In draw mode the ring size is no power of two."""
    ring_size = 1000 if draw else RING
    idx = None if draw else _rows(torch, 3, 4, batch, 31)
    want = three.by_single_launches(ring_size, batch, 4, idx)
    got = three.by_group_launches(ring_size, batch, 4, idx)
    three.same(got, want)
    for g, ln in enumerate(three.learners):
        assert int(ln["step"].item()) == 3 + 4
        assert ln["rng"].tolist() == [99991 + 7 * g, 17 + g + (4 if draw else 0)]
    if draw:
        assert int(got[2].max()) < 1000 and not torch.equal(got[2][0], got[2][1])      # each learner drew its own rows
    else:
        assert torch.equal(got[2], idx.cpu())


@pytest.mark.parametrize("draw", [True, False], ids=["draw", "rows"])
@pytest.mark.parametrize("batch", [32, 20])
def test_grouped_multi_step_call(torch, three, batch, draw):
    """K = 5 in one grouped call against five single launches per learner AND against mn_dqn_train_steps per learner; cut into 2 + 3 it is the same."""
    idx = None if draw else _rows(torch, 3, 5, batch, 37)
    loop = three.by_single_launches(RING, batch, 5, idx)
    assert not torch.equal(loop[0], three.snap[:three.ws_off].cpu())
    multi = three.by_single_multi_calls(RING, batch, 5, idx)
    got = three.by_group_multi_calls(RING, batch, [5], idx)
    three.same(got, loop)
    three.same(got, multi)
    three.same(three.by_group_multi_calls(RING, batch, [2, 3], idx), got)
    for g, ln in enumerate(three.learners):
        assert int(ln["step"].item()) == 3 + 5 and ln["rng"].tolist() == [99991 + 7 * g, 17 + g + (5 if draw else 0)]


def test_group_of_one(torch, L, rings, base_params):
    one = Arena(torch, L, 1, rings, base_params, _ws_floats(L, 1, [(32, 0), (32, 3)]))
    want = one.by_single_launches(RING, 32, 3)
    one.same(one.by_group_launches(RING, 32, 3), want)
    one.same(one.by_group_multi_calls(RING, 32, [3]), want)
    one.same(one.by_single_multi_calls(RING, 32, 3), want)
    assert L.mn_dqn_group_destroy(one.handle) == 0


def test_the_limit_of_64_learners(torch, L, rings, base_params):
    """One grouped step and one K = 2 multi-step call at G = 64, batch 32: every learner equals its own single calls.  (The learners share the three
    rings; their written buffers are their own.)"""
    big = Arena(torch, L, 64, rings, base_params, _ws_floats(L, 64, [(32, 0), (32, 2)]))
    big.same(big.by_group_launches(1000, 32, 1), big.by_single_launches(1000, 32, 1))
    want = big.by_single_launches(RING, 32, 2)
    got = big.by_group_multi_calls(RING, 32, [2])
    big.same(got, want)
    assert len({tuple(r.tolist()) for r in got[2][:, 0]}) == 64      # 64 draw states, 64 different batches
    assert L.mn_dqn_group_destroy(big.handle) == 0


def test_no_learner_writes_outside_its_own_buffers(torch, L, three):
    """The shapes of the two cases above once more, looking only at the guard words: between every two buffers of the arena, in the two spare words of
    every vector's slot and behind the last workspace slice (whose stride is the largest here: batch 48)."""
    r4 = lambda n: (n + 3) // 4 * 4
    assert three.ws.numel() == 3 * r4(L.mn_dqn_train_workspace_floats(48))      # the guard sits right behind the last slice of the largest shape
    for batch in (32, 20, 48):
        three.by_group_launches(RING, batch, 2)
        assert three.guards_intact(), batch
        three.by_group_launches(RING, batch, 2, _rows(torch, 3, 2, batch, 41))
        assert three.guards_intact(), batch
    for batch in (32, 20):
        three.by_group_multi_calls(RING, batch, [5])
        assert three.guards_intact(), batch
    # (and the check can fail: a word written over a guard is seen)
    three.mem[three.ws_off - 1] = 0
    assert not three.guards_intact()
    three.restore()
    assert three.guards_intact()


def _load_ring(ag, ring):
    m = ag.memory
    n = ring[0].shape[0]
    for dst, src in zip((m.states, m.actions, m.rewards, m.next_states, m.dones), ring):
        dst[:n].copy_(src)
    m.size, m.ptr = n, n % m.capacity


def _bits(t):
    import torch
    return t.detach().contiguous().view(-1).view({4: torch.int32, 8: torch.int64}[t.element_size()]).cpu()


def test_group_and_single_calls_interleave(torch, rings):
    """Group step, learner 1 alone, group multi-step call -- against the same sequence done with single calls only."""
    from distributional_rl_navigation_amd.dqn.group_train import LearnerGroup
    grouped, alone = ([_agent(torch, seed=21 + g) for g in range(3)] for _ in range(2))
    for ags in (grouped, alone):
        for ag, ring in zip(ags, rings):
            _load_ring(ag, ring)
    obs = rings[0][0][:64].contiguous()
    for ag in grouped:
        ag.policy.act_batch(obs)      # the act image exists BEFORE the steps: a stale one would act on these weights
    group = LearnerGroup(grouped)
    l0 = group.train()
    l1 = grouped[1].train()
    l2 = group.train_many(4)
    assert l0.shape == (3,) and l2.shape == (3, 4) and group.last_idx.shape == (3, 4, 32)
    w0 = torch.stack([ag.train() for ag in alone])
    w1 = alone[1].train()
    w2 = torch.stack([torch.stack([ag.train() for _ in range(4)]) for ag in alone])
    assert torch.equal(_bits(l0), _bits(w0)) and torch.equal(_bits(l1), _bits(w1)) and torch.equal(_bits(l2), _bits(w2))
    for g, (a, b) in enumerate(zip(grouped, alone)):
        fa, fb = a._fused, b._fused
        for name in ("local", "target", "exp_avg", "exp_avg_sq", "grad", "step_dev", "rng_state"):
            assert torch.equal(_bits(getattr(fa, name)), _bits(getattr(fb, name))), (g, name)
        assert a.n_updates == b.n_updates == (6 if g == 1 else 5) and a._train_path == "hip"
        assert torch.equal(a.act_batch(obs, 0), b.act_batch(obs, 0))
        with torch.no_grad():
            assert torch.equal(a.act_batch(obs, 0).long(), a.q_net(obs).argmax(dim=1))      # the act image follows the grouped steps
    group.sync_target()
    for a in grouped:
        assert torch.equal(a._fused.target, a._fused.local)
    # the eager step afterwards continues each agent's one Adam state
    for g, (a, b) in enumerate(zip(grouped, alone)):
        for ag in (a, b):
            m = ag.memory
            rows = torch.arange(32, device=DEV)
            ag.train(tuple(t[rows] for t in (m.states, m.actions, m.rewards, m.next_states, m.dones)))
        pa, pb = next(iter(a.q_net.parameters())), next(iter(b.q_net.parameters()))
        assert float(a.optimizer.state[pa]["step"]) == float(b.optimizer.state[pb]["step"]) == (7 if g == 1 else 6)
        assert a.n_updates == b.n_updates
    # unequal ring fills are refused at the call, in words
    grouped[2].memory.size = 1000
    with pytest.raises(ValueError, match="equally full"):
        group.train()
    group.close()


def test_arguments(torch, L, three):
    from distributional_rl_navigation_amd import _capi
    three.restore()
    torch.cuda.synchronize()
    assert isinstance(three.create(n=0), int) and three.create(n=0) == INVALID
    assert three.create(three.table(65), n=65) == INVALID
    tab = three.table()
    tab[1].params_local = None
    assert three.create(tab) == INVALID
    tab = three.table()
    tab[2].params_local = tab[0].params_local
    assert three.create(tab) == INVALID
    tab = three.table()
    tab[1].exp_avg = tab[0].exp_avg
    assert three.create(tab) == INVALID
    tab = three.table()
    tab[1].grad = tab[0].exp_avg_sq + 4 * (P_TOTAL // 2)      # overlapping by half a vector
    assert three.create(tab) == INVALID
    tab = three.table()
    tab[1].step = tab[0].step
    assert three.create(tab) == INVALID
    tab = three.table()
    tab[1].rng_state = None      # legal: a group that is only ever called with rows
    rows_only = three.create(tab)
    assert not isinstance(rows_only, int)

    losses, out = torch.zeros((3, 4), device=DEV), torch.zeros((3, 4, 64), dtype=torch.int64, device=DEV)
    idx = torch.zeros((3, 4, 64), dtype=torch.int64, device=DEV)
    off = three.ws[1:]      # 4 bytes past a 16-byte boundary
    assert three.group_step(RING, 32, losses, out, handle=rows_only) == INVALID and three.group_steps(RING, 32, 4, losses, out, handle=rows_only) == INVALID
    assert three.group_step(RING, 0, losses, out) == INVALID and three.group_step(RING, 257, losses, out) == INVALID
    assert three.group_step(RING, 257, losses, out, idx) == INVALID
    assert three.group_steps(RING, 33, 4, losses, out) == INVALID and three.group_steps(RING, 33, 4, losses, out, idx) == INVALID
    assert three.group_steps(RING, 32, 0, losses, out) == INVALID and three.group_steps(RING, 32, 1025, losses, out) == INVALID
    assert three.group_step(31, 32, losses, out) == INVALID and three.group_steps(31, 32, 4, losses, out) == INVALID
    assert three.group_step(RING, 32, losses, out, ws=off) == INVALID and three.group_steps(RING, 32, 4, losses, out, ws=off) == INVALID
    assert L.mn_dqn_group_train_step(None, RING, None, None, _p(three.ws), _p(losses), 32, *HYPER, _stream(torch)) == INVALID
    assert L.mn_dqn_group_destroy(None) == INVALID
    torch.cuda.synchronize()
    assert torch.equal(three.mem, three.snap)      # nothing was launched
    # the same buffers are fine with legal arguments, and a rows-only group runs with rows
    assert three.group_step(RING, 32, losses, out) == 0 and three.group_steps(RING, 32, 4, losses, out) == 0
    assert three.group_step(RING, 32, losses, out, idx[:, 0, :32].contiguous(), handle=rows_only) == 0
    torch.cuda.synchronize()
    assert all(three.moved(g) for g in range(3)) and three.guards_intact()
    assert three.learners[1]["rng"].tolist() == [99991 + 7, 17 + 1 + 5]      # 1 + 4 draws; the rows-only call left it alone
    assert L.mn_dqn_group_destroy(rows_only) == 0
    three.restore()


def _nested_equal(a, b):
    """Equality of ragged nests (object arrays / lists of arrays), leaf by leaf."""
    if isinstance(a, (list, tuple)) or (isinstance(a, np.ndarray) and a.dtype == object):
        return isinstance(b, (list, tuple, np.ndarray)) and len(a) == len(b) and all(_nested_equal(x, y) for x, y in zip(a, b))
    return np.array_equal(np.asarray(a), np.asarray(b))


@pytest.mark.parametrize("per_call", [1, "multi"])
def test_driver_files_equal_the_sequential_runs(torch, tmp_path, per_call):
    """A toy reference-budget run: seeds 3 and 4 through run_trials_together, and each through run_trial."""
    from distributional_rl_navigation_amd.train_dqn import run_trial, run_trials_together
    from distributional_rl_navigation_amd.train_iqn import create_eval_configs
    TOTAL, N = 2_000, 16
    REFERENCE = dict(learning_starts=400, target_update_interval=400)
    cfg = create_eval_configs(DEV)
    eval_config = {k: cfg[k] for k in list(cfg)[:3]}      # three evaluation worlds
    common = dict(verbose=False, env_budget="reference", reference=REFERENCE, eval_config=eval_config, max_eval_steps=60, train_steps_per_call=per_call)
    params = lambda seed, name: dict(agent="DQN", seed=seed, total_timesteps=TOTAL, eval_freq=400, save_dir=str(tmp_path), training_time=name)
    seen = []
    dirs, agents = run_trials_together(DEV, [params(s, "together") for s in (3, 4)], N, return_agents=True,
                                       on_step=[lambda it, d, s=s: seen.append((s, it, float(d["last"]["eps"]))) for s in (3, 4)], **common)
    assert [os.path.basename(d) for d in dirs] == ["seed_3", "seed_4"] and len(seen) == 2 * (TOTAL // N) and seen[0][:2] == (3, 0) and seen[1][:2] == (4, 0)
    for seed, d, agent in zip((3, 4), dirs, agents):
        assert agent.n_updates == 1_600
        d1, alone = run_trial(DEV, params(seed, "alone"), N, return_agent=True, **common)
        assert alone.n_updates == 1_600
        assert torch.equal(_bits(agent._fused.local), _bits(alone._fused.local)) and torch.equal(_bits(agent._fused.target), _bits(alone._fused.target))
        assert not torch.equal(agent._fused.local, agents[0 if seed == 4 else 1]._fused.local)
        assert sorted(os.listdir(d)) == sorted(os.listdir(d1))
        for f in ("evaluations.npz", "training_log.npz"):
            za, zb = (np.load(os.path.join(x, f), allow_pickle=True) for x in (d, d1))
            assert sorted(za.files) == sorted(zb.files) and len(za.files) > 0
            for k in za.files:
                if za[k].dtype == object:
                    assert _nested_equal(za[k], zb[k]), (f, k)      # (actions: per evaluation point a list of per-world arrays of different lengths)
                else:
                    assert np.array_equal(za[k], zb[k], equal_nan=za[k].dtype.kind == "f"), (f, k)
