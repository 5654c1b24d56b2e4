"""Many IQN learners per launch (`mn_iqn_group_train_step`, csrc/iqn_train.hip; iqn/group_train.py; `train_iqn.run_trials_together`) on the GPU: every
learner of a grouped step is BIT for bit what the single calls leave from the same state -- loss, parameters, clipped gradient, both moments, step counter,
generator state, the drawn rows and taus -- at one, three and sixteen workgroups per learner, in draw mode and with given batches, against the default single
form and the three-launch form, for a group of one and at the limit of 64; nothing is written outside a learner's own buffers (guard words); group and single
calls interleave on one agent; the argument checks; the driver's files.

The reference of every comparison is the single call (`agent.train_from_memory()`, `FusedTrainer.step`, `mn_iqn_train_step`), never a grouped call's own
earlier output.  Rings have 2 048 rows from a 256-env, 8-step rollout of the HIP env; in draw mode 1 000 of them count, so the ring size is no power of two."""
import ctypes as C
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
RING, FILL = 2048, 1000
P_TOTAL, P_SLOT = 35785, 35788      # a vector's slot in the arena: its 35 785 floats and three spare words
NQ = 8
GUARD = 4
SENT = 0x7FC0DEAD    # (a NaN with a payload, as float)
INVALID = -1         # MN_ERR_INVALID
LR, GAMMA = 1e-4, 0.99
STATE = ("loss", "local", "target", "grad", "exp_avg", "exp_avg_sq", "step_dev", "rng_state")


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


def _agent(torch, batch=32, seed=3):
    from distributional_rl_navigation_amd.iqn.agent import IQNAgent
    return IQNAgent(26, 9, BATCH_SIZE=batch, BUFFER_SIZE=RING, device=DEV, seed=seed)


@pytest.fixture(scope="module")
def rings(torch):
    """Three replay rings of 2 048 rows, each from its own 256-env, 8-step rollout of the HIP env (random actions, auto-reset), computed once and never
    written: (states, actions, rewards, next_states, dones)."""
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


def _bits(t):
    import torch
    return t.detach().contiguous().view(-1).view({4: torch.int32, 8: torch.int64}[t.element_size()]).cpu()


def _use_ring(ag, ring, fill, own=False):
    """The agent's replay memory IS `ring` (shared, read-only for the gradient step), or -- `own` -- a copy of it; `fill` rows count."""
    m = ag.memory
    m.states, m.actions, m.rewards, m.next_states, m.dones = (t.clone() for t in ring) if own else ring
    m.size, m.ptr = fill, fill % m.capacity
    m.version += 1


def _learners(torch, rings, G, batch, fill, own=False, warm=2):
    """G agents on the three rings, each with networks of its own seed, a target network unlike the local one and -- `warm` single steps -- a non-zero Adam
    state, a moved generator and a batch staged in its workspace.  Deterministic: two calls give two equal sets."""
    ags = []
    for g in range(G):
        ag = _agent(torch, batch, seed=21 + g)
        _use_ring(ag, rings[g % len(rings)], fill, own)
        ft = ag._fused_trainer()
        ft.target.copy_(ft.local * 1.05 + 0.01)
        for _ in range(warm):
            ag.train_from_memory()
        ags.append(ag)
    return ags


def _state(ag, batch=None):
    ft = ag._fused
    out = {k: _bits(getattr(ft, k)) for k in STATE}
    if batch is not None:
        out["idx"], out["taus"] = _bits(ft._idx[batch]), _bits(ft._taus[batch])
    return out


def _same(torch, got, want, who=""):
    assert got.keys() == want.keys()
    for k in got:
        assert torch.equal(got[k], want[k]), (who, k)


def _ring5(ag):
    m = ag.memory
    return (m.states, m.actions, m.rewards, m.next_states, m.dones)


def _given(torch, G, K, batch, seed):
    """Given batches: rows with a repeat inside a batch and the same row in two learners, injected taus."""
    gen = torch.Generator(device=DEV).manual_seed(seed)
    idx = torch.randint(0, RING, (K, G, batch), device=DEV, generator=gen)
    idx[:, 0, 1] = idx[:, 0, 0]
    idx[:, G - 1, 0] = idx[:, 0, 0]
    tt = torch.rand((K, G, batch, NQ), device=DEV, generator=gen)
    tl = torch.rand((K, G, batch, NQ), device=DEV, generator=gen)
    return idx, tt, tl


def _compare(torch, rings, G, batch, K, draw, alone_setup=None):
    """K grouped steps of G learners against K single steps per learner, from equal states; the losses of every step, the whole state at the end."""
    from distributional_rl_navigation_amd.iqn.group_train import LearnerGroup
    fill = FILL if draw else RING
    grouped, alone = _learners(torch, rings, G, batch, fill), _learners(torch, rings, G, batch, fill)
    for g in range(G):      # the two sets start equal, and the warm-up has moved them
        _same(torch, _state(grouped[g], batch), _state(alone[g], batch), g)
        assert int(grouped[g]._fused.step_dev.item()) == 2
    for ag in alone:
        (alone_setup or (lambda a: None))(ag)
    group = LearnerGroup(grouped)
    assert len(group) == G
    before = [_state(ag)["local"] for ag in grouped]
    given = None if draw else _given(torch, G, K, batch, 31)
    got, want = [], []
    for k in range(K):
        got.append(group.train() if draw else group.train(given[0][k], given[1][k], given[2][k]))
        if k == 0:      # the first step must already have moved every learner's parameters, or the comparison proves nothing
            assert all(not torch.equal(_state(ag)["local"], b) for ag, b in zip(grouped, before))
    for k in range(K):
        if draw:
            want.append(torch.stack([ag.train_from_memory().clone() for ag in alone]))
        else:
            want.append(torch.stack([ag._fused.step(_ring5(ag), given[0][k][g], given[1][k][g], given[2][k][g]).clone() for g, ag in enumerate(alone)]))
    torch.cuda.synchronize()
    assert torch.equal(_bits(torch.stack(got)), _bits(torch.stack(want))), "losses"
    assert bool(torch.isfinite(torch.stack(got)).all())
    for g in range(G):
        _same(torch, _state(grouped[g], batch if draw else None), _state(alone[g], batch if draw else None), g)
        assert int(grouped[g]._fused.step_dev.item()) == 2 + K
        assert grouped[g]._fused.rng_state.tolist()[1] == 2 + (K if draw else 0)
        assert grouped[g]._train_path == "hip" and grouped[g]._fused._staged_key is None
        if draw:
            assert grouped[g].grad_steps == alone[g].grad_steps == 2 + K
            assert int(grouped[g]._fused._idx[batch].max()) < FILL
        assert grouped[g]._fused.timeouts() == 0 and alone[g]._fused.timeouts() == 0
    if draw and G > 1:
        assert not torch.equal(grouped[0]._fused._idx[batch], grouped[1]._fused._idx[batch])      # each learner drew its own rows
    group.close()
    return grouped, alone


@pytest.mark.parametrize("draw", [True, False], ids=["draw", "given"])
@pytest.mark.parametrize("batch", [32, 6, 2])
def test_grouped_step_equals_single_steps(torch, rings, batch, draw):
    """Batch 32: 16 workgroups per learner; 6: three (not a multiple of 8, not a shape of the fused one-launch form); 2: a single workgroup per learner.
    Four consecutive grouped steps against four single steps (default form) per learner."""
    _compare(torch, rings, 3, batch, 4, draw)


def test_grouped_step_equals_the_three_launch_form(torch, rings):
    def three_launches(ag):
        ag.two_launch_step = False
    _, alone = _compare(torch, rings, 3, 32, 4, True, alone_setup=three_launches)
    assert alone[0]._fused.launches_per_step() == 3


def test_group_of_one(torch, rings):
    _compare(torch, rings, 1, 32, 3, True)


@pytest.mark.parametrize("batch", [32, 6])
def test_the_limit_of_64_learners(torch, rings, batch):
    """One grouped step at G = 64: 1 024 (batch 32) forward / backward workgroups of 97 KB of LDS in one launch, more than the device holds at once.  The
    learners share the three rings; their written buffers are their own.  Every learner equals its single call."""
    grouped, _ = _compare(torch, rings, 64, batch, 1, True)
    assert len({tuple(ag._fused._idx[batch].tolist()) for ag in grouped}) == 64      # 64 generator states, 64 different batches


def test_more_than_64_agents_are_refused(torch, rings):
    from distributional_rl_navigation_amd.iqn.group_train import LearnerGroup
    ag = _learners(torch, rings, 1, 32, FILL, warm=0)[0]
    with pytest.raises(ValueError, match="1..64"):
        LearnerGroup([ag] * 65)


def test_group_and_single_calls_interleave(torch, rings):
    """group step, learner 1 alone (staging on), group step, a ring write, learner 0 alone twice (the second from its staged batch), group step -- against
    the same sequence with single calls only, after every step."""
    from distributional_rl_navigation_amd.iqn.group_train import LearnerGroup
    grouped, alone = (_learners(torch, rings, 3, 32, FILL, own=True) for _ in range(2))
    obs = rings[0][0][:64].contiguous()
    for ag in grouped + alone:
        ag.act_batch(obs, 0.0)      # the act image exists BEFORE the steps: a stale one would act on these weights
    group = LearnerGroup(grouped)
    staged_used = []

    def check(tag):
        torch.cuda.synchronize()
        for g in range(3):
            _same(torch, _state(grouped[g], 32), _state(alone[g], 32), (tag, g))
            assert grouped[g].grad_steps == alone[g].grad_steps, (tag, g)
            assert grouped[g]._fused.timeouts() == 0 and alone[g]._fused.timeouts() == 0

    def ring_write(ags):
        for ag in ags:      # 16 rows of ring 1 appended to every ring: the fill moves to 1 016, the version with it
            src = rings[1]
            ag.memory.add_batch(src[0][:16], src[1][:16].view(-1), src[2][:16].view(-1), src[3][:16], src[4][:16].view(-1))

    def single(ag):
        ft = ag._fused
        m = ag.memory
        key = (m.states.data_ptr(), int(m.version), int(m.size), 32, ft._ws.data_ptr())
        staged_used.append(key == ft._staged_key)
        return ag.train_from_memory().clone()

    l = [group.train()]
    w = [torch.stack([single(a) for a in alone])]
    check("group step 1")
    l.append(single(grouped[1])); w.append(single(alone[1]))
    assert staged_used[-2:] == [False, True]      # behind a grouped step nothing is staged; behind its own single step the batch is
    check("learner 1 alone")
    l.append(group.train()); w.append(torch.stack([single(a) for a in alone]))
    check("group step 2")
    ring_write(grouped); ring_write(alone)
    assert grouped[0].memory.size == FILL + 16
    for _ in range(2):
        l.append(single(grouped[0])); w.append(single(alone[0]))
    assert staged_used[-4:] == [False, False, True, True]      # the first single step behind the group step draws in its launch, the second starts staged
    check("learner 0 alone twice")
    l.append(group.train()); w.append(torch.stack([single(a) for a in alone]))
    check("group step 3")
    for a, b in zip(l, w):
        assert torch.equal(_bits(a), _bits(b))
    assert [ag.grad_steps for ag in grouped] == [2 + 5, 2 + 4, 2 + 3]
    for a, b in zip(grouped, alone):      # the act image follows the grouped steps
        assert torch.equal(a.act_batch(obs, 0.0), b.act_batch(obs, 0.0))
    # unequal ring fills are refused at the call, in words
    grouped[2].memory.size = 900
    with pytest.raises(ValueError, match="equally full"):
        group.train()
    group.close()


def test_target_copy_between_grouped_steps(torch, rings):
    from distributional_rl_navigation_amd.iqn.group_train import LearnerGroup
    grouped, alone = (_learners(torch, rings, 3, 32, FILL) for _ in range(2))
    group = LearnerGroup(grouped)
    l = [group.train_many(2)]
    group.sync_target()
    l.append(group.train_many(2))
    w = []
    for ag in alone:
        a = [ag.train_from_memory() for _ in range(2)][-1].clone()
        ag._sync_target()
        w.append((a, [ag.train_from_memory() for _ in range(2)][-1].clone()))
    torch.cuda.synchronize()
    for g in range(3):
        assert not torch.equal(grouped[g]._fused.target, grouped[g]._fused.local) and grouped[g]._last_sync_at == alone[g]._last_sync_at == 4
        _same(torch, _state(grouped[g], 32), _state(alone[g], 32), g)
        assert torch.equal(_bits(l[0][g]), _bits(w[g][0])) and torch.equal(_bits(l[1][g]), _bits(w[g][1]))
    group.close()


# ---- the C-ABI on raw buffers: guards, arguments ------------------------------------------------------------------------------------------------------
def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _stream(torch):
    from distributional_rl_navigation_amd import _capi
    return _capi.stream_ptr(torch.device(DEV))


HYPER = (C.c_float(GAMMA), C.c_double(LR), C.c_double(0.9), C.c_double(0.999), C.c_double(1e-8), C.c_double(0.5))
VECS = ("local", "target", "grad", "exp_avg", "exp_avg_sq")


class Arena:
    """G learners as slices of ONE int32 allocation with guard words between all buffers: per learner five vectors (35 785 floats in a slot of 35 788),
    loss, step, generator state, the drawn rows and taus, and a workspace of exactly mn_iqn_train_workspace_floats(batch) floats."""

    def __init__(self, torch, L, G, batch, rings):
        self.torch, self.L, self.G, self.batch = torch, L, G, batch
        self.rings = [rings[g % len(rings)] for g in range(G)]
        self.ws_floats = int(L.mn_iqn_train_workspace_floats(batch))
        assert self.ws_floats > 0
        r4 = lambda n: (n + 3) // 4 * 4
        sizes = [(v, P_TOTAL, P_SLOT) for v in VECS] + [("loss", 1, 4), ("step", 1, 4), ("rng", 4, 4), ("idx", 2 * batch, r4(2 * batch)),
                                                          ("taus", 2 * batch * NQ, 2 * batch * NQ), ("ws", self.ws_floats, r4(self.ws_floats))]
        per = sum(GUARD + slot for _, _, slot in sizes)
        n = G * per + GUARD
        self.mem = torch.full((n,), SENT, dtype=torch.int32, device=DEV)
        assert self.mem.data_ptr() % 16 == 0
        self.guard = torch.ones(n, dtype=torch.bool, device=DEV)
        gen = torch.Generator(device=DEV).manual_seed(4321)
        base = [torch.cat([p.detach().reshape(-1) for p in net.parameters()]) for net in (_agent(torch, seed=11).qnetwork_local, _agent(torch, seed=12).qnetwork_local)]
        self.learners, o = [], 0
        for g in range(G):
            ln = {}
            for name, used, slot in sizes:
                o += GUARD
                ln[name] = self.mem[o:o + used]
                self.guard[o:o + used] = False
                o += slot
            for f in VECS:
                ln[f] = ln[f].view(torch.float32)
            ln["loss"], ln["ws"], ln["taus"], ln["rng"], ln["idx"] = (ln["loss"].view(torch.float32), ln["ws"].view(torch.float32), ln["taus"].view(torch.float32),
                                                                      ln["rng"].view(torch.int64), ln["idx"].view(torch.int64))
            for f, b in zip(("local", "target"), base):      # each learner its own networks, the target unlike the local one
                ln[f].copy_(b * (1 + 0.1 * torch.randn(P_TOTAL, device=DEV, generator=gen)))
            for f in ("grad", "exp_avg", "exp_avg_sq", "loss", "idx", "taus"):
                ln[f].zero_()
            ln["step"].zero_()
            ln["rng"].copy_(torch.tensor([99991 + 7 * g, 17 + g], dtype=torch.int64))
            assert ln["ws"].data_ptr() % 16 == 0
            assert L.mn_iqn_train_workspace_init(_p(ln["ws"]), batch, _stream(torch)) == 0
            self.learners.append(ln)
        assert o + GUARD == n
        torch.cuda.synchronize()
        self.snap = self.mem.clone()
        assert bool((self.snap[self.guard] == SENT).all()) and int(self.guard.sum()) >= GUARD * (11 * G + 1) + 3 * 5 * G
        self.handle = self.create()
        assert not isinstance(self.handle, int)

    def restore(self):
        self.mem.copy_(self.snap)

    def guards_intact(self):
        return bool((self.mem[self.guard] == SENT).all())

    def fields(self):
        """Everything but the workspaces (whose hand-off words differ between the launch forms), as bits."""
        return [{k: _bits(v) for k, v in ln.items() if k != "ws"} for ln in self.learners]

    def table(self, n=None):
        from distributional_rl_navigation_amd import _capi
        n = self.G if n is None else n
        tab = (_capi.MnIqnLearner * max(n, 1))()
        for g in range(n):
            ln, ring = self.learners[g % self.G], self.rings[g % self.G]
            row = tab[g]
            row.ring_states, row.ring_actions, row.ring_rewards, row.ring_next_states, row.ring_dones = (t.data_ptr() for t in ring)
            row.rng_state, row.params_local, row.params_target, row.workspace = ln["rng"].data_ptr(), ln["local"].data_ptr(), ln["target"].data_ptr(), ln["ws"].data_ptr()
            row.grad, row.loss, row.exp_avg, row.exp_avg_sq = ln["grad"].data_ptr(), ln["loss"].data_ptr(), ln["exp_avg"].data_ptr(), ln["exp_avg_sq"].data_ptr()
            row.step, row.idx_out, row.taus_out = ln["step"].data_ptr(), ln["idx"].data_ptr(), ln["taus"].data_ptr()
        return tab

    def create(self, tab=None, n=None, batch=None):
        h = C.c_void_p()
        rc = self.L.mn_iqn_group_create(self.table() if tab is None else tab, self.G if n is None else n, self.batch if batch is None else batch, C.byref(h))
        if rc:
            assert not h.value
            return rc
        return h

    def group_step(self, ring_size, idx=None, tt=None, tl=None, handle=None):
        return self.L.mn_iqn_group_train_step(handle or self.handle, ring_size, _p(idx), _p(tt), _p(tl), *HYPER, _stream(self.torch))

    def single_step(self, g, ring_size, idx=None, tt=None, tl=None):
        ln = self.learners[g]
        states, actions, rewards, next_states, dones = self.rings[g]
        draw = idx is None
        return self.L.mn_iqn_train_step(_p(states), _p(next_states), _p(actions), _p(rewards), _p(dones), ring_size, _p(ln["rng"]) if draw else None, _p(idx), _p(tt),
                                        _p(tl), _p(ln["idx"]), _p(ln["taus"]), _p(ln["local"]), _p(ln["target"]), _p(ln["ws"]), _p(ln["grad"]), _p(ln["loss"]),
                                        _p(ln["exp_avg"]), _p(ln["exp_avg_sq"]), _p(ln["step"]), self.batch, NQ, HYPER[0], 0, *HYPER[1:], _stream(self.torch))


@pytest.fixture(scope="module")
def arena(torch, L, rings):
    return Arena(torch, L, 3, 6, rings)


def test_no_learner_writes_outside_its_own_buffers(torch, L, arena):
    """Two drawn and one given grouped step on learners that live side by side in one arena: the guard words between all buffers, the three spare words of
    every vector's slot and the words behind every workspace (sized by mn_iqn_train_workspace_floats) are untouched; every learner moved, and equals the same
    steps through mn_iqn_train_step."""
    idx, tt, tl = (x[0].contiguous() for x in _given(torch, 3, 1, 6, 43))
    arena.restore()
    for k in range(2):
        assert arena.group_step(FILL) == 0
    assert arena.group_step(FILL, idx, tt, tl) == 0
    torch.cuda.synchronize()
    assert arena.guards_intact()
    got = arena.fields()
    snap_fields = None
    for g, ln in enumerate(arena.learners):
        assert int(ln["step"].item()) == 3 and ln["rng"].tolist() == [99991 + 7 * g, 17 + g + 2]
        assert bool(torch.isfinite(ln["local"]).all()) and bool(torch.isfinite(ln["loss"]).all())
    arena.restore()
    snap_fields = arena.fields()
    for g in range(3):
        for k in range(2):
            assert arena.single_step(g, FILL) == 0
        assert arena.single_step(g, FILL, idx[g].contiguous(), tt[g].contiguous(), tl[g].contiguous()) == 0
    torch.cuda.synchronize()
    assert arena.guards_intact()
    want = arena.fields()
    for g in range(3):
        _same(torch, got[g], want[g], g)
        assert not torch.equal(got[g]["local"], snap_fields[g]["local"]) and torch.equal(got[g]["target"], snap_fields[g]["target"])
    # (and the check can fail: a word written over a guard is seen)
    arena.mem[GUARD - 1] = 0
    assert not arena.guards_intact()
    arena.restore()
    assert arena.guards_intact()


def test_arguments(torch, L, arena):
    arena.restore()
    torch.cuda.synchronize()
    idx, tt, tl = (x[0].contiguous() for x in _given(torch, 3, 1, 6, 47))
    assert arena.create(n=0) == INVALID and arena.create(arena.table(65), n=65) == INVALID
    assert arena.create(batch=7) == INVALID and arena.create(batch=0) == INVALID and arena.create(batch=1026) == INVALID
    tab = arena.table()
    tab[1].params_local = None
    assert arena.create(tab) == INVALID
    tab = arena.table()
    tab[1].workspace = None
    assert arena.create(tab) == INVALID
    tab = arena.table()
    tab[2].params_local = tab[0].params_local      # two learners sharing their parameters
    assert arena.create(tab) == INVALID
    tab = arena.table()
    tab[1].params_target = tab[0].params_local      # one's target network is what another writes
    assert arena.create(tab) == INVALID
    tab = arena.table()
    tab[1].workspace = tab[0].workspace
    assert arena.create(tab) == INVALID
    # one's gradient overlapping another's first moment by ONE float (addresses only: creation dereferences nothing)
    spare = torch.zeros(2 * P_TOTAL, device=DEV)
    tab = arena.table()
    tab[0].exp_avg, tab[1].grad = spare.data_ptr(), spare.data_ptr() + 4 * (P_TOTAL - 1)
    assert arena.create(tab) == INVALID
    tab[1].grad = spare.data_ptr() + 4 * P_TOTAL      # ... and side by side they are fine
    side_by_side = arena.create(tab)
    assert not isinstance(side_by_side, int) and L.mn_iqn_group_destroy(side_by_side) == 0
    tab = arena.table()
    tab[1].rng_state = tab[1].idx_out = tab[1].taus_out = None      # legal: a group that is only ever called with given batches
    given_only = arena.create(tab)
    assert not isinstance(given_only, int)

    assert L.mn_iqn_group_train_step(None, FILL, None, None, None, *HYPER, _stream(torch)) == INVALID
    assert arena.group_step(FILL, idx, None, None) == INVALID and arena.group_step(FILL, idx, tt, None) == INVALID
    assert arena.group_step(FILL, None, tt, tl) == INVALID and arena.group_step(FILL, None, None, tl) == INVALID
    assert arena.group_step(5) == INVALID and arena.group_step(0) == INVALID and arena.group_step(1 << 31) == INVALID      # ring_size < batch = 6; beyond 2^31 - 1
    assert arena.group_step(FILL, handle=given_only) == INVALID      # a learner without a generator state cannot draw
    assert L.mn_iqn_group_destroy(None) == INVALID
    torch.cuda.synchronize()
    assert torch.equal(arena.mem, arena.snap)      # nothing was launched
    # the same buffers are fine with legal arguments, and a given-only group runs with given batches
    assert arena.group_step(6) == 0 and arena.group_step(FILL, idx, tt, tl, handle=given_only) == 0
    torch.cuda.synchronize()
    assert arena.guards_intact()
    for g, ln in enumerate(arena.learners):
        assert int(ln["step"].item()) == 2 and ln["rng"].tolist() == [99991 + 7 * g, 17 + g + 1]      # one draw; the given call left the state alone
        assert int(ln["idx"].max()) < 6
    assert L.mn_iqn_group_destroy(given_only) == 0
    arena.restore()


# ---- the driver ---------------------------------------------------------------------------------------------------------------------------------------
def _nested_equal(a, b):
    """Equality of ragged nests (object arrays / lists of arrays), leaf by leaf; NaN equals NaN in float leaves."""
    if isinstance(a, (list, tuple)) or (isinstance(a, np.ndarray) and a.dtype == object):
        return isinstance(b, (list, tuple, np.ndarray)) and len(a) == len(b) and all(_nested_equal(x, y) for x, y in zip(a, b))
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and np.array_equal(a, b, equal_nan=a.dtype.kind == "f")


def _files_equal(torch, fa, fb):
    if fa.endswith(".npz"):
        za, zb = np.load(fa, allow_pickle=True), np.load(fb, allow_pickle=True)
        assert sorted(za.files) == sorted(zb.files) and len(za.files) > 0, fa
        for k in za.files:
            assert _nested_equal(za[k], zb[k]), (fa, k)
    elif fa.endswith(".pth"):
        sa, sb = torch.load(fa, map_location="cpu"), torch.load(fb, map_location="cpu")
        assert list(sa) == list(sb) and len(sa) > 0, fa
        for k in sa:
            assert torch.equal(_bits(sa[k]), _bits(sb[k])), (fa, k)
    elif fa.endswith(".json"):
        ja, jb = json.load(open(fa)), json.load(open(fb))
        for j in (ja, jb):      # (the two runs live in two directories: the one entry that has to differ)
            if isinstance(j, dict):
                j.pop("save_dir", None)
        assert ja == jb, fa
    else:
        assert open(fa, "rb").read() == open(fb, "rb").read(), fa


def test_driver_files_equal_the_sequential_runs(torch, tmp_path):
    """A toy reference-budget run (the sizes of tests/test_reference_budget_gpu.py): seeds 3 and 4 through run_trials_together, and each through run_trial."""
    from distributional_rl_navigation_amd.train_iqn import create_eval_configs, run_trial, run_trials_together
    TOTAL, N = 4_000, 16
    REFERENCE = dict(learning_starts=400, target_update_interval=400)
    cfg = create_eval_configs(DEV)
    eval_config = {k: cfg[k] for k in list(cfg)[:3]}      # three evaluation worlds
    common = dict(verbose=False, env_budget="reference", reference=REFERENCE, eval_config=eval_config, max_eval_steps=60, episode_log="full",
                  eval_deferred=dict(verbose=False))
    params = lambda seed, where: dict(agent="IQN", seed=seed, total_timesteps=TOTAL, eval_freq=400, save_dir=str(tmp_path / where), training_time="toy")
    seen = []
    dirs, agents = run_trials_together(DEV, [params(s, "together") for s in (3, 4)], N, return_agents=True,
                                       on_step=[lambda it, st, s=s: seen.append((s, it, float(st["last"]["eps"]))) for s in (3, 4)], **common)
    assert [os.path.basename(d) for d in dirs] == ["seed_3", "seed_4"]
    assert len(seen) == 2 * (TOTAL // N) and [x[:2] for x in seen[:4]] == [(3, 0), (4, 0), (3, 1), (4, 1)]      # per seed and step, in seed order
    assert not torch.equal(agents[0]._fused.local, agents[1]._fused.local)
    for seed, d, agent in zip((3, 4), dirs, agents):
        alone_seen = []
        d1, alone = run_trial(DEV, params(seed, "alone"), N, return_agent=True, on_step=lambda it, st: alone_seen.append((seed, it, float(st["last"]["eps"]))), **common)
        assert agent.grad_steps == alone.grad_steps == 900          # (4 000 - 400) / 4
        assert alone_seen == [x for x in seen if x[0] == seed]
        for name in ("local", "target", "exp_avg", "exp_avg_sq", "step_dev", "rng_state"):
            assert torch.equal(_bits(getattr(agent._fused, name)), _bits(getattr(alone._fused, name))), (seed, name)
        assert agent._fused.timeouts() == 0
        names = sorted(os.listdir(d))
        assert names == sorted(os.listdir(d1)) and "network_params.pth" in names and "greedy_evaluations.npz" in names and "training_episodes.npz" in names
        for f in names:
            assert os.path.isfile(os.path.join(d, f)), f
            _files_equal(torch, os.path.join(d, f), os.path.join(d1, f))
