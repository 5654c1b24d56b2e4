"""The stacked collect on the GPU (`mn_iqn_actor_group_*`, csrc/iqn_act.hip + iqn_act_group.h + replay.hip; iqn/group_collect.py; `train_iqn.run_trials_together(
stack_envs=True)`): every actor of a grouped act call is BIT for bit what `mn_iqn_act_rng` leaves for it alone from the same state -- actions, the [33 n] draws,
the generator state, the weight image with its constants -- in the plain form (eps = 0), the listed form (eps = 0.5) and the listed form with empty lists
(eps = 1), at n = 13 (33 n no multiple of 4, n no multiple of 8), 16 and 80; a stale image is rebuilt for the stale actor only; grouped and single calls
interleave; one actor and sixty-four; the grouped append against `mn_replay_append`; the argument checks; the driver's files.

The reference of every comparison is the single call on a twin of the actor (the same network, generator state and observations), never a grouped call's own
earlier output.  Every caller-owned buffer of an actor (draws, generator state, ring arrays) and the launch's action array lie in one arena with guard words
between them.  The buffers a context owns (image, constants, greedy-row list) are the library's own allocations and cannot be fenced from here: the image is
compared through `mn_iqn_export_image` (a device copy once the context is fresh), the constants through the image words they are folded into."""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 4            # words; every buffer starts on a 16-byte boundary
SENT = 0x7FC0DEAD    # (a NaN with a payload, as float)
INVALID = -1         # MN_ERR_INVALID


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


class Arena:
    """One int32 tensor of sentinel words; `take` carves typed buffers out of it with GUARD words on both sides."""

    def __init__(self, torch, words):
        self.torch = torch
        self.mem = torch.full((words,), SENT, dtype=torch.int32, device=DEV)
        self.used = torch.zeros(words, dtype=torch.bool, device=DEV)
        self.at = GUARD

    def take(self, shape, dtype):
        torch = self.torch
        words = int(np.prod(shape)) * torch.empty(0, dtype=dtype).element_size()
        words = (words + 3) // 4
        lo = self.at
        self.at = (lo + words + GUARD + 3) // 4 * 4
        assert self.at + GUARD <= self.mem.numel(), "arena too small"
        self.used[lo:lo + words] = True
        flat = self.mem[lo:lo + words]
        t = flat.view(torch.uint8)[:int(np.prod(shape)) * torch.empty(0, dtype=dtype).element_size()].view(dtype).view(*shape)
        return t

    def guards_intact(self):
        return bool((self.mem[~self.used] == SENT).all())


def _obs_of_stacked_env(torch, G, n, seed0=70):
    from distributional_rl_navigation_amd.marinenav_env.vec_env import VecMarineNavEnv, stacked_seeds
    env = VecMarineNavEnv(G * n, seeds=stacked_seeds(n, [seed0 + g for g in range(G)]), device=DEV)
    obs = env.reset().clone()
    env.close()
    return obs


class Actors:
    """G actors with distinct random networks, each with a twin (same weights, own context, own generator state and draws) for the single calls."""

    def __init__(self, torch, L, G, n, ring_cap=None, seed0=40, create=True):
        from distributional_rl_navigation_amd import _capi
        from distributional_rl_navigation_amd.iqn.fused_act import ActContext
        from distributional_rl_navigation_amd.iqn.model import ObsEncoder
        self.torch, self.L, self.G, self.n, self.cap = torch, L, G, n, ring_cap
        ring_words = 0 if ring_cap is None else ring_cap * (26 * 2 + 2 + 1 + 1) + 16 * GUARD
        self.arena = Arena(torch, G * (33 * n + 4 + 4 * GUARD + ring_words) + G * n + 16 * GUARD)
        # (ObsEncoder seeds torch's global generator: distinct seeds, distinct weights; a twin is built from the same seed)
        self.nets = [ObsEncoder(26, 9, seed=seed0 + g, device=DEV) for g in range(G)]
        self.twins = [ObsEncoder(26, 9, seed=seed0 + g, device=DEV) for g in range(G)]
        if G > 1:
            assert not torch.equal(self.nets[0].output_layer.weight, self.nets[1].output_layer.weight)
        assert torch.equal(self.nets[0].hidden_layer.weight, self.twins[0].hidden_layer.weight)
        self.ctx = [ActContext(DEV) for _ in range(G)]
        self.ctx_twin = [ActContext(DEV) for _ in range(G)]
        self.rng, self.draws, self.rings = [], [], []
        for g in range(G):
            st = self.arena.take((2,), torch.int64)
            st.copy_(torch.tensor([9001 + 13 * g, 5 + g], dtype=torch.int64))
            self.rng.append(st)
            self.draws.append(self.arena.take((33 * n,), torch.float32))
            if ring_cap is not None:
                self.rings.append(dict(states=self.arena.take((ring_cap, 26), torch.float32), next_states=self.arena.take((ring_cap, 26), torch.float32),
                                       actions=self.arena.take((ring_cap, 1), torch.int64), rewards=self.arena.take((ring_cap, 1), torch.float32),
                                       dones=self.arena.take((ring_cap, 1), torch.float32)))
                for k, t in self.rings[-1].items():      # (what was in the ring before: every slot the append leaves alone must keep it)
                    t.copy_(torch.arange(t.numel(), device=DEV).view(t.shape).to(t.dtype) + 1000 * g)
        self.actions = self.arena.take((G * n,), torch.int32)
        self.rng_twin = [s.clone() for s in self.rng]
        self.draws_twin = [torch.full((33 * n,), float("nan"), device=DEV) for _ in range(G)]
        self.actions_twin = torch.full((G * n,), -7, dtype=torch.int32, device=DEV)
        self.table = (_capi.MnIqnActor * G)()
        for g, row in enumerate(self.table):
            row.ctx, row.weights = self.ctx[g].h.value, C.cast(self.ctx[g].weights(self.nets[g]), C.c_void_p).value
            self.ctx_twin[g].weights(self.twins[g])
            row.rng_state, row.draws = self.rng[g].data_ptr(), self.draws[g].data_ptr()
            if ring_cap is not None:
                r = self.rings[g]
                row.ring_states, row.ring_next_states, row.ring_actions = r["states"].data_ptr(), r["next_states"].data_ptr(), r["actions"].data_ptr()
                row.ring_rewards, row.ring_dones = r["rewards"].data_ptr(), r["dones"].data_ptr()
        self.h = None
        if create:
            h = C.c_void_p()
            assert L.mn_iqn_actor_group_create(self.table, G, n, C.byref(h)) == 0
            self.h = h
        self.obs = _obs_of_stacked_env(torch, G, n)
        torch.cuda.synchronize()
        assert self.arena.guards_intact()

    def close(self):
        if self.h is not None:
            assert self.L.mn_iqn_actor_group_destroy(self.h) == 0
            self.h = None

    def act(self, eps, cvar=1.0, obs=None):
        return self.L.mn_iqn_actor_group_act(self.h, _p(self.obs if obs is None else obs), C.c_float(cvar), C.c_float(eps), _p(self.actions), _stream(self.torch))

    def act_twin(self, g, eps, cvar=1.0):
        """The single call on actor g's twin (its rows of the observations, its slice of the twin action array)."""
        n = self.n
        obs = self.obs[g * n:(g + 1) * n]
        rc = self.L.mn_iqn_act_rng(self.ctx_twin[g].h, _p(obs), self.ctx_twin[g]._ptrs, _p(self.rng_twin[g]), _p(self.draws_twin[g]), None, C.c_float(cvar),
                                   C.c_float(eps), _p(self.actions_twin[g * n:(g + 1) * n]), None, None, n, 32, _stream(self.torch))
        assert rc == 0

    def image(self, ctx, net):
        from distributional_rl_navigation_amd.iqn.fused_act import image_floats
        out = self.torch.zeros(image_floats(), dtype=self.torch.int32, device=DEV)
        assert self.L.mn_iqn_export_image(ctx.h, ctx._ptrs, _p(out), _stream(self.torch)) == 0
        return out

    def assert_equal_twins(self, where, groups=None):
        torch = self.torch
        torch.cuda.synchronize()
        assert self.arena.guards_intact(), where
        assert torch.equal(self.actions, self.actions_twin), where
        assert int(self.actions.min()) >= 0 and int(self.actions.max()) <= 8, where
        for g in (range(self.G) if groups is None else groups):
            assert torch.equal(_bits(self.draws[g]), _bits(self.draws_twin[g])), (where, g)
            assert self.rng[g].tolist() == self.rng_twin[g].tolist(), (where, g)
            assert torch.equal(self.image(self.ctx[g], self.nets[g]), self.image(self.ctx_twin[g], self.twins[g])), (where, g)


@pytest.mark.parametrize("n", [13, 16, 80])
def test_act_equals_the_single_calls(torch, L, n):
    a = Actors(torch, L, 3, n)
    calls = 0
    for cvar in (1.0, 0.25):
        for eps in (0.0, 0.5, 1.0):
            assert a.act(eps, cvar) == 0
            for g in range(3):
                a.act_twin(g, eps, cvar)
            calls += 1
            a.assert_equal_twins((n, eps, cvar))
            assert [int(s[1]) for s in a.rng] == [5 + g + calls for g in range(3)]
            if eps == 0.5:      # the call did explore on some rows and not on others
                u = torch.stack([d[32 * n:] for d in a.draws])
                assert bool((u > 0.5).any()) and bool((u <= 0.5).any())
            if cvar == 0.25:
                assert float(torch.stack([d[:32 * n] for d in a.draws]).max()) < 0.25
    assert not torch.equal(a.draws[0], a.draws[1])      # every actor its own stream, keyed by the row's index inside the group
    a.close()


def test_only_a_stale_image_is_rebuilt(torch, L):
    a = Actors(torch, L, 3, 16)
    assert a.act(0.5) == 0
    for g in range(3):
        a.act_twin(g, 0.5)
    a.assert_equal_twins("first call")
    before = [a.image(a.ctx[g], a.nets[g]) for g in range(3)]
    with torch.no_grad():
        for net in (a.nets[1], a.twins[1]):
            for prm in net.parameters():
                prm.mul_(1.25)
    assert L.mn_iqn_weights_changed(a.ctx[1].h) == 0 and L.mn_iqn_weights_changed(a.ctx_twin[1].h) == 0
    assert a.act(0.5) == 0
    for g in range(3):
        a.act_twin(g, 0.5)
    a.assert_equal_twins("after the weights of actor 1 changed")      # (actor 1's image = the single call's fresh rebuild)
    after = [a.image(a.ctx[g], a.nets[g]) for g in range(3)]
    assert torch.equal(after[0], before[0]) and torch.equal(after[2], before[2]) and not torch.equal(after[1], before[1])
    # nothing stale: a wrong rebuild would show, because the weights have moved under the image of actor 0 without a word to its context
    with torch.no_grad():
        a.nets[0].output_layer.bias.add_(1.0)
    assert a.act(0.0) == 0
    torch.cuda.synchronize()
    assert all(torch.equal(a.image(a.ctx[g], a.nets[g]), after[g]) for g in range(3))
    a.close()


def test_grouped_and_single_calls_interleave(torch, L):
    """Grouped, single on actor 2, grouped, single on actor 0 -- on the group's OWN contexts and generator states -- against the all-single sequence on the twins."""
    a = Actors(torch, L, 3, 16)
    n, eps = 16, 0.5
    single_out = torch.empty(n, dtype=torch.int32, device=DEV)

    def single(g):
        rc = L.mn_iqn_act_rng(a.ctx[g].h, _p(a.obs[g * n:(g + 1) * n]), a.ctx[g]._ptrs, _p(a.rng[g]), _p(a.draws[g]), None, C.c_float(1.0), C.c_float(eps),
                              _p(single_out), None, None, n, 32, _stream(torch))
        assert rc == 0
        a.act_twin(g, eps)
        torch.cuda.synchronize()
        assert torch.equal(single_out, a.actions_twin[g * n:(g + 1) * n]) and torch.equal(_bits(a.draws[g]), _bits(a.draws_twin[g]))

    def grouped():
        assert a.act(eps) == 0
        for g in range(3):
            a.act_twin(g, eps)
        a.assert_equal_twins("grouped")

    grouped(); single(2); grouped(); single(0)
    assert [int(s[1]) - (5 + g) for g, s in enumerate(a.rng)] == [3, 2, 3]
    assert [s.tolist() for s in a.rng] == [s.tolist() for s in a.rng_twin]
    # a stale context is rebuilt by whichever call comes first
    L.mn_iqn_weights_changed(a.ctx[2].h); L.mn_iqn_weights_changed(a.ctx_twin[2].h)
    single(2); grouped()
    a.close()


@pytest.mark.parametrize("G,n", [(1, 13), (64, 8)])
def test_one_actor_and_sixty_four(torch, L, G, n):
    a = Actors(torch, L, G, n)
    for eps in (0.5, 0.0):
        assert a.act(eps) == 0
        for g in range(G):
            a.act_twin(g, eps)
        a.assert_equal_twins((G, eps), groups=range(G) if G == 1 else (0, 31, 63))
        for g in range(G):
            assert torch.equal(_bits(a.draws[g]), _bits(a.draws_twin[g])) and a.rng[g].tolist() == a.rng_twin[g].tolist(), g
    a.close()
    if G == 64:      # one more than the limit
        from distributional_rl_navigation_amd import _capi
        table = (_capi.MnIqnActor * 65)()
        for i in range(65):
            C.memmove(C.byref(table[i]), C.byref(a.table[i % 64]), C.sizeof(_capi.MnIqnActor))
        h = C.c_void_p()
        assert L.mn_iqn_actor_group_create(table, 65, n, C.byref(h)) == INVALID and not h.value


def test_greedy_rows_off_gives_the_same_actions(torch, L):
    a = Actors(torch, L, 3, 16)
    for c in a.ctx:
        assert L.mn_iqn_set_greedy_rows(c.h, 0) == 0
    assert a.act(0.5) == 0      # every row runs the network; the twins stay on the listed form
    for g in range(3):
        a.act_twin(g, 0.5)
    a.assert_equal_twins("greedy rows off")
    assert L.mn_iqn_set_greedy_rows(a.ctx[1].h, 1) == 0      # the contexts of a call must agree
    before = a.actions.clone()
    assert a.act(0.5) == INVALID
    torch.cuda.synchronize()
    assert torch.equal(a.actions, before) and [s.tolist() for s in a.rng] == [s.tolist() for s in a.rng_twin]
    a.close()


@pytest.mark.parametrize("cap,ptr", [(40, 30), (10, 7), (1000, 123)])
def test_append_equals_mn_replay_append(torch, L, cap, ptr):
    G, n = 3, 16
    a = Actors(torch, L, G, n, ring_cap=cap)
    gen = torch.Generator(device=DEV); gen.manual_seed(cap)
    obs, nxt = a.obs, torch.randn(G * n, 26, device=DEV, generator=gen)
    act = torch.randint(0, 9, (G * n,), device=DEV, generator=gen, dtype=torch.int32)
    rew = torch.randn(G * n, device=DEV, generator=gen)
    done = torch.randint(0, 2, (G * n,), device=DEV, generator=gen).to(torch.uint8) * 3      # (any non-zero byte is "done")
    want = [{k: t.clone() for k, t in r.items()} for r in a.rings]
    for g, r in enumerate(want):
        s = slice(g * n, (g + 1) * n)
        assert L.mn_replay_append(_p(obs[s]), _p(act[s]), _p(rew[s]), _p(nxt[s]), _p(done[s]), _p(r["states"]), _p(r["next_states"]), _p(r["actions"]),
                                  _p(r["rewards"]), _p(r["dones"]), n, ptr, cap, _stream(torch)) == 0
    assert L.mn_iqn_actor_group_append(a.h, _p(obs), _p(act), _p(rew), _p(nxt), _p(done), ptr, cap, _stream(torch)) == 0
    torch.cuda.synchronize()
    assert a.arena.guards_intact()
    for g in range(G):
        for k in want[g]:
            assert torch.equal(_bits(a.rings[g][k]), _bits(want[g][k])), (g, k)
    # the rule in words: row i of group g at slot (ptr + i - first) mod cap, first = max(0, n - cap); every other slot as it was
    first = max(0, n - cap)
    for g in range(G):
        for i in range(first, n):
            slot = (ptr + i - first) % cap
            assert torch.equal(a.rings[g]["states"][slot], obs[g * n + i]) and int(a.rings[g]["actions"][slot]) == int(act[g * n + i])
            assert float(a.rings[g]["dones"][slot]) == float(done[g * n + i] != 0)
    if cap > n:
        untouched = [s for s in range(cap) if (s - ptr) % cap >= n]
        assert float(a.rings[1]["rewards"][untouched[0], 0]) == float(untouched[0] + 1000)
    a.close()


def test_argument_checks_launch_nothing(torch, L):
    from distributional_rl_navigation_amd import _capi
    from distributional_rl_navigation_amd.iqn.fused_act import ActContext
    G, n = 3, 16
    a = Actors(torch, L, G, n, ring_cap=40)
    h = C.c_void_p()

    def refused(edit, count=G, rows=n):
        table = (_capi.MnIqnActor * max(count, 1))()
        for i in range(min(count, G)):
            C.memmove(C.byref(table[i]), C.byref(a.table[i]), C.sizeof(_capi.MnIqnActor))
        keep = edit(table)      # (whatever the edit allocates stays alive over the call)
        rc = L.mn_iqn_actor_group_create(table, count, rows, C.byref(h))
        del keep
        return rc == INVALID and not h.value

    assert L.mn_iqn_actor_group_create(None, G, n, C.byref(h)) == INVALID and L.mn_iqn_actor_group_create(a.table, G, n, None) == INVALID
    assert refused(lambda t: None, count=0) and refused(lambda t: None, rows=0) and refused(lambda t: None, rows=-3)
    for field in ("ctx", "weights", "rng_state", "draws"):
        assert refused(lambda t, f=field: setattr(t[1], f, None)), field
    for field in ("ring_states", "ring_next_states", "ring_actions", "ring_rewards", "ring_dones"):
        assert refused(lambda t, f=field: setattr(t[2], f, None)), field      # rings: all five or none

    def no_rings(t, which):
        for g in which:
            for f in ("ring_states", "ring_next_states", "ring_actions", "ring_rewards", "ring_dones"):
                setattr(t[g], f, None)
    assert refused(lambda t: no_rings(t, (1,)))      # ... and in every actor or in none

    def hole(t):
        w = (C.c_void_p * 14)(*[a.ctx[0]._ptrs[i] for i in range(14)])
        w[9] = None
        t[0].weights = C.cast(w, C.c_void_p).value
        return w
    assert refused(hole)
    assert refused(lambda t: setattr(t[1], "ctx", t[0].ctx)) and refused(lambda t: setattr(t[2], "rng_state", t[0].rng_state))
    assert refused(lambda t: setattr(t[2], "draws", t[0].draws + 4 * (33 * n - 1)))      # the last float of actor 0's draws
    assert refused(lambda t: setattr(t[1], "ring_rewards", t[0].ring_rewards)) and refused(lambda t: setattr(t[1], "ring_states", t[0].ring_next_states))
    odd = ActContext(DEV)
    odd.weights(a.nets[0])
    odd.set_variant(0)
    assert refused(lambda t: setattr(t[0], "ctx", odd.h.value))
    odd.set_variant(2); odd.set_tau_mode(1)
    assert refused(lambda t: setattr(t[0], "ctx", odd.h.value))
    if torch.cuda.device_count() > 1:      # a context of another device than the current one
        far = ActContext("cuda:1")
        assert refused(lambda t: setattr(t[0], "ctx", far.h.value))

    # ---- act
    state = lambda: ([s.tolist() for s in a.rng], _bits(a.actions).clone(), [_bits(d).clone() for d in a.draws])
    s0 = state()
    assert L.mn_iqn_actor_group_act(None, _p(a.obs), C.c_float(1.0), C.c_float(0.5), _p(a.actions), _stream(torch)) == INVALID
    assert L.mn_iqn_actor_group_act(a.h, None, C.c_float(1.0), C.c_float(0.5), _p(a.actions), _stream(torch)) == INVALID
    assert L.mn_iqn_actor_group_act(a.h, _p(a.obs), C.c_float(1.0), C.c_float(0.5), None, _stream(torch)) == INVALID
    mask, flags = torch.zeros(n, dtype=torch.uint8, device=DEV), torch.zeros(n, dtype=torch.int32, device=DEV)
    assert L.mn_iqn_set_late_rows(a.ctx[1].h, _p(mask), _p(flags), C.c_uint32(1), n) == 0      # late rows armed on one context: no grouped form
    assert a.act(0.5) == INVALID
    assert L.mn_iqn_set_late_rows(a.ctx[1].h, None, None, C.c_uint32(0), 0) == 0
    a.ctx[2].set_tau_mode(1)
    assert a.act(0.5) == INVALID
    a.ctx[2].set_tau_mode(0); a.ctx[0].set_variant(0)
    assert a.act(0.5) == INVALID
    a.ctx[0].set_variant(2)
    # ---- append
    rew, done = torch.zeros(G * n, device=DEV), torch.zeros(G * n, dtype=torch.uint8, device=DEV)
    rings0 = [{k: _bits(t).clone() for k, t in r.items()} for r in a.rings]
    args = lambda **kw: [kw.get(k, v) for k, v in (("g", a.h), ("obs", _p(a.obs)), ("act", _p(a.actions)), ("rew", _p(rew)), ("nxt", _p(a.obs)), ("done", _p(done)),
                                                   ("ptr", 0), ("cap", 40))] + [_stream(torch)]
    for bad in (dict(g=None), dict(obs=None), dict(act=None), dict(rew=None), dict(nxt=None), dict(done=None), dict(cap=0), dict(ptr=-1), dict(ptr=40)):
        assert L.mn_iqn_actor_group_append(*args(**bad)) == INVALID, bad
    acting_only = Actors(torch, L, 2, n, seed0=90)      # a group without rings acts ...
    assert acting_only.act(0.5) == 0
    assert L.mn_iqn_actor_group_append(*args(g=acting_only.h)) == INVALID      # ... and never appends
    acting_only.close()
    torch.cuda.synchronize()
    s1 = state()
    assert s0[0] == s1[0] and torch.equal(s0[1], s1[1]) and all(torch.equal(x, y) for x, y in zip(s0[2], s1[2]))      # no refused call launched anything
    assert all(torch.equal(_bits(t), rings0[g][k]) for g, r in enumerate(a.rings) for k, t in r.items())
    assert a.arena.guards_intact()
    assert a.act(0.5) == 0      # the group is as good as new
    for g in range(G):
        a.act_twin(g, 0.5)
    a.assert_equal_twins("after the refusals")
    a.close()


# ---- the driver ---------------------------------------------------------------------------------------------------------------------------------------
def _nested_equal(a, b):
    """Equality of ragged nests (object arrays / lists of arrays), leaf by leaf; NaN equals NaN in float leaves."""
    if isinstance(a, (list, tuple)) or (isinstance(a, np.ndarray) and a.dtype == object):
        return isinstance(b, (list, tuple, np.ndarray)) and len(a) == len(b) and all(_nested_equal(x, y) for x, y in zip(a, b))
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and np.array_equal(a, b, equal_nan=a.dtype.kind == "f")


def _files_equal(torch, fa, fb):
    """The rule of tests/test_iqn_group_train_gpu.py's driver test."""
    import json
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


def _stacked_against_alone(torch, tmp_path, total, n, common, grad_steps):
    from distributional_rl_navigation_amd.train_iqn import run_trial, run_trials_together
    params = lambda seed, where: dict(agent="IQN", seed=seed, total_timesteps=total, eval_freq=400, save_dir=str(tmp_path / where), training_time="toy")
    seen = []
    dirs, agents = run_trials_together(DEV, [params(s, "stacked") for s in (3, 4)], n, return_agents=True, stack_envs=True,
                                       on_step=[lambda it, st, s=s: seen.append((s, it, float(st["last"]["eps"]), int(st["last"]["done"].sum()),
                                                                                 float(st["last"]["reward"].sum()))) for s in (3, 4)], **common)
    assert [os.path.basename(d) for d in dirs] == ["seed_3", "seed_4"]
    assert [x[:2] for x in seen[:4]] == [(3, 0), (4, 0), (3, 1), (4, 1)]      # per seed and step, in seed order
    assert not torch.equal(agents[0]._fused.local, agents[1]._fused.local)
    eps = [x[2] for x in seen]
    for seed, d, agent in zip((3, 4), dirs, agents):
        alone_seen = []
        d1, alone = run_trial(DEV, params(seed, "alone"), n, return_agent=True,
                              on_step=lambda it, st: alone_seen.append((seed, it, float(st["last"]["eps"]), int(st["last"]["done"].sum()), float(st["last"]["reward"].sum()))),
                              **common)
        assert agent.grad_steps == alone.grad_steps == grad_steps
        assert alone_seen == [x for x in seen if x[0] == seed]      # the hook sequences, with every step's episode ends and reward sum
        for name in ("local", "target", "exp_avg", "exp_avg_sq", "step_dev", "rng_state"):
            assert torch.equal(_bits(getattr(agent._fused, name)), _bits(getattr(alone._fused, name))), (seed, name)
        assert agent._act_rng.state.tolist() == alone._act_rng.state.tolist() and agent._act_rng.state[1] > 0, seed
        ma, mb = agent.memory, alone.memory      # the ring: the grouped append against mn_step_append
        assert (ma.size, ma.ptr) == (mb.size, mb.ptr) and ma.size > 0
        for k in ("states", "next_states", "actions", "rewards", "dones"):
            assert torch.equal(_bits(getattr(ma, k)[:ma.size]), _bits(getattr(mb, k)[:mb.size])), (seed, k)
        assert agent._fused.timeouts() == 0
        names = sorted(os.listdir(d))
        assert names == sorted(os.listdir(d1)) and "network_params.pth" in names and "greedy_evaluations.npz" in names
        for f in names:
            assert os.path.isfile(os.path.join(d, f)), f
            _files_equal(torch, os.path.join(d, f), os.path.join(d1, f))
    return eps, seen


def _eval_worlds(n=3):
    from distributional_rl_navigation_amd.train_iqn import create_eval_configs
    cfg = create_eval_configs(DEV)
    return {k: cfg[k] for k in list(cfg)[:n]}


def test_driver_files_equal_the_sequential_runs(torch, tmp_path):
    """The toy reference-budget run of tests/test_iqn_group_train_gpu.py: seeds 3 and 4 through run_trials_together(stack_envs=True), and each through run_trial."""
    common = dict(verbose=False, env_budget="reference", reference=dict(learning_starts=400, target_update_interval=400), eval_config=_eval_worlds(), max_eval_steps=60,
                  episode_log="full", eval_deferred=dict(verbose=False))
    _, seen = _stacked_against_alone(torch, tmp_path, 4_000, 16, common, grad_steps=900)      # (4 000 - 400) / 4
    assert len(seen) == 2 * (4_000 // 16)
    assert "training_episodes.npz" in os.listdir(tmp_path / "stacked" / "training_toy" / "seed_3")


def test_driver_learner_budget_with_falling_eps_and_a_moving_curriculum(torch, tmp_path, monkeypatch):
    """The learner-budget mode at 32 envs per seed for 300 vector steps: the exploration rate falls through (0, 1) (listed rows, lists of changing length) and
    -- with the curriculum's thresholds brought into the toy run -- every env's world size changes twice."""
    from distributional_rl_navigation_amd import train_iqn
    monkeypatch.setattr(train_iqn, "TRAINING_SCHEDULE", dict(timesteps=[0, 400, 800], num_cores=[4, 6, 8], num_obstacles=[6, 8, 10],
                                                             min_start_goal_dis=[30.0, 35.0, 40.0]))
    common = dict(verbose=False, batch=32, eval_config=_eval_worlds(), max_eval_steps=60, episode_log="full")
    eps, seen = _stacked_against_alone(torch, tmp_path, 1_200, 32, common, grad_steps=299)      # (behind the first vector step the ring holds one batch, not more than one: agent.py:129)
    assert len(seen) == 2 * 300
    assert eps[0] == 1.0 and 0.0 < min(eps) < 0.5 and len({e for e in eps if 0.0 < e < 1.0}) > 10
    assert sum(x[3] for x in seen) > 0      # episodes did end (and were reset in the stacked handle)
