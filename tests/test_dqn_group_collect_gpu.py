"""Many DQN actors per launch (C-ABI mn_dqn_actor_group_*, csrc/dqn_collect.hip + replay.hip; dqn/group_collect.py; `train_dqn --together --stack-envs`):
every actor of a grouped call against the single calls it stands for -- mn_dqn_act_rng with its own seed, call index, weights and image, mn_replay_append
into its own ring -- bit for bit, and the stacked driver's files against each seed's own run."""
import ctypes as C
import io
import json
import os
import zipfile

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENT = 0x7FC0DEAD    # (a NaN with a payload, as float)
GUARD = 3            # rows in front of and behind every ring, rows behind every output
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


def _sentinels(torch, shape, dtype):
    words = int(np.prod(shape)) * torch.empty(0, dtype=dtype).element_size() // 4
    return torch.full((words,), SENT, dtype=torch.int32, device=DEV).view(dtype).view(*shape)


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


@pytest.fixture(scope="module")
def policies(torch):
    """64 policies with distinct random networks."""
    return [_random_policy(torch, 900 + g) for g in range(64)]


class Ring:
    """The five arrays of a replay ring of `cap` rows between GUARD sentinel rows."""

    def __init__(self, torch, cap):
        self.cap = cap
        rows = cap + 2 * GUARD
        self.full = dict(states=_sentinels(torch, (rows, 26), torch.float32), next_states=_sentinels(torch, (rows, 26), torch.float32),
                         actions=_sentinels(torch, (rows, 1), torch.int64), rewards=_sentinels(torch, (rows, 1), torch.float32),
                         dones=_sentinels(torch, (rows, 1), torch.float32))
        for k, t in self.full.items():
            setattr(self, k, t[GUARD:GUARD + cap])


class Actors:
    """G actors -- policies[g], seed 100 + 11 g, an image and (with `ring_cap`) a ring of its own -- as a group, and a second image and ring per actor for
    the single calls."""

    def __init__(self, torch, L, policies, G, n, ring_cap=None):
        from distributional_rl_navigation_amd import _capi
        self.torch, self.L, self.G, self.n, self.cap = torch, L, G, n, ring_cap
        self.policies = policies[:G]
        floats = int(L.mn_dqn_image_floats())
        self.ptrs, self.seeds = [], [100 + 11 * g + (g % 3 << 40) for g in range(G)]
        for pol in self.policies:
            st, _ = pol._image(torch.device(DEV))
            self.ptrs.append((C.c_void_p * 18)(*[st["ptrs"][i] for i in range(18)]))
        self.images = [_sentinels(torch, (floats,), torch.float32) for _ in range(G)]
        self.images_single = [_sentinels(torch, (floats,), torch.float32) for _ in range(G)]
        self.rings = [Ring(torch, ring_cap) for _ in range(G)] if ring_cap else None
        self.rings_single = [Ring(torch, ring_cap) for _ in range(G)] if ring_cap else None
        table = (_capi.MnDqnActor * G)()
        for g, row in enumerate(table):
            row.weights, row.image, row.seed = C.cast(self.ptrs[g], C.c_void_p).value, self.images[g].data_ptr(), self.seeds[g]
            if ring_cap:
                r = self.rings[g]
                row.ring_states, row.ring_next_states, row.ring_actions = r.states.data_ptr(), r.next_states.data_ptr(), r.actions.data_ptr()
                row.ring_rewards, row.ring_dones = r.rewards.data_ptr(), r.dones.data_ptr()
        self.table = table
        self.h = C.c_void_p()
        assert L.mn_dqn_actor_group_create(table, G, n, C.byref(self.h)) == 0
        self.obs = torch.randn(G * n + GUARD, 26, generator=torch.Generator().manual_seed(1000 * G + n)).to(DEV)

    def close(self):
        assert self.L.mn_dqn_actor_group_destroy(self.h) == 0

    def calls(self, k=0):
        """Distinct call indices, some beyond 2^32."""
        return [3 * g + k + ((g % 2) << 33) for g in range(self.G)]

    def act(self, eps, stale, calls):
        torch, G, n = self.torch, self.G, self.n
        a = _sentinels(torch, (G * n + GUARD,), torch.int32)
        rc = self.L.mn_dqn_actor_group_act(self.h, _p(self.obs), C.c_float(eps), stale, (C.c_uint64 * G)(*calls), _p(a), _stream(torch))
        assert rc == 0
        assert (a[G * n:] == SENT).all()
        return a[:G * n]

    def act_single(self, eps, repack, calls):
        """The G single calls, each on its own rows with its own second image; `repack`: per actor."""
        torch, G, n = self.torch, self.G, self.n
        a = _sentinels(torch, (G * n + GUARD,), torch.int32)
        for g in range(G):
            rc = self.L.mn_dqn_act_rng(_p(self.obs[g * n:]), self.ptrs[g], _p(self.images_single[g]), int(repack[g]), self.seeds[g], calls[g], C.c_float(eps),
                                       None, None, _p(a[g * n:]), n, _stream(torch))
            assert rc == 0
        return a[:G * n]


@pytest.mark.parametrize("eps", [0.05, 1.0])
@pytest.mark.parametrize("G,n", [(1, 17), (3, 1), (3, 130), (64, 16)])
def test_act_equals_the_single_calls(torch, L, policies, G, n, eps):
    ac = Actors(torch, L, policies, G, n)
    every = (1 << G) - 1
    want = ac.act_single(eps, [1] * G, ac.calls())
    got = ac.act(eps, every, ac.calls())
    assert torch.equal(got, want)
    for g in range(G):      # the grouped pack writes the single pack's image
        assert torch.equal(_bits(ac.images[g]), _bits(ac.images_single[g])), g
    if G > 1 and n > 1 and eps < 1:
        rows = got.view(G, n)
        assert not torch.equal(rows[0], rows[1])      # other weights, other draws
    # the workgroups per group change nothing, and neither does a second call with fresh images
    for grid in (1, 2, 1000, 0):
        assert L.mn_dqn_actor_group_set_grid(ac.h, grid) == 0
        assert torch.equal(ac.act(eps, 0, ac.calls()), want), grid
    other = ac.act(0.5, 0, ac.calls(1))
    assert torch.equal(other, ac.act_single(0.5, [0] * G, ac.calls(1)))
    ac.close()


def test_only_the_stale_images_are_rebuilt(torch, L, policies):
    G, n = 3, 40
    own = [_random_policy(torch, 50 + g) for g in range(G)]      # (policies of this test's own: it writes their weights)
    ac = Actors(torch, L, own, G, n)
    first = ac.act(0.0, 0b111, ac.calls())
    assert torch.equal(first, ac.act_single(0.0, [1, 1, 1], ac.calls()))
    before = [_bits(im) for im in ac.images]
    with torch.no_grad():
        for g, action in ((0, 2), (1, 7)):
            own[g].q_net.q_net[4].bias[action] += 1.0e3      # now that action wins everywhere
    got = ac.act(0.0, 0b010, ac.calls(1)).view(G, n)      # only actor 1 is named
    assert torch.equal(got[0], first.view(G, n)[0]) and not (got[0] == 2).all()      # actor 0: the old image
    assert (got[1] == 7).all()      # actor 1: the new one
    assert torch.equal(got[2], first.view(G, n)[2])
    assert torch.equal(_bits(ac.images[0]), before[0]) and torch.equal(_bits(ac.images[2]), before[2])
    assert not torch.equal(_bits(ac.images[1]), before[1])
    assert torch.equal(got.view(-1), ac.act_single(0.0, [0, 1, 0], ac.calls(1)))
    got = ac.act(0.3, 0b001, ac.calls(2)).view(G, n)
    assert torch.equal(got.view(-1), ac.act_single(0.3, [1, 0, 0], ac.calls(2)))
    ac.close()


@pytest.mark.parametrize("cap,ptr,n", [(64, 0, 17), (64, 60, 17), (16, 3, 17)])
def test_append_equals_mn_replay_append(torch, L, policies, cap, ptr, n):
    """A plain append, one that wraps, and n > capacity, where only the newest rows survive."""
    G = 3
    ac = Actors(torch, L, policies, G, n, ring_cap=cap)
    gen = torch.Generator().manual_seed(cap + ptr)
    obs, nxt = (torch.randn(G * n, 26, generator=gen).to(DEV) for _ in range(2))
    actions = torch.randint(0, 9, (G * n,), generator=gen, dtype=torch.int32).to(DEV)
    reward = torch.randn(G * n, generator=gen).to(DEV)
    done = (torch.rand(G * n, generator=gen) < 0.3).to(torch.uint8).to(DEV)
    assert L.mn_dqn_actor_group_append(ac.h, _p(obs), _p(actions), _p(reward), _p(nxt), _p(done), ptr, cap, _stream(torch)) == 0
    for g in range(G):
        r, sl = ac.rings_single[g], slice(g * n, (g + 1) * n)
        rc = L.mn_replay_append(_p(obs[sl]), _p(actions[sl]), _p(reward[sl]), _p(nxt[sl]), _p(done[sl]), _p(r.states), _p(r.next_states), _p(r.actions),
                                _p(r.rewards), _p(r.dones), n, ptr, cap, _stream(torch))
        assert rc == 0
        for k in r.full:
            assert torch.equal(_bits(ac.rings[g].full[k]), _bits(r.full[k])), (g, k)      # guard rows included
        for k, t in ac.rings[g].full.items():
            words = t.contiguous().view(-1).view(torch.int32).view(cap + 2 * GUARD, -1)
            assert (words[:GUARD] == SENT).all() and (words[GUARD + cap:] == SENT).all(), (g, k)
        written = min(n, cap)
        rows = [(ptr + i) % cap for i in range(written)]
        assert torch.equal(ac.rings[g].states[rows], obs[sl][n - written:])      # row i of the group at slot (ptr + i - first) mod cap
        assert torch.equal(ac.rings[g].actions[rows, 0], actions[sl][n - written:].long())
    ac.close()


def test_argument_checks_launch_nothing(torch, L, policies):
    from distributional_rl_navigation_amd import _capi
    G, n = 3, 20
    ac = Actors(torch, L, policies, G, n, ring_cap=32)
    h = C.c_void_p()

    def bad(edit, count=G, rows=n):
        t = (_capi.MnDqnActor * G)(*ac.table)      # a copy of the good table with one thing wrong
        edit(t)
        return L.mn_dqn_actor_group_create(t, count, rows, C.byref(h))

    same = lambda t: None
    assert bad(same, count=0) == INVALID and bad(same, rows=0) == INVALID and L.mn_dqn_actor_group_create(None, G, n, C.byref(h)) == INVALID
    assert L.mn_dqn_actor_group_create(ac.table, G, n, None) == INVALID
    assert L.mn_dqn_actor_group_create((_capi.MnDqnActor * 65)(), 65, n, C.byref(h)) == INVALID
    assert bad(lambda t: setattr(t[1], "weights", None)) == INVALID
    assert bad(lambda t: setattr(t[1], "image", None)) == INVALID
    assert bad(lambda t: setattr(t[2], "image", t[0].image)) == INVALID      # two actors, one image
    assert bad(lambda t: setattr(t[2], "ring_dones", None)) == INVALID      # rings given in part
    assert bad(lambda t: setattr(t[2], "ring_states", t[0].ring_states)) == INVALID      # two actors, one ring array
    holed = (C.c_void_p * 18)(*[ac.ptrs[1][i] for i in range(18)])
    holed[4] = None
    assert bad(lambda t: setattr(t[1], "weights", C.cast(holed, C.c_void_p).value)) == INVALID
    assert h.value is None
    # act and append: the outputs, the images and the rings keep their sentinels
    a = _sentinels(torch, (G * n,), torch.int32)
    calls = (C.c_uint64 * G)(*ac.calls())
    s = _stream(torch)
    assert L.mn_dqn_actor_group_act(None, _p(ac.obs), C.c_float(0.5), 0b111, calls, _p(a), s) == INVALID
    assert L.mn_dqn_actor_group_act(ac.h, None, C.c_float(0.5), 0b111, calls, _p(a), s) == INVALID
    assert L.mn_dqn_actor_group_act(ac.h, _p(ac.obs), C.c_float(0.5), 0b111, None, _p(a), s) == INVALID
    assert L.mn_dqn_actor_group_act(ac.h, _p(ac.obs), C.c_float(0.5), 0b111, calls, None, s) == INVALID
    assert L.mn_dqn_actor_group_act(ac.h, _p(ac.obs), C.c_float(0.5), 0b1000, calls, _p(a), s) == INVALID      # a bit beyond the group
    assert L.mn_dqn_actor_group_set_grid(ac.h, -1) == INVALID and L.mn_dqn_actor_group_set_grid(None, 1) == INVALID
    act = torch.zeros(G * n, dtype=torch.int32, device=DEV)
    rew = torch.zeros(G * n, device=DEV)
    done = torch.zeros(G * n, dtype=torch.uint8, device=DEV)
    ap = lambda g, o, ptr, cap: L.mn_dqn_actor_group_append(g, o, _p(act), _p(rew), _p(ac.obs), _p(done), ptr, cap, s)
    assert ap(None, _p(ac.obs), 0, 32) == INVALID and ap(ac.h, None, 0, 32) == INVALID
    assert ap(ac.h, _p(ac.obs), 32, 32) == INVALID and ap(ac.h, _p(ac.obs), -1, 32) == INVALID and ap(ac.h, _p(ac.obs), 0, 0) == INVALID
    acting = Actors(torch, L, policies, 2, n)      # a group without rings cannot append
    assert ap(acting.h, _p(ac.obs), 0, 32) == INVALID
    acting.close()
    torch.cuda.synchronize()
    assert (a == SENT).all()
    for g in range(G):
        assert (ac.images[g].view(torch.int32) == SENT).all()
        for t in ac.rings[g].full.values():
            assert (t.contiguous().view(-1).view(torch.int32) == SENT).all()
    ac.close()
    assert L.mn_dqn_actor_group_destroy(None) == INVALID


# ---- the agents' group --------------------------------------------------------------------------------------------------------------------------------
def _agents(G, **kw):
    from distributional_rl_navigation_amd.dqn import DQNAgent
    return [DQNAgent(device=DEV, seed=20 + g, **dict(dict(buffer_size=64, batch_size=8, fused_collect=True), **kw)) for g in range(G)]


def test_grouped_and_single_calls_interleave_on_the_same_agents(torch):
    """Agents of a CollectorGroup act and append through the group and alone in turn, with weight writes between; their twins only ever act alone."""
    from types import SimpleNamespace
    from distributional_rl_navigation_amd.dqn.group_collect import CollectorGroup
    G, n = 3, 21
    agents, twins = _agents(G), _agents(G)
    group = CollectorGroup(agents, SimpleNamespace(n_envs=G * n))
    gen = torch.Generator().manual_seed(8)
    rows = lambda g: slice(g * n, (g + 1) * n)

    def batch():
        obs, nxt = (torch.randn(G * n, 26, generator=gen).to(DEV) for _ in range(2))
        return obs, nxt, torch.randn(G * n, generator=gen).to(DEV), (torch.rand(G * n, generator=gen) < 0.3).to(torch.uint8).to(DEV)

    def alone(ags, obs, eps):
        return torch.cat([ag.act_batch(obs[rows(g)], eps) for g, ag in enumerate(ags)])

    def write(ags, g, k):
        with torch.no_grad():
            ags[g].q_net.q_net[4].bias[k] += 0.5      # (a PyTorch write: the version counter marks the image stale)

    for step, (eps, grouped) in enumerate(((1.0, True), (0.5, False), (0.5, True), (0.05, True), (0.0, False), (0.3, True))):
        obs, nxt, reward, done = batch()
        if step in (2, 3):
            for ags in (agents, twins):
                write(ags, step - 2, 4)
        a = group.act(obs, eps) if grouped else alone(agents, obs, eps)
        b = alone(twins, obs, eps)
        assert torch.equal(a, b), step
        if grouped:
            group.append(obs, a, reward, nxt, done)
        else:
            for g, ag in enumerate(agents):
                ag.memory.add_vector_step(obs[rows(g)], a[rows(g)].contiguous(), reward[rows(g)], nxt[rows(g)], done[rows(g)])
        for g, ag in enumerate(twins):
            ag.memory.add_vector_step(obs[rows(g)], b[rows(g)].contiguous(), reward[rows(g)], nxt[rows(g)], done[rows(g)])
        assert [ag.act_calls for ag in agents] == [step + 1] * G == [ag.act_calls for ag in twins]
    for ag, tw in zip(agents, twins):      # 126 rows into rings of 64: wrapped
        assert (ag.memory.ptr, ag.memory.size) == (tw.memory.ptr, tw.memory.size) == (6 * n % 64, 64)
        for k in ("states", "next_states", "actions", "rewards", "dones"):
            assert torch.equal(_bits(getattr(ag.memory, k)), _bits(getattr(tw.memory, k))), k
    agents[1].memory.advance(1)
    with pytest.raises(ValueError, match="write position"):
        group.append(*(lambda o, x, r, d: (o, torch.zeros(G * n, dtype=torch.int32, device=DEV), r, x, d))(*batch()))
    group.close()


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
    elif fa.endswith(".zip"):      # a checkpoint: the tensors of its policy.pth
        sa, sb = (torch.load(io.BytesIO(zipfile.ZipFile(f).read("policy.pth")), map_location="cpu") for f in (fa, fb))
        assert list(sa) == list(sb) and len(sa) > 0, fa
        for k in sa:
            assert torch.equal(_bits(sa[k]), _bits(sb[k])), (fa, k)
    elif fa.endswith(".json"):
        ja, jb = json.load(open(fa)), json.load(open(fb))
        for j in (ja, jb):      # (the runs live in different directories: the one entry that has to differ)
            if isinstance(j, dict):
                j.pop("save_dir", None)
        assert ja == jb, fa
    else:
        assert open(fa, "rb").read() == open(fb, "rb").read(), fa


def _eval_worlds(n=3):
    from distributional_rl_navigation_amd.train_iqn import create_eval_configs
    cfg = create_eval_configs(DEV)
    return {k: cfg[k] for k in list(cfg)[:n]}


def _hook(seen, seed):
    return lambda it, st: seen.append((seed, it, float(st["last"]["eps"]), int(st["last"]["done"].sum()), float(st["last"]["reward"].sum())))


def _stacked_against_together_and_alone(torch, tmp_path, total, n, common, n_updates):
    """Seeds 3 and 4 through run_trials_together(stack_envs=True), through run_trials_together(fused_collect=True) and each through
    run_trial(fused_collect=True): the hook sequences, the learners, the rings and every file, seed by seed."""
    from distributional_rl_navigation_amd.train_dqn import run_trial, run_trials_together
    params = lambda seed, where: dict(agent="DQN", seed=seed, total_timesteps=total, eval_freq=400, save_dir=str(tmp_path / where), training_time="toy")
    seen, seen_t = [], []
    dirs, agents = run_trials_together(DEV, [params(s, "stacked") for s in (3, 4)], n, return_agents=True, stack_envs=True,
                                       on_step=[_hook(seen, s) for s in (3, 4)], **common)
    dirs_t, agents_t = run_trials_together(DEV, [params(s, "together") for s in (3, 4)], n, return_agents=True, fused_collect=True,
                                           on_step=[_hook(seen_t, s) for s in (3, 4)], **common)
    assert [os.path.basename(d) for d in dirs] == ["seed_3", "seed_4"]
    assert [x[:2] for x in seen[:4]] == [(3, 0), (4, 0), (3, 1), (4, 1)]      # per seed and step, in seed order
    assert seen == seen_t
    assert not torch.equal(agents[0]._fused.local, agents[1]._fused.local)
    for seed, d, dt, agent, agent_t in zip((3, 4), dirs, dirs_t, agents, agents_t):
        alone_seen = []
        d1, alone = run_trial(DEV, params(seed, "alone"), n, return_agent=True, fused_collect=True, on_step=_hook(alone_seen, seed), **common)
        assert agent.n_updates == agent_t.n_updates == alone.n_updates == n_updates
        assert alone_seen == [x for x in seen if x[0] == seed]      # the hook sequences, with every step's episode ends and reward sum
        assert agent.act_calls == agent_t.act_calls == alone.act_calls > 0 and agent.num_timesteps == alone.num_timesteps
        for other in (agent_t, alone):
            for name in ("local", "target", "exp_avg", "exp_avg_sq", "step_dev", "rng_state"):
                assert torch.equal(_bits(getattr(agent._fused, name)), _bits(getattr(other._fused, name))), (seed, name)
            ma, mb = agent.memory, other.memory      # the ring: the grouped append against mn_step_append
            assert (ma.size, ma.ptr) == (mb.size, mb.ptr) and ma.size > 0
            for k in ("states", "next_states", "actions", "rewards", "dones"):
                assert torch.equal(_bits(getattr(ma, k)[:ma.size]), _bits(getattr(mb, k)[:mb.size])), (seed, k)
        names = sorted(os.listdir(d))
        assert names == sorted(os.listdir(dt)) == sorted(os.listdir(d1))
        assert {"evaluations.npz", "latest_model.zip", "best_model.zip", "trial_config.json"} <= set(names), names
        for f in names:
            assert os.path.isfile(os.path.join(d, f)), f
            _files_equal(torch, os.path.join(d, f), os.path.join(dt, f))
            _files_equal(torch, os.path.join(d, f), os.path.join(d1, f))
    return seen


def test_driver_files_equal_the_sequential_runs(torch, tmp_path):
    """The toy reference-budget run of tests/test_dqn_group_train_gpu.py (2 000 env steps in vector steps of 16, learning from 400 on, target copies every
    400 gradient steps, three evaluation worlds of 60 steps)."""
    common = dict(verbose=False, env_budget="reference", reference=dict(learning_starts=400, target_update_interval=400), eval_config=_eval_worlds(),
                  max_eval_steps=60)
    seen = _stacked_against_together_and_alone(torch, tmp_path, 2_000, 16, common, n_updates=1_600)
    assert len(seen) == 2 * (2_000 // 16)
    assert "training_log.npz" in os.listdir(tmp_path / "stacked" / "training_toy" / "seed_3")


def test_driver_learner_budget_with_falling_eps_and_a_moving_curriculum(torch, tmp_path, monkeypatch):
    """The learner-budget mode at 128 envs per seed for 200 vector steps (learning from vector step 79 on: sb3's learning_starts of 10 000 env steps): the
    exploration rate falls from 1 to 0.05 over the first 20, the ring of 8 192 rows wraps, and -- with the curriculum's thresholds brought into the toy
    run -- every env's world size changes twice."""
    from distributional_rl_navigation_amd import train_dqn
    monkeypatch.setattr(train_dqn, "TRAINING_SCHEDULE", dict(timesteps=[0, 400, 800], num_cores=[4, 6, 8], num_obstacles=[6, 8, 10],
                                                             min_start_goal_dis=[30.0, 35.0, 40.0]))
    common = dict(verbose=False, batch=32, replay=8_192, total_grad_steps=200, eval_config=_eval_worlds(), max_eval_steps=60, episode_log="full")
    seen = _stacked_against_together_and_alone(torch, tmp_path, 1_200, 128, common, n_updates=200 - 78)
    assert len(seen) == 2 * 200
    eps = [x[2] for x in seen]
    assert eps[0] == 1.0 and min(eps) == pytest.approx(0.05) and len({e for e in eps if 0.05 < e < 1.0}) >= 19
    assert sum(x[3] for x in seen) > 0      # episodes did end (and were reset in the stacked handle)
