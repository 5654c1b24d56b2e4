"""Episode bookkeeping (distributional_rl_navigation_amd/episodes.py) against statements of the per-step loop that do not use it: `tally` and
`steps_run` on hand-made traces, `energy_table` against the torch expression it replaced, `loop_episodes` on CPU tensors with a scripted env, and the
sweep's record builder on top of `tally`.  No GPU."""
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from distributional_rl_navigation_amd.episodes import energy_table, loop_episodes, steps_run, tally, trace_buffers

SHIPPED_A, SHIPPED_W = [-0.4, 0.0, 0.4], [-math.pi / 6, 0.0, math.pi / 6]      # mn_default_params


def _torch_energy_table(a, w):
    """The expression the evaluation loops carried (robot.py:72-77)."""
    a_tab = torch.tensor(a); w_tab = torch.tensor(w)
    return ((a_tab / a_tab.max()).abs().view(3, 1) + (w_tab / w_tab.max()).abs().view(1, 3)).reshape(-1)


def _loop_restated(reward, done, info, action, discount, energy_tab, groups=1):
    """The evaluation loop body as the per-step loops carried it (torch, CPU), fed from traces.  Also counts, step by step, the envs alive before
    each step in each of `groups` equal slices of the envs."""
    T, n = reward.shape
    etab = torch.from_numpy(np.asarray(energy_tab, dtype=np.float32))
    alive = torch.ones(n, dtype=torch.bool)
    ret = torch.zeros(n, dtype=torch.float64)
    length = torch.zeros(n, dtype=torch.int64)
    energy = torch.zeros(n, dtype=torch.float64)
    last_info = torch.zeros(n, dtype=torch.uint8)
    acts = torch.full((T, n), -1, dtype=torch.int32)
    live = []
    for t in range(T):
        live.append(alive.view(groups, n // groups).sum(dim=1).tolist())
        a = torch.from_numpy(action[t]).clamp(0, 8)      # (a dead row carries some action; masked either way)
        r = torch.from_numpy(reward[t]); d = torch.from_numpy(done[t]); i = torch.from_numpy(info[t])
        ret += torch.where(alive, (discount ** t) * r.double(), torch.zeros_like(ret))
        length += alive.long()
        energy += torch.where(alive, etab[a.long()].double(), torch.zeros_like(energy))
        acts[t] = torch.where(alive, a, torch.full_like(a, -1))
        last_info = torch.where(alive, i, last_info)
        alive = alive & ~d.bool()
        if not bool(alive.any()):
            break
    acts_h, length_h = acts.numpy(), length.numpy()
    return dict(ret=ret.numpy(), energy=energy.numpy(), length=length_h, last_info=last_info.numpy(),
                actions=[[int(x) for x in acts_h[:length_h[k], k]] for k in range(n)]), live


def _traces(seed, T=120, n=24, past_T=True):
    """Traces as an episode launch writes them: env i ends with step ends[i] - 1 (some never within T when `past_T`); behind its end reward 0, done 1,
    its terminal info code and action -1."""
    rng = np.random.RandomState(seed)
    ends = rng.randint(1, T + 30, size=n) if past_T else rng.randint(1, T - 40, size=n)
    ends[1] = 1                                        # one episode over after its first step
    t_idx = np.arange(T)[:, None]
    alive_before = t_idx < ends[None, :]
    done = (t_idx >= ends[None, :] - 1).astype(np.uint8)
    term = rng.randint(1, 5, size=n).astype(np.uint8)
    info = np.where(t_idx >= ends[None, :] - 1, term[None, :], 0).astype(np.uint8)
    reward = rng.standard_normal((T, n)).astype(np.float32)
    reward[rng.rand(T, n) < 0.1] = np.float32(-0.0)
    reward[0, 0] = np.float32(-0.0)                  # a return that starts from -0.0
    reward = np.where(alive_before, reward, np.float32(0)).astype(np.float32)
    action = np.where(alive_before, rng.randint(0, 9, size=(T, n)), -1).astype(np.int32)
    assert (reward < 0).any() and (np.signbit(reward) & (reward == 0)).any() and (action == -1).any()
    return dict(reward=reward, done=done, info=info, action=action), ends


def _assert_tally_equal(got, want):
    assert sorted(got) == sorted(want)
    for k in ("ret", "energy", "length", "last_info"):
        assert got[k].dtype == want[k].dtype, k
        assert got[k].tobytes() == want[k].tobytes(), k      # bit for bit (the sign of a zero included)
    assert got["actions"] == want["actions"]
    assert all(type(x) is int for row in got["actions"] for x in row)


@pytest.mark.parametrize("seed,past_T", [(0, True), (1, True), (2, False), (3, False)])
def test_tally_equals_restated_loop_cut_and_uncut(seed, past_T):
    tr, ends = _traces(seed, past_T=past_T)
    etab = _torch_energy_table(SHIPPED_A, SHIPPED_W).numpy()
    want, _ = _loop_restated(tr["reward"], tr["done"], tr["info"], tr["action"], 0.99, etab)
    T = steps_run(tr["done"])
    assert T == min(120, ends.max()) and (T == 120) == past_T
    uncut = tally(tr["reward"], tr["done"], tr["info"], tr["action"], 0.99, etab)
    cut = tally(tr["reward"][:T], tr["done"][:T], tr["info"][:T], tr["action"][:T], 0.99, etab)
    _assert_tally_equal(uncut, want)
    _assert_tally_equal(cut, want)
    assert want["length"].tolist() == np.minimum(ends, 120).tolist()


def test_steps_run():
    T, n = 7, 5
    assert steps_run(np.ones((T, n), dtype=np.uint8)) == 1                 # all done at step 0
    assert steps_run(np.zeros((T, n), dtype=np.uint8)) == T                # none done
    d = np.zeros((T, n), dtype=np.uint8)
    d[2:, :4] = 1
    assert steps_run(d) == T                                               # one env still alive behind the traces
    d[T - 1, 4] = 1
    assert steps_run(d) == T                                               # the last episode ends on row T - 1
    d[T - 2, 4] = 1
    assert steps_run(d) == T - 1
    assert steps_run(d.astype(bool)) == T - 1


@pytest.mark.parametrize("a,w", [(SHIPPED_A, SHIPPED_W), ([-0.3, 0.1, 0.7], [-0.45, 0.2, 1.3])])
def test_energy_table_equals_torch_expression(a, w):
    got, want = energy_table(a, w), _torch_energy_table(a, w).numpy()
    assert got.dtype == np.float32 and got.shape == (9,)
    assert got.tobytes() == want.tobytes()
    if a is not SHIPPED_A:      # ratios that float32 has to round
        assert any(float(np.float32(x) / np.float32(max(a))) != x / max(a) for x in a)


def test_trace_buffers_table():
    tr = trace_buffers(3, 4, "cpu", ("obs", "reward", "done", "info", "action", "cvar", "q"), obs_dim=26, n_actions=9)
    assert {k: (tuple(v.shape), v.dtype) for k, v in tr.items()} == dict(
        obs=((3, 4, 26), torch.float32), reward=((3, 4), torch.float32), done=((3, 4), torch.uint8), info=((3, 4), torch.uint8),
        action=((3, 4), torch.int32), cvar=((3, 4), torch.float32), q=((3, 4, 9), torch.float32))
    assert bool((tr["obs"] == 0).all()) and bool(tr["cvar"].isnan().all()) and bool(tr["q"].isnan().all())
    assert list(trace_buffers(2, 2, "cpu", ("done", "obs"), fill=False)) == ["done", "obs"]


class _ScriptedEnv:
    """Env i ends with step ends[i] - 1 and, like the real env without a reset, goes on being stepped: behind its end it reports junk (reward 5,
    done 0, info 7) that the loop has to mask."""

    def __init__(self, script, ends):
        self.script, self.ends, self.t, self.seen = script, torch.from_numpy(ends), 0, []

    def step(self, a):
        t, self.t = self.t, self.t + 1
        self.seen.append(a.clone())
        over = t >= self.ends
        reward = torch.where(over, torch.full((len(over),), 5.0), torch.from_numpy(self.script["reward"][t]))
        done = (t == self.ends - 1).to(torch.uint8)
        info = torch.where(over, torch.full((len(over),), 7, dtype=torch.uint8), torch.from_numpy(self.script["info"][t]))
        return torch.full((len(over), 26), float(t + 1)), reward, done, info


@pytest.mark.parametrize("max_steps", [120, 50])
def test_loop_episodes_on_a_scripted_env(max_steps):
    script, ends = _traces(5, past_T=False)
    n = len(ends)
    want_steps = min(max_steps, int(ends.max()))
    env = _ScriptedEnv(script, ends)
    rng = np.random.RandomState(6)
    chosen = rng.randint(0, 9, size=(120, n)).astype(np.int32)      # the policy also "acts" for finished envs
    calls, stepped = [], []

    def act(t, obs):
        assert float(obs[0, 0]) == float(t)      # the observation of the step before
        calls.append(t)
        return torch.from_numpy(chosen[t])
    tr = loop_episodes(env, torch.zeros(n, 26), act, max_steps, after_step=stepped.append)
    assert calls == list(range(want_steps)) and stepped == calls and env.t == want_steps
    assert tr["steps_run"] == want_steps and float(tr["final_obs"][0, 0]) == float(want_steps)
    assert all(torch.equal(s, torch.from_numpy(chosen[t])) for t, s in enumerate(env.seen))
    got = {k: tr[k].numpy() for k in ("reward", "done", "info", "action")}
    assert {k: (v.shape, v.dtype) for k, v in got.items()} == dict(
        reward=((want_steps, n), np.float32), done=((want_steps, n), np.uint8), info=((want_steps, n), np.uint8), action=((want_steps, n), np.int32))
    # every entry is what an episode launch writes: the script's, with the policy's actions for the live envs
    alive_before = np.arange(want_steps)[:, None] < ends[None, :]
    assert got["reward"].tobytes() == script["reward"][:want_steps].tobytes()
    assert np.array_equal(got["done"], script["done"][:want_steps])
    assert np.array_equal(got["info"], script["info"][:want_steps])
    assert np.array_equal(got["action"], np.where(alive_before, chosen[:want_steps], -1))
    dead = ~alive_before
    assert dead.any() and (got["reward"][dead] == 0).all() and (got["done"][dead] == 1).all() and (got["action"][dead] == -1).all()
    etab = energy_table(SHIPPED_A, SHIPPED_W)
    scripted = dict(script, action=np.where(np.arange(120)[:, None] < ends[None, :], chosen, -1).astype(np.int32))
    scripted = {k: v[:max_steps] for k, v in scripted.items()}
    _assert_tally_equal(tally(got["reward"], got["done"], got["info"], got["action"], 0.99, etab),
                        tally(scripted["reward"], scripted["done"], scripted["info"], scripted["action"], 0.99, etab))
    want, _ = _loop_restated(scripted["reward"], scripted["done"], scripted["info"], scripted["action"], 0.99, etab)
    _assert_tally_equal(tally(got["reward"], got["done"], got["info"], got["action"], 0.99, etab), want)


@pytest.mark.parametrize("past_T", [True, False])
def test_sweep_record_builder(past_T):
    from distributional_rl_navigation_amd.experiments import _records_from_traces
    names, num = ("adaptive_IQN", "DQN", "APF"), 8
    tr, ends = _traces(7, n=len(names) * num, past_T=past_T)
    params = SimpleNamespace(discount=0.99, a=SHIPPED_A, w=SHIPPED_W, dt=0.05, N=5)
    want, live = _loop_restated(tr["reward"], tr["done"], tr["info"], tr["action"], 0.99, _torch_energy_table(SHIPPED_A, SHIPPED_W).numpy(),
                                groups=len(names))
    steps = len(live)
    total = int(want["length"].sum())
    step_s = {name: [1e-6 * (1 + t) + 1e-3 * p for t in range(steps)] for p, name in enumerate(names)}
    by_launch = _records_from_traces(tr, params, names, num, launch_s=0.25)
    by_step = _records_from_traces(tr, params, names, num, step_s=step_s)
    assert list(by_launch) == list(names) == list(by_step)
    for p, name in enumerate(names):
        sl = slice(p * num, (p + 1) * num)
        for rec in (by_launch[name], by_step[name]):
            assert rec["reward"] == [float(v) for v in want["ret"][sl]] and rec["energy"] == [float(v) for v in want["energy"][sl]]
            assert rec["time"] == [float(0.05 * 5 * l) for l in want["length"][sl]]
            assert rec["success"] == [bool(v) for v in want["last_info"][sl] == 4]
            assert rec["out_of_area"] == [bool(v) for v in want["last_info"][sl] == 1]
            assert rec["actions"] == want["actions"][sl]
            assert len(rec["computation_times"]) == int(want["length"][sl].sum())      # one entry per step of every episode, either way
        assert by_launch[name]["computation_times"] == [0.25 / total] * int(want["length"][sl].sum())
        # step t appears once per env alive before it, counted step by step in the restated loop
        assert by_step[name]["computation_times"] == [step_s[name][t] for t in range(steps) for _ in range(live[t][p])]
        assert [int((want["length"][sl] > t).sum()) for t in range(steps)] == [live[t][p] for t in range(steps)]
    assert sum(len(r["computation_times"]) for r in by_launch.values()) == total == sum(len(r["computation_times"]) for r in by_step.values())
