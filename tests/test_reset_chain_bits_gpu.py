"""The episode reset's short-chain forms (csrc/mn_reset_body.h: the RNG block as doubles in LDS, accepted cores / obstacles in registers, branch-free pair
tests, the start velocity across lanes) generate what the reset always generated.

References: the CPU twin of the C-ABI (oracle/libmarinenav_cpu.so, driven through tests/test_cpu_twin.py's Driver as the other reset tests do) for world
tables, counts, start / goal, pose and the position of every RNG stream, bit for bit, and for the first observations to the tolerance those tests use (the
twin's libm is not the device's); and, byte for byte in everything incl. the MT19937 rows, `mt_pos`, the compact tables and the float32 observation rows, the
four launches that run the body against one another -- mn_reset, mn_reset_done (queue-driven), the reset owed to the next act call's preparation launch
(`reset_done(under_next_act=True, eps=1.0)` + `act_batch(..., late_env=env)`) and the reset under the act kernel, whose kernel keeps the earlier forms
(MtInPlace, accepted objects in LDS, branching pair tests).

Shapes: 64 and 200 envs (200 is no multiple of 64), both precisions, world sizes (8, 10), (8, 5), (4, 6); four consecutive resets of every env behind the
first one.  Plus what the new forms can get wrong: rejection batches of each kind that begin 0, 2, 4 and 6 words in front of a block boundary, resets that
cross several block boundaries and loops that run out of their 500 tries (tests/params_sets.py R1, R3, R5), worlds without cores / without obstacles, and a
curriculum stage change between two resets."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import params_sets as PS      # noqa: E402
import test_cpu_twin as TW    # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ALWAYS = 2 ** 31 - 1
ROUNDS = 4
PATHS = ("reset", "reset_done", "owed", "under_act")
RAW = ("mt", "mt_pos", "qcx", "qcy", "qcg", "qox", "qoy", "qor")
OBS_ATOL = {"f64": 1e-10, "mixed": 1e-5}      # first observation against the twin (tests/test_env_gpu.py)


@pytest.fixture(scope="module")
def torch():
    import torch as t
    if not t.cuda.is_available():
        pytest.skip("no GPU")
    return t


@pytest.fixture(scope="module")
def agent(torch):
    from distributional_rl_navigation_amd.iqn.agent import IQNAgent
    return IQNAgent(26, 9, device=DEV, seed=4)


def _env(n, precision, spec, path=None, seed=3, schedule=None):
    from distributional_rl_navigation_amd import _capi
    from distributional_rl_navigation_amd.marinenav_env.vec_env import VecMarineNavEnv
    env = VecMarineNavEnv(n, seed=seed, device=DEV, precision=precision, obs64=precision == "f64", params=PS.apply(_capi.default_params(), spec),
                          schedule=schedule)
    if "start" in spec:
        env.set_start_goal(spec["start"], spec["goal"])
    if path == "owed":
        env.set_reset_owed_max_rows(ALWAYS)      # whatever eps and the episode count: left to the next act call's preparation launch
    if path == "under_act":
        env.set_reset_under_act_max(ALWAYS)      # however many episodes end: under the act kernel
    return env


def _twin(n, seeds, spec, schedule=None):
    d = TW.numpy_driver(TW.bind(TW.TWIN), n, seeds=seeds)
    PS.driver_set(d, spec)
    if schedule is not None:
        ts = np.ascontiguousarray(schedule["timesteps"], np.int64); nc = np.ascontiguousarray(schedule["num_cores"], np.int32)
        no = np.ascontiguousarray(schedule["num_obstacles"], np.int32); md = np.ascontiguousarray(schedule["min_start_goal_dis"], np.float64)
        assert d.L.mn_set_schedule(d.h, len(ts), ts.ctypes.data_as(C.POINTER(C.c_int64)), nc.ctypes.data_as(C.POINTER(C.c_int32)),
                                   no.ctypes.data_as(C.POINTER(C.c_int32)), md.ctypes.data_as(C.POINTER(C.c_double)), 1.0) == 0
    return d


def _twin_snapshot(d, obs):
    w = d.worlds()
    return dict(w=w, peek=d.peek(), state=d.state()[0], obs=obs)


def _gpu_snapshot(torch, env):
    """Everything a reset writes, as host arrays."""
    torch.cuda.synchronize()
    n = env.n_envs
    worlds = env.get_worlds()
    out = dict(worlds=[(w["cores"], w["obstacles"], w["start"], w["goal"], np.float64(w["init_theta"]), np.float64(w["init_speed"])) for w in worlds],
               peek=env.peek_next_double(), state=env.get_state()[0], obs=env.obs.cpu().numpy())
    if env.obs64_enabled:
        out["obs64"] = env.get_obs64()
    for k in RAW:
        a = env.debug_read(k)
        out[k] = a[:n] if k in ("mt", "mt_pos") else a[:, :n]      # (the rows of real envs: padding rows are never written)
    return out


def _against_twin(g, t, precision):
    """Tables, counts, start / goal, pose and stream position bit for bit; velocity and first observation to the twin's libm."""
    w = t["w"]
    for i, (cores, obst, start, goal, th, sp) in enumerate(g["worlds"]):
        nc, no = int(w["ncores"][i]), int(w["nobs"][i])
        assert cores.shape[0] == nc and obst.shape[0] == no, (i, cores.shape, nc, obst.shape, no)
        assert cores.tobytes() == np.ascontiguousarray(w["cores"][i, :nc]).tobytes(), i
        assert obst.tobytes() == np.ascontiguousarray(w["obstacles"][i, :no]).tobytes(), i
        assert start.tobytes() == w["start"][i].tobytes() and goal.tobytes() == w["goal"][i].tobytes(), i
        assert th.tobytes() == w["theta0"][i].tobytes() and sp.tobytes() == w["speed0"][i].tobytes(), i
    assert g["peek"].tobytes() == t["peek"].tobytes()
    assert g["state"][:, :4].tobytes() == np.ascontiguousarray(t["state"][:, :4]).tobytes()
    np.testing.assert_allclose(g["state"][:, 4:], t["state"][:, 4:], rtol=0, atol=1e-9)
    np.testing.assert_allclose(g["obs64"] if "obs64" in g else g["obs"], t["obs"], rtol=0, atol=OBS_ATOL[precision])
    # the compact tables are a function of the float64 ones (MnArrays): 2^-24 m fixed point, float32 signed Gamma / radius, zero behind the count
    n = len(g["worlds"])
    q = {k: np.zeros_like(g[k]) for k in RAW[2:]}
    for i in range(n):
        nc, no = int(w["ncores"][i]), int(w["nobs"][i])
        c, o = w["cores"][i, :nc], w["obstacles"][i, :no]
        q["qcx"][:nc, i] = np.rint(c[:, 0] * 16777216.0).astype(np.int32); q["qcy"][:nc, i] = np.rint(c[:, 1] * 16777216.0).astype(np.int32)
        q["qcg"][:nc, i] = np.where(c[:, 2] != 0, c[:, 3], -c[:, 3]).astype(np.float32)
        q["qox"][:no, i] = np.rint(o[:, 0] * 16777216.0).astype(np.int32); q["qoy"][:no, i] = np.rint(o[:, 1] * 16777216.0).astype(np.int32)
        q["qor"][:no, i] = o[:, 2].astype(np.float32)
    for k in q:
        assert g[k].tobytes() == q[k].tobytes(), k


def _same_bytes(a, b, what):
    assert a.keys() == b.keys(), what
    for k in a:
        if k == "worlds":
            for i, (x, y) in enumerate(zip(a[k], b[k])):
                assert all(p.tobytes() == q.tobytes() for p, q in zip(x, y)), (what, k, i)
        else:
            assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), (what, k)


def _finish_every_env(torch, env):
    """An episode limit of one step: the second step of an episode times out, so every env sits in the done-queue."""
    a = torch.zeros(env.n_envs, dtype=torch.int32, device=DEV)
    env.step(a)
    env.step(a)
    assert int(env.done.sum()) == env.n_envs


def _reset_through(torch, env, agent, path):
    if path == "reset":
        env.reset()
        return
    _finish_every_env(torch, env)
    if path == "reset_done":
        env.reset_done()
    elif path == "owed":
        env.reset_done(under_next_act=True, eps=1.0)
        assert env.reset_owed and env.late_rows is None
        agent.act_batch(env.obs, 1.0, late_env=env)      # its preparation launch runs the resets
        from distributional_rl_navigation_amd import _capi
        assert _capi.lib().mn_reset_is_owed(env.h) == 0
    else:
        env.reset_done(under_next_act=True)
        assert env.late_rows is not None      # it did go under: the kernel with the earlier forms
        env.join_reset()


_TWIN_RUNS = {}


def _twin_run(n, seeds, spec, rounds):
    """The twin's snapshots of `rounds` + 1 consecutive resets of every env, computed once per (n, set)."""
    key = (n, tuple(sorted((k, tuple(v) if isinstance(v, (tuple, list)) else v) for k, v in spec.items())), rounds)
    if key not in _TWIN_RUNS:
        d = _twin(n, seeds, spec)
        snaps = [_twin_snapshot(d, d.reset())]
        for r in range(rounds):
            snaps.append(_twin_snapshot(d, d.reset()))
        d.close()
        _TWIN_RUNS[key] = snaps
    return _TWIN_RUNS[key]


def _run_paths(torch, agent, n, precision, spec, rounds=ROUNDS):
    """rounds + 1 consecutive resets of every env through each path; every snapshot against the twin, and the paths against one another byte for byte."""
    runs = {}
    for path in PATHS:
        env = _env(n, precision, dict(spec, max_episode_steps=1), path)      # (the twin keeps the reference's 1000-step limit: it is reset as a whole)
        ref = _twin_run(n, [int(s) for s in env.seeds], spec, rounds)
        env.reset()
        snaps = [_gpu_snapshot(torch, env)]
        for r in range(rounds):
            _reset_through(torch, env, agent, path)
            snaps.append(_gpu_snapshot(torch, env))
        env.close()
        for r, (g, t) in enumerate(zip(snaps, ref)):
            _against_twin(g, t, precision)
        runs[path] = snaps
    for path in PATHS[1:]:
        for r, (a, b) in enumerate(zip(runs["under_act"], runs[path])):
            _same_bytes(a, b, f"{path} round {r}")
    _same_bytes(runs["under_act"][-1], runs["reset"][-1], "reset last round")      # (mn_reset: not queue-driven, the same streams)
    return runs


@pytest.mark.parametrize("size", [(8, 10), (8, 5), (4, 6)])
@pytest.mark.parametrize("n,precision", [(64, "f64"), (200, "f64"), (64, "mixed"), (200, "mixed")])
def test_four_consecutive_resets_through_every_launch(torch, agent, n, precision, size):
    runs = _run_paths(torch, agent, n, precision, dict(num_cores=size[0], num_obs=size[1], min_start_goal_dis=40.0))
    pos = runs["reset_done"][-1]["mt_pos"]
    first = runs["reset_done"][0]["mt_pos"]
    assert (pos < first).any() or size != (8, 10)      # ~300 words a reset: streams have crossed block boundaries


@pytest.mark.parametrize("size", [(0, 10), (8, 0), (0, 0)])
def test_worlds_without_cores_or_without_obstacles(torch, agent, size):
    runs = _run_paths(torch, agent, 200, "f64", dict(num_cores=size[0], num_obs=size[1], min_start_goal_dis=40.0))
    for cores, obst, *_ in runs["owed"][-1]["worlds"]:
        assert cores.shape[0] == size[0] and obst.shape[0] == size[1]


@pytest.mark.parametrize("name", ["R1", "R3", "R5"])
def test_loops_that_run_out_of_their_500_tries_and_resets_that_cross_several_blocks(torch, agent, name):
    """R1: the start / goal loop takes all 500 tries (4 000 words: six block boundaries in one reset); R3: the core loop gives up short of 8 cores; R5: the
    obstacle loop gives up short of 10 obstacles.  Accepted counts and stream positions are the twin's."""
    spec = dict(PS.RESET_SETS)[name]
    runs = _run_paths(torch, agent, 64, "f64", spec, rounds=2)
    last = runs["owed"][-1]["worlds"]
    if name == "R3":
        assert any(c.shape[0] < spec["num_cores"] for c, *_ in last)
    if name == "R5":
        assert any(o.shape[0] < spec["num_obs"] for _, o, *_ in last)


def _masked(torch, env, d, mask):
    """mn_reset of the masked envs on both sides."""
    if not mask.any():
        return
    env.reset(torch.from_numpy(mask.astype(np.uint8)))
    m = np.ascontiguousarray(mask, np.uint8)
    assert d.L.mn_reset(d.h, m.ctypes.data_as(C.c_void_p), d.ptr(d.obs[d.cur]), None) == 0


def _set_both(env, d, spec):
    PS.vec_env_set(env, spec)
    PS.driver_set(d, spec)


@pytest.mark.parametrize("precision", ["f64", "mixed"])
def test_batches_that_begin_0_2_4_6_words_in_front_of_a_block_boundary(torch, precision):
    """Env e gets its stream to 624 - d words into a block, d = 0, 2, 4, 6, and then runs a reset whose FIRST rejection batch is of kind e // 4 % 3: start /
    goal pairs, cores (start / goal fixed), obstacles (start / goal fixed, no cores).  The stream is moved by resets that draw the pose only (4 words) and,
    for the positions that are 2 mod 4, by resets that place one obstacle (6 words a try + 4); the positions are read back (`mt_pos`), the twin stays in
    lock-step (peek).  Then one more reset of every env: the batch behind the boundary, and the block written back.  (mn_reset with a mask: mn_reset_kernel, which
    inlines the body in the preparation launch's form.)"""
    n = 48
    fixed = dict(reset_start_and_goal=0, start=(5.0, 5.0), goal=(45.0, 45.0), min_start_goal_dis=40.0)
    move4, move6 = dict(fixed, num_cores=0, num_obs=0), dict(fixed, num_cores=0, num_obs=1)
    env = _env(n, precision, move4)
    d = _twin(n, [int(s) for s in env.seeds], move4)
    target = 624 - 2 * (np.arange(n) % 4)
    for it in range(400):
        torch.cuda.synchronize()
        pos = env.debug_read("mt_pos")[:n].astype(np.int64)
        left = (target - pos) % 624
        if not left.any():
            break
        odd = (left % 4 == 2) & (left >= 10)
        _set_both(env, d, move6); _masked(torch, env, d, odd)
        _set_both(env, d, move4); _masked(torch, env, d, ~odd & (left != 0))
    assert not left.any(), left
    assert env.peek_next_double().tobytes() == d.peek().tobytes()
    kinds = [dict(num_cores=8, num_obs=10, min_start_goal_dis=40.0, reset_start_and_goal=1), dict(fixed, num_cores=8, num_obs=10),
             dict(fixed, num_cores=0, num_obs=10)]
    kind = np.arange(n) // 4 % 3
    for again in range(2):
        for k, spec in enumerate(kinds):
            _set_both(env, d, spec)
            _masked(torch, env, d, kind == k)
        g = _gpu_snapshot(torch, env)
        _against_twin(g, _twin_snapshot(d, d.obs64()), precision)
        if again == 0:
            assert (g["mt_pos"] < 624 - 6).all()      # every env's first batch went over the boundary
    env.close(); d.close()


@pytest.mark.parametrize("precision", ["f64", "mixed"])
def test_curriculum_stage_change_between_two_resets(torch, agent, precision):
    """Stage 0 (4 cores, 6 obstacles) until 3 total timesteps, then stage 1 (8, 10): every env has run 2 steps at its second reset and 4 at its third."""
    sched = dict(timesteps=[0, 3], num_cores=[4, 8], num_obstacles=[6, 10], min_start_goal_dis=[30.0, 40.0])
    n = 200
    outs = {}
    for path in PATHS[1:]:
        env = _env(n, precision, dict(max_episode_steps=1), path, schedule=sched)
        d = _twin(n, [int(s) for s in env.seeds], {}, schedule=sched)
        env.reset()
        obs = d.reset()
        snaps = []
        for r in range(3):
            _reset_through(torch, env, agent, path)
            a = np.zeros(n, np.int32)
            d.step(a, d.set_actions); d.step(a, d.set_actions)      # (its total_timesteps count them; its 1000-step limit ends no episode: mn_reset)
            obs = d.reset()
            g = _gpu_snapshot(torch, env)
            _against_twin(g, _twin_snapshot(d, obs), precision)
            snaps.append(g)
        counts = [sorted({(c.shape[0], o.shape[0]) for c, o, *_ in s["worlds"]}) for s in snaps]
        assert counts[0] == [(4, 6)] and counts[1] == [(8, 10)] and counts[2] == [(8, 10)], counts
        outs[path] = snaps
        env.close(); d.close()
    for path in ("reset_done", "owed"):
        for r, (a, b) in enumerate(zip(outs["under_act"], outs[path])):
            _same_bytes(a, b, f"{path} round {r}")
