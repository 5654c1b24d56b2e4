"""The n-step window append as one HIP launch (`mn_replay_append_nstep`, csrc/replay.hip) against the torch ops it replaces
(`ReplayBuffer._nstep_window` + `add_batch`, which test_replay_nstep_cpu.py holds to a plain restatement of the rule): every tensor bit for bit after
every add, in both modes; the refusals; states moving between the two paths; a whole agent and a stopped-and-resumed `train_iqn --n-step 3
--n-step-mode episode` run."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import replay_nstep_cases as H      # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = ("reference", "episode")


@pytest.fixture(scope="module")
def torch():
    import torch as t
    if not t.cuda.is_available():
        pytest.skip("no GPU")
    return t


def _ring(capacity, n_step, mode, kernel, seed=5):
    from distributional_rl_navigation_amd.iqn.replay_buffer import ReplayBuffer
    buf = ReplayBuffer(capacity, 8, DEV, seed=seed, gamma=H.GAMMA, n_step=n_step, nstep_mode=mode)
    buf.use_nstep_kernel = kernel
    return buf


def _device_stream(torch, stream):
    """The arrays of `make_stream` on the device, in the dtypes the HIP env hands to `add_vector_step`."""
    return tuple(torch.from_numpy(x).to(DEV) for x in stream)


def _add(buf, dev, t):
    obs, act, rew, nxt, dn = dev
    buf.add_vector_step(obs[t], act[t], rew[t], nxt[t], dn[t])


def _capacities(k):
    """A ring that one launch wraps in (k + k // 3 + 1 rows: the second emitting call already crosses its end; a single stream wraps between calls), and
    -- four streams and more -- one smaller than a call (k - 3: only the newest rows survive)."""
    return [k + k // 3 + 1] + ([k - 3] if k > 3 else [])


@pytest.mark.parametrize("n_step", [2, 3, 5, 16])
@pytest.mark.parametrize("k", [1, 20, 257])      # 20 rows x 13 float2 straddle a 256-lane block; 257 leaves a partial block
@pytest.mark.parametrize("mode", MODES)
def test_kernel_equals_the_torch_window_after_every_add(torch, mode, k, n_step):
    """3 n + 2 adds; every done pattern (random p = 0.25, none, all, newest slot only, head only, two in a window); both capacities: the five ring tensors,
    every window tensor, the window's count, ptr and size are EQUAL after every add.  Rewards: standard normal with -0.0, 1e-30 and 3e38 * 0.3 planted."""
    adds = 3 * n_step + 2
    for p, pattern in enumerate(H.DONE_PATTERNS):
        stream = H.make_stream(adds, k, n_step, pattern, seed=1000 * n_step + 10 * k + p)
        dev = _device_stream(torch, stream)
        for capacity in _capacities(k):
            a, b = _ring(capacity, n_step, mode, kernel=True), _ring(capacity, n_step, mode, kernel=False)
            for t in range(adds):
                _add(a, dev, t); _add(b, dev, t)
                H.same_rings(a, b)
            assert a.size == min(capacity, k * (adds - n_step + 1)) and a._hist["count"] == adds
            if k == 20 and n_step == 3 and capacity > k:      # ... and the torch path on the device is the rule itself (the CPU test's restatement)
                plain = H.PlainNstep(capacity, k, n_step, mode)
                for t in range(adds):
                    plain.add(H.rows_of(stream, t))
                H.same_as_plain(a, plain)


def test_refusals_launch_nothing(torch):
    """MN_ERR_INVALID for NULL pointers, n_step outside 2..16, a bad ptr or capacity, an unknown mode, episode mode without its two window arrays: ring and
    window untouched."""
    from distributional_rl_navigation_amd import _capi
    lib, k, n = _capi.lib(), 20, 3
    dev = _device_stream(torch, H.make_stream(1, k, n, "all", seed=4))
    batch = [x[0].contiguous() for x in dev]
    buf = _ring(64, n, "episode", kernel=True)
    h = buf._window(k, 26)
    for t in [t for key, t in h.items() if key != "count"] + [getattr(buf, name) for name in H.RING]:
        t.fill_(3)
    held = [t.clone() for key, t in h.items() if key != "count"] + [getattr(buf, name).clone() for name in H.RING]
    g = _capi.MnNstepGamma()
    for i in range(n):
        g.g[i] = H.GAMMA ** i
    p = lambda t: C.c_void_p(t.data_ptr())
    ptrs = [p(t) for t in batch] + [p(h[key]) for key in ("s", "a", "r", "ns", "d")]
    ring = [p(getattr(buf, name)) for name in H.RING]

    def call(ptrs=ptrs, count=2, n_step=n, mode=_capi.NSTEP_EPISODE, ring=ring, k=k, ptr=0, capacity=64):
        return lib.mn_replay_append_nstep(*ptrs, count, n_step, g, mode, *ring, k, ptr, capacity, _capi.stream_ptr(buf.device))

    without = lambda seq, i: [None if j == i else x for j, x in enumerate(seq)]
    rcs = [call(ptrs=without(ptrs, i)) for i in range(10)]                                  # each batch / window pointer NULL (episode mode needs all ten)
    rcs += [call(ring=without(ring, i)) for i in range(5)]
    rcs += [call(n_step=v) for v in (1, 0, -2, 17, 1 << 20)]
    rcs += [call(ptr=-1), call(ptr=64), call(capacity=0), call(capacity=-5), call(k=0), call(k=-1), call(count=-1), call(mode=2), call(mode=-1)]
    torch.cuda.synchronize()
    assert rcs == [-1] * len(rcs)      # MN_ERR_INVALID
    now = [t for key, t in h.items() if key != "count"] + [getattr(buf, name) for name in H.RING]
    assert all(torch.equal(x, y) for x, y in zip(held, now))
    # reference mode takes the call without the two episode arrays: the window holds rewards 3, 3 in front of this call's
    assert call(ptrs=without(without(ptrs, 8), 9), mode=_capi.NSTEP_REFERENCE) == 0
    torch.cuda.synchronize()
    older = float(np.float32(np.float32(3) + np.float32(np.float32(H.GAMMA) * np.float32(3))))
    assert torch.equal(buf.rewards[:k, 0], batch[2] * float(np.float32(H.GAMMA ** 2)) + older)
    assert torch.equal(buf.rewards[k:], held[-2][k:]) and torch.equal(h["ns"], held[3]) and torch.equal(h["d"], held[4])


@pytest.mark.parametrize("mode", MODES)
def test_a_state_moves_between_the_kernel_and_the_torch_path(torch, mode):
    """state_dict() of a ring on one path, inside the filling window and again behind a wrap, continues on a ring of the other path: equal emissions."""
    k, n, adds = 20, 3, 12
    dev = _device_stream(torch, H.make_stream(adds, k, n, "random", seed=8))
    straight = _ring(90, n, mode, kernel=False)
    for t in range(adds):
        _add(straight, dev, t)
    for first_kernel in (True, False):
        a = _ring(90, n, mode, kernel=first_kernel)
        switch_at = (2, 7)      # inside the first window; after 5 emitting calls = 100 rows into 90
        for t in range(adds):
            if t in switch_at:
                b = _ring(90, n, mode, kernel=not a.use_nstep_kernel, seed=99)
                b.load_state_dict(a.state_dict())
                a = b
            _add(a, dev, t)
        H.same_rings(a, straight)


def _agent_run(torch, mode, kernel, n_envs=64, steps=12):
    """(agent, its network's parameters) behind `steps` vector steps of learn_vec."""
    from distributional_rl_navigation_amd.iqn.agent import IQNAgent
    from distributional_rl_navigation_amd.marinenav_env.vec_env import VecMarineNavEnv
    env = VecMarineNavEnv(n_envs, seed=3, device=DEV, precision="f64")
    env.params.max_episode_steps = 4      # every episode ends inside a window: at the latest by time-out, behind its 4th step
    env.set_attrs(min_start_goal_dis=30.0)
    ag = IQNAgent(26, 9, n_step=3, n_step_mode=mode, BATCH_SIZE=32, BUFFER_SIZE=1024, device=DEV, seed=1, learning_starts=0, UPDATE_EVERY=1)
    ag.memory.use_nstep_kernel = kernel
    ag.learn_vec(total_vector_steps=steps, train_env=env, verbose=False)
    torch.cuda.synchronize()
    params = torch.cat([p.detach().reshape(-1).clone() for p in ag.qnetwork_local.parameters()])
    env.close()
    return ag, params


@pytest.mark.parametrize("mode", MODES)
def test_agent_with_and_without_the_kernel(torch, mode):
    """IQNAgent(n_step = 3) on 64 envs, 12 vector steps of learn_vec from the same seeds: ring, window and network parameters are bit-equal."""
    a, pa = _agent_run(torch, mode, True)
    b, pb = _agent_run(torch, mode, False)
    assert a.memory.size == 64 * 10 and a.grad_steps == b.grad_steps >= 4 and a.memory._hist["count"] == 12
    assert float(a.memory.dones[:a.memory.size].sum()) > 0
    H.same_rings(a.memory, b.memory)
    assert torch.equal(pa, pb)


# ---- the trainer: --n-step 3 --n-step-mode episode, stopped and resumed in a fresh process --------------------------------------------------
ARGS = ["--n-envs", "64", "--batch", "32", "--replay", "4096", "--grad-steps", "1", "--total-grad-steps", "60", "--n-evals", "3", "--eval-worlds", "3",
        "--max-eval-steps", "40", "--n-step", "3", "--n-step-mode", "episode"]      # tests/test_resume_gpu.py's learner case: 60 vector steps of 64 envs


def _train(cwd, *extra):
    os.makedirs(cwd, exist_ok=True)
    with open(os.path.join(cwd, "config.json"), "w") as f:
        json.dump(dict(agent="IQN", seed=3, save_dir="runs", total_timesteps=2000, eval_freq=500), f)
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    cmd = [sys.executable, "-m", "distributional_rl_navigation_amd.train_iqn", "-C", "config.json", "-D", DEV, "--run-name", "toy", *ARGS, *extra]
    r = subprocess.run(cmd, cwd=cwd, env=env, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, (cmd, r.stdout[-1500:], r.stderr[-3000:])
    return r.stdout


def _same(x, y, path):
    import torch as t
    if isinstance(x, dict):
        assert isinstance(y, dict) and x.keys() == y.keys(), path
        for key in x:
            _same(x[key], y[key], f"{path}.{key}")
    elif isinstance(x, (list, tuple)):
        assert type(x) is type(y) and len(x) == len(y), path
        for i, (a, b) in enumerate(zip(x, y)):
            _same(a, b, f"{path}[{i}]")
    elif t.is_tensor(x):
        assert t.is_tensor(y) and x.dtype == y.dtype and x.shape == y.shape and x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes(), path
    elif isinstance(x, np.ndarray):
        if x.dtype == object:
            _same(x.tolist(), y.tolist(), path)
        else:
            assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), path
    elif isinstance(x, float) and x != x:
        assert y != y, path
    else:
        assert x == y, (path, x, y)


def _same_file(a, b, name):
    import torch as t
    if name.endswith(".npz"):
        za, zb = np.load(a, allow_pickle=True), np.load(b, allow_pickle=True)
        assert sorted(za.files) == sorted(zb.files), name
        for key in za.files:
            _same(za[key], zb[key], f"{name}:{key}")
    elif name.endswith((".pth", ".pt")):
        _same(t.load(a, map_location="cpu", weights_only=False), t.load(b, map_location="cpu", weights_only=False), name)
    elif name.endswith(".json"):
        with open(a) as f, open(b) as g:
            _same(json.load(f), json.load(g), name)
    else:
        with open(a, "rb") as f, open(b, "rb") as g:
            assert f.read() == g.read(), name


def test_trainer_in_episode_mode_stopped_and_resumed_writes_the_files_of_the_straight_run(torch, tmp_path):
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    seed_a, seed_b = (os.path.join(d, "runs", "training_toy", "seed_3") for d in (a, b))
    _train(a, "--dump-final-state", "final.pt")
    out = _train(b, "--stop-after", "31")      # (31 = 3 * 10 + 1: the window's write slot is not 0 at the stop)
    assert "stopped after vector step 31 of 60" in out
    ck = torch.load(os.path.join(seed_b, "checkpoint.pt"), map_location="cpu", weights_only=False)
    assert ck["args"]["n_step"] == 3 and ck["args"]["n_step_mode"] == "episode" and ck["ring"]["nstep_mode"] == "episode"
    assert sorted(ck["ring"]["hist"]) == ["a", "count", "d", "ns", "r", "s"] and ck["ring"]["hist"]["count"] == 31 and ck["ring"]["size"] == 64 * 29
    out = _train(b, "--resume", os.path.join("runs", "training_toy"), "--dump-final-state", "final.pt")
    assert "continuing from vector step 31 (checkpoint.pt)" in out
    files_a = sorted(os.listdir(seed_a))
    assert {"completed.json", "network_params.pth", "greedy_evaluations.npz", "trial_config.json"} <= set(files_a)
    assert sorted(set(os.listdir(seed_b)) - {"checkpoint.pt", "checkpoint.prev.pt"}) == files_a
    for f in files_a:
        _same_file(os.path.join(seed_a, f), os.path.join(seed_b, f), f)
    _same_file(os.path.join(a, "final.pt"), os.path.join(b, "final.pt"), "final.pt")
    final = torch.load(os.path.join(a, "final.pt"), map_location="cpu", weights_only=False)
    assert final["ring"]["size"] == 64 * 58 and float(final["ring"]["dones"].sum()) > 0
