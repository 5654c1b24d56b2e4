"""Snapshot and restore of an env handle (csrc/mn_state.hip; C-ABI mn_state_bytes / mn_state_save / mn_state_load; `VecMarineNavEnv.save_state`, `load_state`,
`state_dict`, `load_state_dict`): a handle put back from a blob behaves exactly as the saved one would have.  Every comparison is byte for byte.

192 envs (the handle pads its rows to 256, the blob does not), both precisions.  max_episode_steps = 15 and a two-stage schedule that changes at total timestep
28 put time-outs (steps 15 and 30), collisions and a stage change inside the 40-step window; the save is made after step 20."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ALWAYS = 2 ** 31 - 1
N, T, SAVE_AT, ACTION_SEED = 192, 40, 20, 77
SCHEDULE = dict(timesteps=[0, 28], num_cores=[4, 8], num_obstacles=[3, 10], min_start_goal_dis=[20.0, 35.0])
RAW = ("mt", "mt_pos", "qcx", "qcy", "qcg", "qox", "qoy", "qor")


@pytest.fixture(scope="module")
def torch():
    import torch as t
    if not t.cuda.is_available():
        pytest.skip("no GPU")
    return t


def _env(precision, seed=3, n=N, max_episode_steps=15):
    from distributional_rl_navigation_amd.marinenav_env.vec_env import VecMarineNavEnv
    env = VecMarineNavEnv(n, seed=seed, device=DEV, precision=precision, schedule=SCHEDULE)
    env.params.max_episode_steps = max_episode_steps
    env.set_attrs(min_start_goal_dis=30.0)
    env.reset()
    return env


def _steps(env, t0, t1, debt_at=None, debt=None, save_every=False):
    """Vector steps [t0, t1) of mn_random_actions -> mn_step -> mn_reset_done, every output as host arrays.  `debt_at`: the reset of that step is asked for with
    under_next_act=True and a snapshot is taken right behind it (returned); `save_every`: a snapshot after every step."""
    out, blob, scratch = [], None, None
    for t in range(t0, t1):
        env.step(env.random_actions(ACTION_SEED, t))
        rec = dict(reward=env.reward.cpu().numpy(), done=env.done.cpu().numpy(), info=env.info.cpu().numpy())
        if t == debt_at:
            env.reset_done(under_next_act=True, eps=0.9)
            assert (env.reset_owed, env.late_rows is not None) == ((True, False) if debt == "owed" else (False, True)), (env.reset_owed, env.late_rows)
            blob = env.save_state()
            assert not env.reset_owed and env.late_rows is None
        else:
            env.reset_done()
        if save_every:
            scratch = env.save_state(scratch)
        rec["obs"] = env.obs.cpu().numpy()
        out.append(rec)
    return out, blob


def _end(env):
    state, ep_t, tot_t = env.get_state()
    out = dict(state=state, ep_t=ep_t, tot_t=tot_t, peek=env.peek_next_double(),
               worlds=[[w["cores"], w["obstacles"], w["start"], w["goal"], np.float64(w["init_theta"]), np.float64(w["init_speed"])] for w in env.get_worlds()])
    for k in RAW:
        a = env.debug_read(k)
        out[k] = a[:env.n_envs] if k in ("mt", "mt_pos") else a[:, :env.n_envs]      # (the rows of real envs: padding rows are never read)
    return out


def _equal(x, y, path=""):
    if isinstance(x, dict):
        assert x.keys() == y.keys(), path
        for k in x:
            _equal(x[k], y[k], f"{path}.{k}")
    elif isinstance(x, (list, tuple)):
        assert len(x) == len(y), path
        for i, (a, b) in enumerate(zip(x, y)):
            _equal(a, b, f"{path}[{i}]")
    elif isinstance(x, np.ndarray):
        assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), path      # byte for byte
    else:
        assert x == y, path


_STRAIGHT = {}


def _straight(torch, precision):
    """The uninterrupted run: all 40 steps, the end state, and the blob of step 20 (kept on the host)."""
    if precision not in _STRAIGHT:
        env = _env(precision)
        first, _ = _steps(env, 0, SAVE_AT)
        blob = env.save_state()
        sd = env.state_dict()
        rest, _ = _steps(env, SAVE_AT, T)
        _STRAIGHT[precision] = dict(steps=first + rest, end=_end(env), blob=blob.cpu(), state_dict=sd)
        env.close()
    return _STRAIGHT[precision]


@pytest.mark.parametrize("precision", ["f64", "mixed"])
def test_window_has_resets_timeouts_and_a_stage_change(torch, precision):
    ref = _straight(torch, precision)
    infos = np.stack([s["info"] for s in ref["steps"][SAVE_AT:]])
    dones = np.stack([s["done"] for s in ref["steps"][SAVE_AT:]])
    assert (infos == 2).any() and (infos == 3).any() and 0 < dones.sum() < dones.size      # "too long episode", "collision"
    sizes = {(w[0].shape[0], w[1].shape[0]) for w in ref["end"]["worlds"]}
    assert (8, 10) in sizes      # worlds of the second stage (generated after total timestep 28) -- smaller ones only where obstacles could not be placed
    assert ref["blob"].numel() == 1024 + N * 2496 + 2 * 1024 * 4 + 32 * 64 * 4 + 67 * N * 8 + 57 * N * 4      # compact over n, not the padded 256


@pytest.mark.parametrize("precision", ["f64", "mixed"])
def test_done_queue_lists_are_canonical_in_the_blob(torch, precision):
    """The step kernel's waves append to a shard's list in the order they reach its counter, and entries of earlier steps stay behind the count: wave timing, not
    state.  The blob holds, per shard, the live entries of the half the last step filled in ascending order and zeros behind them -- so it is a function of the
    history (which `test_replay_after_load_into_the_same_handle` relies on when it compares blobs of two runs)."""
    env = _env(precision)
    for t in range(20):      # up to the step at which every env that did not collide before runs into max_episode_steps: three shards of up to 64 entries, pushed by racing waves
        steps, _ = _steps(env, t, t + 1)
        if int(steps[-1]["done"].sum()) > N // 2:
            break
    blob = env.save_state().cpu()
    env.close()
    q = blob.numpy()[1024 + N * 2496:][:2 * 1024 * 4 + 32 * 64 * 4].view(np.int32)
    counts, lists = q[:2048].reshape(2, 32, 32)[:, :, 0], q[2048:].reshape(32, 64)
    finished = np.flatnonzero(steps[-1]["done"])
    assert len(finished) > N // 2
    live = [h for h in (0, 1) if int(counts[h].sum()) == len(finished)]
    assert live, (counts.sum(axis=1), len(finished))
    c = counts[live[-1]]
    listed = []
    for sh in range(32):
        row = lists[sh]
        assert (row[c[sh]:] == 0).all() and (np.diff(row[:c[sh]]) > 0).all(), (sh, c[sh], row)
        assert all((e >> 6) % 32 == sh for e in row[:c[sh]])
        listed += row[:c[sh]].tolist()
    assert sorted(listed) == finished.tolist()


@pytest.mark.parametrize("precision", ["f64", "mixed"])
def test_replay_after_load_into_the_same_handle(torch, precision):
    ref = _straight(torch, precision)
    env = _env(precision)
    _steps(env, 0, SAVE_AT)
    blob = env.save_state()
    # the blob is a function of the history: everything in it is, the done-queue's lists because the save writes them in a canonical order (see above)
    assert blob.cpu().numpy().tobytes() == ref["blob"].numpy().tobytes()
    went_on, _ = _steps(env, SAVE_AT, T)
    _equal(went_on, ref["steps"][SAVE_AT:], "went on")
    env.load_state(blob)
    again, _ = _steps(env, SAVE_AT, T)
    _equal(again, ref["steps"][SAVE_AT:], "replayed")
    _equal(_end(env), ref["end"], "end")
    env.close()


@pytest.mark.parametrize("precision", ["f64", "mixed"])
@pytest.mark.parametrize("via", ["blob", "state_dict"])
def test_replay_after_load_into_a_fresh_handle_with_another_seed(torch, precision, via):
    ref = _straight(torch, precision)
    env = _env(precision, seed=99)
    if via == "blob":
        env.load_state(ref["blob"])
    else:
        env.load_state_dict(ref["state_dict"])
        assert env.obs.cpu().numpy().tobytes() == ref["steps"][SAVE_AT - 1]["obs"].tobytes()
        assert env.reward.cpu().numpy().tobytes() == ref["steps"][SAVE_AT - 1]["reward"].tobytes()
    again, _ = _steps(env, SAVE_AT, T)
    _equal(again, ref["steps"][SAVE_AT:], "replayed")
    _equal(_end(env), ref["end"], "end")
    env.close()


@pytest.mark.parametrize("precision", ["f64", "mixed"])
@pytest.mark.parametrize("debt", ["owed", "under"])
def test_save_with_a_reset_still_to_run(torch, precision, debt):
    """The save comes right behind reset_done(under_next_act=True): with the reset owed to the next act call (nothing launched yet), and with it running on the
    handle's own stream.  The save settles either first; the blob is that of a run whose reset ran in front."""
    from distributional_rl_navigation_amd import _capi
    ref = _straight(torch, precision)
    env = _env(precision)
    if debt == "owed":
        env.set_reset_owed_max_rows(ALWAYS)
    else:
        env.set_reset_under_act_max(ALWAYS)
    first, blob = _steps(env, 0, SAVE_AT, debt_at=SAVE_AT - 1, debt=debt)
    assert _capi.lib().mn_reset_is_owed(env.h) == 0
    _equal(first, ref["steps"][:SAVE_AT], "before the save")
    went_on, _ = _steps(env, SAVE_AT, T)
    _equal(went_on, ref["steps"][SAVE_AT:], "went on")
    _equal(_end(env), ref["end"], "end")
    fresh = _env(precision, seed=99)
    fresh.load_state(blob)
    again, _ = _steps(fresh, SAVE_AT, T)
    _equal(again, ref["steps"][SAVE_AT:], "replayed")
    _equal(_end(fresh), ref["end"], "end of the replay")
    env.close()
    fresh.close()


@pytest.mark.parametrize("precision", ["f64", "mixed"])
def test_saving_is_read_only(torch, precision):
    ref = _straight(torch, precision)
    env = _env(precision)
    steps, _ = _steps(env, 0, T, save_every=True)
    _equal(steps, ref["steps"], "steps")
    _equal(_end(env), ref["end"], "end")
    env.close()


def test_refusals_leave_the_handle_untouched(torch):
    from distributional_rl_navigation_amd import _capi
    L = _capi.lib()
    env = _env("f64")
    _steps(env, 0, 5)
    good = env.save_state()
    before = _end(env)
    others = {"another n": _env("f64", n=256), "another precision": _env("mixed"), "other params": _env("f64", max_episode_steps=16)}
    cases = {k: (e.save_state(), None) for k, e in others.items()}
    cases["one byte short"] = (good, good.numel() - 1)
    bad_magic = good.clone()
    bad_magic[0] ^= 0xFF
    cases["bad magic"] = (bad_magic, None)
    expect = {"another n": "n = 256", "another precision": "precision", "other params": "params.max_episode_steps", "one byte short": "bytes", "bad magic": "magic"}
    for name, (blob, nbytes) in cases.items():
        rc = L.mn_state_load(env.h, C.c_void_p(blob.data_ptr()), int(blob.numel() if nbytes is None else nbytes), env._stream())
        msg = L.mn_last_error(env.h).decode()
        assert rc == -1 and expect[name] in msg, (name, rc, msg)
        with pytest.raises(_capi.MarineNavHipError):
            env.load_state(blob if nbytes is None else blob[:nbytes])
        _equal(_end(env), before, name)
    assert L.mn_state_load(env.h, None, int(good.numel()), env._stream()) == -1 and L.mn_last_error(env.h)
    assert L.mn_state_save(env.h, None, int(good.numel()), env._stream()) == -1 and L.mn_last_error(env.h)
    assert L.mn_state_save(env.h, C.c_void_p(good.data_ptr()), int(good.numel()) - 1, env._stream()) == -1
    assert L.mn_state_bytes(None) == -1 and L.mn_state_bytes(env.h) == good.numel()
    env.load_state(good)      # ... and the good one still loads
    _equal(_end(env), before, "good")
    for e in list(others.values()) + [env]:
        e.close()


# ---- the whole trainer: stop, resume in a fresh process, compare with the uninterrupted run -----------------------------------------------
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STOP, EVERY = 30, 25
COMMON = ["--eval-worlds", "3", "--max-eval-steps", "40"]
# learner budget: 60 vector steps of 64 envs, one batch-32 gradient step behind each, inline evaluations behind steps 20 / 40 / 60
LEARNER = dict(config=dict(total_timesteps=2000, eval_freq=500), vector_steps=60,
               args=["--n-envs", "64", "--batch", "32", "--replay", "4096", "--grad-steps", "1", "--total-grad-steps", "60", "--n-evals", "3"])
# reference budget at toy size: 60 vector steps of 16 env steps, 4 gradient steps behind each from learning_starts on, deferred evaluations, the full episode log
REFERENCE = dict(config=dict(total_timesteps=960, eval_freq=320), vector_steps=60, args=["--env-budget", "reference", "--n-envs", "16", "--episode-log", "full"])
CASES = {
    "learner": dict(LEARNER),
    # learning starts at vector step 40: the stop falls before it, with an empty optimizer and no evaluation taken yet
    "reference_before_learning_starts": dict(REFERENCE, args=REFERENCE["args"] + ["--reference", "learning_starts=640", "target_update_interval=160", "replay=4096"]),
    # learning from vector step 10 on, a target copy every 10 vector steps (the stop follows the second), eps still on its ramp (48 vector steps long)
    "reference_after_target_copy_inside_eps_ramp": dict(REFERENCE, args=REFERENCE["args"] + ["--reference", "learning_starts=160", "target_update_interval=160",
                                                                                             "exploration_fraction=0.8", "replay=4096"]),
    # the PyTorch gradient step, with 3-step returns (the ring's per-stream window is part of the state; step + append as a launch pair)
    "torch_train": dict(LEARNER, args=LEARNER["args"] + ["--torch-train", "--n-step", "3"]),
    # the mixed-precision env kernels, launch-shared taus (resets stay in front of the act kernel), the episode log in its summary-only form
    "mixed": dict(LEARNER, args=LEARNER["args"] + ["--precision", "mixed", "--shared-taus", "--episode-log"]),
}


def _train(cwd, case, *extra, seed=3):
    """One `python -m ...train_iqn` child in `cwd` (which holds the config; save_dir is relative, so every run records the same trial_config.json)."""
    os.makedirs(cwd, exist_ok=True)
    with open(os.path.join(cwd, "config.json"), "w") as f:
        json.dump(dict(agent="IQN", seed=seed, save_dir="runs", **case["config"]), f)
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    cmd = [sys.executable, "-m", "distributional_rl_navigation_amd.train_iqn", "-C", "config.json", "-D", DEV, "--run-name", "toy", *case["args"], *COMMON, *extra]
    r = subprocess.run(cmd, cwd=cwd, env=env, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, (cmd, r.stdout[-1500:], r.stderr[-3000:])
    return r.stdout


def _same(x, y, path):
    import torch as t
    if isinstance(x, dict):
        assert isinstance(y, dict) and x.keys() == y.keys(), path
        for k in x:
            _same(x[k], y[k], f"{path}.{k}")
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
        for k in za.files:
            _same(za[k], zb[k], f"{name}:{k}")
    elif name.endswith((".pth", ".pt")):
        _same(t.load(a, map_location="cpu", weights_only=False), t.load(b, map_location="cpu", weights_only=False), name)
    elif name.endswith(".json"):
        with open(a) as f, open(b) as g:
            _same(json.load(f), json.load(g), name)
    else:
        with open(a, "rb") as f, open(b, "rb") as g:
            assert f.read() == g.read(), name


@pytest.mark.parametrize("name", list(CASES))
def test_trainer_stopped_and_resumed_writes_the_files_of_the_straight_run(torch, tmp_path, name):
    case = CASES[name]
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    seed_a, seed_b = (os.path.join(d, "runs", "training_toy", "seed_3") for d in (a, b))
    _train(a, case, "--dump-final-state", "final.pt")                                                       # A: straight through
    out = _train(b, case, "--checkpoint-every", str(EVERY), "--stop-after", str(STOP))                       # B: a checkpoint behind step 25, stopped behind step 30
    assert f"stopped after vector step {STOP} of {case['vector_steps']}" in out
    files_b = sorted(os.listdir(seed_b))
    assert "checkpoint.pt" in files_b and "checkpoint.prev.pt" in files_b and "completed.json" not in files_b
    ck = torch.load(os.path.join(seed_b, "checkpoint.pt"), map_location="cpu", weights_only=False)
    prev = torch.load(os.path.join(seed_b, "checkpoint.prev.pt"), map_location="cpu", weights_only=False)
    assert (ck["vector_step"], prev["vector_step"], ck["format"]) == (STOP, EVERY, 1) and ck["plan"]["vector_steps"] == case["vector_steps"]
    # C: a fresh process continues B's directory -- with --checkpoint-every still on, so the run it finishes is itself a resumed run that checkpointed (behind step 50)
    out = _train(b, case, "--resume", os.path.join("runs", "training_toy"), "--checkpoint-every", str(EVERY), "--dump-final-state", "final.pt")
    assert f"continuing from vector step {STOP} (checkpoint.pt)" in out
    assert torch.load(os.path.join(seed_b, "checkpoint.pt"), map_location="cpu", weights_only=False)["vector_step"] == 50
    files_a = sorted(os.listdir(seed_a))
    assert {"completed.json", "network_params.pth", "greedy_evaluations.npz", "adaptive_evaluations.npz", "trial_config.json"} <= set(files_a)
    if "reference" in name:
        assert {"training_log.npz", "training_episodes.npz"} <= set(files_a)
    if name == "mixed":
        assert "training_log.npz" in files_a and "training_episodes.npz" not in files_a
    assert sorted(set(os.listdir(seed_b)) - {"checkpoint.pt", "checkpoint.prev.pt"}) == files_a
    for f in files_a:
        _same_file(os.path.join(seed_a, f), os.path.join(seed_b, f), f)
    _same_file(os.path.join(a, "final.pt"), os.path.join(b, "final.pt"), "final.pt")      # the state_dict()s of agent, ring and env behind the last step
    z = np.load(os.path.join(seed_a, "greedy_evaluations.npz"), allow_pickle=True)
    assert len(z["timesteps"]) >= 2 and z["rewards"].shape[1] == 3
    if name == "learner":      # ... and a complete directory is left alone
        out = _train(b, case, "--resume", os.path.join("runs", "training_toy"))
        assert "holds completed.json, nothing to do" in out


def test_trainer_resume_with_a_pool_of_workers(torch, tmp_path):
    """-P 2: the two seeds of the config stop and resume in worker processes of their own; each seed's files equal those of the sequential, uninterrupted run."""
    case = CASES["reference_after_target_copy_inside_eps_ramp"]
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    _train(a, case, seed=[3, 4])
    out = _train(b, case, "-P", "2", "--stop-after", str(STOP), seed=[3, 4])
    assert out.count(f"stopped after vector step {STOP}") == 2
    out = _train(b, case, "-P", "2", "--resume", os.path.join("runs", "training_toy"), seed=[3, 4])
    for seed in (3, 4):
        da, db = (os.path.join(d, "runs", "training_toy", f"seed_{seed}") for d in (a, b))
        files = sorted(os.listdir(da))
        assert "completed.json" in files and sorted(set(os.listdir(db)) - {"checkpoint.pt", "checkpoint.prev.pt"}) == files
        for f in files:
            _same_file(os.path.join(da, f), os.path.join(db, f), f"seed_{seed}/{f}")
