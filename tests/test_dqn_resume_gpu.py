"""A DQN training run stopped at a vector step and resumed -- in a fresh process, with fresh objects, under `--together` or without -- writes the files of
the uninterrupted run: every file of the trial directory and the final states of agent, ring and env, compared byte for byte (tensor for tensor).

Toy sizes, 60 vector steps a run, three evaluation worlds of 40 steps.  Two configurations:
* learner: 256 envs, batch 32, a ring of 8 192 rows (full behind vector step 32), one gradient step behind every vector step from step 40 on (21 in all),
  inline evaluations behind steps 20 / 40 / 60;
* reference: the reference's budget at toy size -- 16 env steps a vector step, 16 batch-32 gradient steps behind each from step 11 on (800 in all), a target
  copy every 160 of them (behind vector steps 20, 30, ...), deferred evaluations, the full episode log.
A: straight; B: `checkpoint_every=25` and `stop_after`; C: B's directory resumed with `checkpoint_every=25` still on."""
import contextlib
import io
import json
import os
import shutil
import subprocess
import sys
import zipfile

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EVERY, STEPS = 25, 60
CHECKPOINTS = {"checkpoint.pt", "checkpoint.prev.pt"}
LEARNER = dict(config=dict(total_timesteps=2000, eval_freq=500), n_envs=256, grad_steps=21,
               kw=dict(batch=32, replay=8192, grad_steps=1, total_grad_steps=60, n_evals=3),
               args=["--n-envs", "256", "--batch", "32", "--replay", "8192", "--grad-steps", "1", "--total-grad-steps", "60", "--n-evals", "3"])
REFERENCE = dict(config=dict(total_timesteps=960, eval_freq=320), n_envs=16, grad_steps=800,
                 kw=dict(env_budget="reference", reference=dict(learning_starts=160, target_update_interval=160, replay=4096), episode_log="full",
                         fused_collect=True, train_steps_per_call="multi"))
TOY = dict(eval_worlds=3, max_eval_steps=40)


@pytest.fixture(scope="module")
def torch():
    import torch as t
    if not t.cuda.is_available():
        pytest.skip("no GPU")
    return t


# ---- comparing ---------------------------------------------------------------------------------------------------------------------------
def _same(x, y, path):
    import torch as t
    if isinstance(x, dict):
        assert isinstance(y, dict) and x.keys() == y.keys(), (path, sorted(map(str, x)), sorted(map(str, y)))
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


def _load(path):
    import torch as t
    return t.load(path, map_location="cpu", weights_only=False)


def _same_file(a, b, name):
    import torch as t
    if name.endswith(".npz"):
        za, zb = np.load(a, allow_pickle=True), np.load(b, allow_pickle=True)
        assert sorted(za.files) == sorted(zb.files), name
        for k in za.files:
            _same(za[k], zb[k], f"{name}:{k}")      # (the ragged `actions` of evaluations.npz as lists of arrays)
    elif name.endswith(".zip"):      # latest_model.zip / best_model.zip: the tensors of their policy.pth
        with zipfile.ZipFile(a) as za, zipfile.ZipFile(b) as zb:
            assert za.namelist() == zb.namelist() == ["policy.pth"], name
            _same(t.load(io.BytesIO(za.read("policy.pth")), map_location="cpu"), t.load(io.BytesIO(zb.read("policy.pth")), map_location="cpu"), name)
    elif name.endswith((".pth", ".pt")):
        _same(_load(a), _load(b), name)
    elif name.endswith(".json"):
        with open(a) as f, open(b) as g:
            _same(json.load(f), json.load(g), name)
    else:
        with open(a, "rb") as f, open(b, "rb") as g:
            assert f.read() == g.read(), name


def _seed_dir(where, seed=3):
    return os.path.join(str(where), "runs", "training_toy", f"seed_{seed}")


def _same_trial(where_a, where_b, seed=3, reference=False):
    """Every file of seed's directory under `where_b` equals the one under `where_a` (the straight run); the lists are equal apart from the checkpoints."""
    da, db = _seed_dir(where_a, seed), _seed_dir(where_b, seed)
    files = sorted(os.listdir(da))
    assert {"completed.json", "evaluations.npz", "latest_model.zip", "best_model.zip", "trial_config.json", "training_schedule.json"} <= set(files), files
    if reference:
        assert {"training_log.npz", "training_episodes.npz"} <= set(files), files
    assert not CHECKPOINTS & set(files)
    assert sorted(set(os.listdir(db)) - CHECKPOINTS) == files
    for f in files:
        _same_file(os.path.join(da, f), os.path.join(db, f), f"seed_{seed}/{f}")


# ---- running in this process: the cwd is the run's own directory and save_dir is relative, so every run records the same params ----------------------
@contextlib.contextmanager
def _cwd(where):
    os.makedirs(str(where), exist_ok=True)
    old = os.getcwd()
    os.chdir(str(where))
    try:
        yield
    finally:
        os.chdir(old)


def _params(case, seed):
    return dict(agent="DQN", seed=seed, save_dir="runs", training_time="toy", **case["config"])


def _run(where, case, seed=3, **opts):
    from distributional_rl_navigation_amd.train_dqn import run_trial
    with _cwd(where):
        return run_trial(DEV, _params(case, seed), case["n_envs"], return_agent=True, **dict(case["kw"], **TOY, **opts))[1]


def _run_together(where, case, seeds=(3, 4), **opts):
    from distributional_rl_navigation_amd.train_dqn import run_trials_together
    with _cwd(where):
        return run_trials_together(DEV, [_params(case, s) for s in seeds], case["n_envs"], return_agents=True, **dict(case["kw"], **TOY, **opts))[1]


def _checkpoint_steps(where, seed=3):
    d = _seed_dir(where, seed)
    return tuple(_load(os.path.join(d, f))["vector_step"] if os.path.exists(os.path.join(d, f)) else None for f in ("checkpoint.pt", "checkpoint.prev.pt"))


def _straight_stopped_resumed(tmp_path, case, stop, reference=False, **opts):
    a, b = tmp_path / "a", tmp_path / "b"
    agent = _run(a, case, dump_final_state="final.pt", **opts)                                               # A
    assert agent.n_updates == case["grad_steps"] and agent.num_timesteps == STEPS * case["n_envs"]
    stopped = _run(b, case, checkpoint_every=EVERY, stop_after=stop, **opts)                                 # B
    assert _checkpoint_steps(b) == (stop, EVERY) and "completed.json" not in os.listdir(_seed_dir(b))
    ck = _load(os.path.join(_seed_dir(b), "checkpoint.pt"))
    assert ck["format"] == 1 and ck["plan"]["vector_steps"] == STEPS and ck["agent"]["n_updates"] == stopped.n_updates == ck["run"]["grad_steps_done"]
    resumed = _run(b, case, resume=True, checkpoint_every=EVERY, dump_final_state="final.pt", **opts)        # C: fresh objects
    assert resumed is not stopped and _checkpoint_steps(b)[0] == 50
    _same_trial(a, b, reference=reference)
    _same_file(str(a / "final.pt"), str(b / "final.pt"), "final.pt")
    with open(os.path.join(_seed_dir(b), "completed.json")) as f:
        assert json.load(f) == dict(vector_steps=STEPS, grad_steps=case["grad_steps"])
    return ck, _load(str(a / "final.pt"))


# ---- 6. the learner configuration through the command line, every half in a process of its own ----------------------------------------------------
def _child(cwd, case, *extra):
    os.makedirs(cwd, exist_ok=True)
    with open(os.path.join(cwd, "config.json"), "w") as f:
        json.dump(dict(agent="DQN", seed=3, save_dir="runs", **case["config"]), f)
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    cmd = [sys.executable, "-m", "distributional_rl_navigation_amd.train_dqn", "-C", "config.json", "-D", DEV, "--run-name", "toy", *case["args"],
           "--eval-worlds", "3", "--max-eval-steps", "40", *extra]
    r = subprocess.run(cmd, cwd=cwd, env=env, capture_output=True, text=True, timeout=240)      # (one child at a time; the first that fails ends the test)
    assert r.returncode == 0, (cmd, r.stdout[-1500:], r.stderr[-3000:])
    return r.stdout


def test_learner_stopped_and_resumed_in_fresh_processes(torch, tmp_path):
    """Eager collect (torch.Generator), fused gradient step; the stop at 45 falls behind the ring's wrap (32) and behind the first gradient steps (40)."""
    case, a, b = LEARNER, str(tmp_path / "a"), str(tmp_path / "b")
    _child(a, case, "--dump-final-state", "final.pt")
    out = _child(b, case, "--checkpoint-every", str(EVERY), "--stop-after", "45")
    assert f"stopped after vector step 45 of {STEPS}" in out
    assert _checkpoint_steps(b) == (45, EVERY) and "completed.json" not in os.listdir(_seed_dir(b))
    ck = _load(os.path.join(_seed_dir(b), "checkpoint.pt"))
    assert ck["ring"]["size"] == 8192 and ck["ring"]["ptr"] == 45 * 256 % 8192 and ck["agent"]["n_updates"] == 6 and ck["agent"]["adam_step"] == 6
    assert ck["args"]["torch_train"] is False and ck["deferred"] is None and len(ck["run"]["log"]["timesteps"]) == 2
    out = _child(b, case, "--resume", os.path.join("runs", "training_toy"), "--checkpoint-every", str(EVERY), "--dump-final-state", "final.pt")
    assert "continuing from vector step 45 (checkpoint.pt)" in out
    assert _checkpoint_steps(b)[0] == 50
    _same_trial(a, b)
    # the final states, tensor for tensor.  python's generator is no tensor and no function of the run: the OS seeds it per process, and the trainer neither seeds
    # it nor draws from it -- the state carries it so that process C continues with B's, which is what is asserted of it
    final, final_b = _load(os.path.join(a, "final.pt")), _load(os.path.join(b, "final.pt"))
    assert final_b["agent"]["py_random"] == ck["agent"]["py_random"]
    for sd in (final, final_b):
        sd["agent"].pop("py_random")
    _same(final, final_b, "final.pt")
    assert final["agent"]["n_updates"] == 21 and int(final["agent"]["train_rng"][1]) > 0      # (the fused step drew its batches)
    z = np.load(os.path.join(_seed_dir(a), "evaluations.npz"), allow_pickle=True)
    assert len(z["timesteps"]) == 3 and z["rewards"].shape == (3, 3)
    out = _child(b, case, "--resume", os.path.join("runs", "training_toy"))      # a complete directory is left alone
    assert "holds completed.json, nothing to do" in out


# ---- 7. - 9. in this process, fresh objects for the resumed half ------------------------------------------------------------------------------------
def test_learner_stopped_before_the_first_gradient_step(torch, tmp_path):
    ck, final = _straight_stopped_resumed(tmp_path, LEARNER, 30)
    assert ck["agent"]["n_updates"] == 0 and ck["agent"]["adam_step"] == 0 and float(ck["agent"]["exp_avg_sq"].abs().sum()) == 0      # no fused trainer used yet
    assert int(ck["agent"]["train_rng"][1]) == 0 and ck["ring"]["size"] == 30 * 256
    assert final["agent"]["adam_step"] == 21


def test_reference_fused_collect_multi_step_stopped_behind_a_target_copy(torch, tmp_path):
    ck, final = _straight_stopped_resumed(tmp_path, REFERENCE, 30, reference=True)
    assert ck["agent"]["act_calls"] == 30 and ck["agent"]["n_updates"] == 20 * 16 == 2 * 160      # right behind the second target copy of 160 steps ...
    _same(ck["agent"]["q_net"], {k: v for k, v in ck["agent"]["q_net_target"].items()}, "target == local behind the copy")
    assert ck["deferred"]["n_taken"] == 1 and ck["deferred"]["log"]["timesteps"] == [160] and ck["episode_log"] is not None
    assert final["agent"]["act_calls"] == STEPS and final["agent"]["adam_step"] == 800


def test_learner_torch_train_stopped_and_resumed(torch, tmp_path):
    ck, final = _straight_stopped_resumed(tmp_path, LEARNER, 45, torch_train=True)
    assert ck["args"]["torch_train"] is True and ck["agent"]["adam_step"] == 6 and int(ck["agent"]["train_rng"][1]) == 0      # the ring's generator draws there
    assert final["agent"]["adam_step"] == 21


# ---- 10. --together ---------------------------------------------------------------------------------------------------------------------------------
_SHARED = {}


def _shared(tmp_path_factory):
    """Runs several cases share: each seed's straight sequential run, and a copy of a run stopped at 30 under --together / sequentially."""
    if not _SHARED:
        root = tmp_path_factory.mktemp("dqn_resume_together")
        for seed in (3, 4):
            _run(root / "straight", REFERENCE, seed=seed)
        _run_together(root / "stopped_together", REFERENCE, stop_after=30)
        for seed in (3, 4):
            _run(root / "stopped_alone", REFERENCE, seed=seed, stop_after=30)
        for where in ("stopped_together", "stopped_alone"):
            assert [_checkpoint_steps(root / where, s) for s in (3, 4)] == [(30, None)] * 2
        _SHARED["root"] = root
    return _SHARED["root"]


def _copy(root, name, tmp_path):
    shutil.copytree(str(root / name), str(tmp_path / name))
    return tmp_path / name


def _both_seeds_equal_their_straight_runs(root, where):
    for seed in (3, 4):
        _same_trial(root / "straight", where, seed=seed, reference=True)


def test_together_straight(torch, tmp_path, tmp_path_factory):
    root = _shared(tmp_path_factory)
    agents = _run_together(tmp_path / "t", REFERENCE)
    assert [a.n_updates for a in agents] == [800, 800]
    _both_seeds_equal_their_straight_runs(root, tmp_path / "t")


def test_together_stopped_and_resumed_together(torch, tmp_path, tmp_path_factory, capsys):
    root = _shared(tmp_path_factory)
    b = _copy(root, "stopped_together", tmp_path)
    _run_together(b, REFERENCE, resume=True, checkpoint_every=EVERY)
    assert "seeds [3, 4]: continuing from vector step 30" in capsys.readouterr().out
    assert [_checkpoint_steps(b, s) for s in (3, 4)] == [(50, 30)] * 2
    _both_seeds_equal_their_straight_runs(root, b)
    _run_together(b, REFERENCE, resume=True)      # complete directories are left alone
    assert capsys.readouterr().out.count("holds completed.json, nothing to do") == 2


def test_together_stopped_and_resumed_sequentially(torch, tmp_path, tmp_path_factory):
    root = _shared(tmp_path_factory)
    b = _copy(root, "stopped_together", tmp_path)
    for seed in (3, 4):
        _run(b, REFERENCE, seed=seed, resume=True)
    _both_seeds_equal_their_straight_runs(root, b)


def test_stopped_sequentially_and_resumed_together(torch, tmp_path, tmp_path_factory):
    root = _shared(tmp_path_factory)
    b = _copy(root, "stopped_alone", tmp_path)
    _run_together(b, REFERENCE, resume=True)
    _both_seeds_equal_their_straight_runs(root, b)


def test_lockstep_checkpoint_equals_the_sequential_one(torch, tmp_path_factory):
    root = _shared(tmp_path_factory)
    for seed in (3, 4):
        t, s = (_load(os.path.join(_seed_dir(root / where, seed), "checkpoint.pt")) for where in ("stopped_together", "stopped_alone"))
        assert t["vector_step"] == s["vector_step"] == 30 and t["args"].keys() == s["args"].keys()
        _same({k: v for k, v in t.items() if k != "args"}, {k: v for k, v in s.items() if k != "args"}, f"seed_{seed}/checkpoint.pt")


def test_lockstep_resume_refuses_seeds_at_different_steps_before_anything_is_written(torch, tmp_path, tmp_path_factory):
    root = _shared(tmp_path_factory)
    b = _copy(root, "stopped_together", tmp_path)
    os.remove(os.path.join(_seed_dir(b, 4), "checkpoint.pt"))      # seed 4: back at the start
    before = {s: sorted(os.listdir(_seed_dir(b, s))) for s in (3, 4)}
    with pytest.raises(ValueError, match=r"seed 3 at vector step 30, seed 4 at vector step 0 \(no checkpoint\)"):
        _run_together(b, REFERENCE, resume=True)
    assert before == {s: sorted(os.listdir(_seed_dir(b, s))) for s in (3, 4)}


def _filled(torch, seed, rows, **kw):
    from distributional_rl_navigation_amd.dqn.agent import DQNAgent
    ag = DQNAgent(device=DEV, batch_size=32, buffer_size=2048, seed=seed, fused_train=True, **kw)
    g = torch.Generator().manual_seed(rows)
    f = lambda *shape: torch.randn(*shape, generator=g).to(DEV)
    ag.memory.add_batch(f(rows, 26), torch.randint(0, 9, (rows,), generator=g).to(DEV), f(rows), f(rows, 26), (torch.rand(rows, generator=g) < 0.1).float().to(DEV))
    return ag


_BUFFERS = ("local", "target", "exp_avg", "exp_avg_sq", "step_dev", "rng_state")


def test_load_into_a_live_learner_group_keeps_every_buffer_in_place(torch):
    from distributional_rl_navigation_amd.dqn.group_train import LearnerGroup
    agents = [_filled(torch, s, 500) for s in (3, 4)]
    group = LearnerGroup(agents)
    for _ in range(3):
        group.train()
    group.sync_target()
    group.train()
    saved = [(ag.train_state_dict(), ag.memory.state_dict()) for ag in agents]
    assert saved[0][0]["adam_step"] == 4 and int(saved[0][0]["train_rng"][1]) > 0
    alone = []
    for k, (sd, ring) in enumerate(saved):      # an agent of another seed, loaded alone, takes the single step
        ag = _filled(torch, 50 + k, 700)
        ag.memory.load_state_dict(ring)
        ag.load_train_state_dict(sd)
        ag.train()
        alone.append(ag)
    group.train_many(5)      # ... while the group moves on, then gets the states back IN PLACE
    ptrs = [[getattr(ag._fused, n).data_ptr() for n in _BUFFERS] for ag in agents]
    trainers = [ag._fused for ag in agents]
    for ag, (sd, ring) in zip(agents, saved):
        ag.memory.load_state_dict(ring)
        ag.load_train_state_dict(sd)
    assert [ag._fused for ag in agents] == trainers and ptrs == [[getattr(ag._fused, n).data_ptr() for n in _BUFFERS] for ag in agents]
    group.train()
    for ag, one in zip(agents, alone):
        assert ag.n_updates == one.n_updates == 5
        for n in _BUFFERS:
            _same(getattr(ag._fused, n), getattr(one._fused, n), n)
    group.close()


# ---- 11. the act kernel's weight image ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fused_collect, eps", [(False, 0.0), (True, 0.5)])
def test_first_act_after_a_load_uses_the_loaded_weights(torch, fused_collect, eps):
    obs = torch.randn(300, 26, generator=torch.Generator().manual_seed(1)).to(DEV)
    src = _filled(torch, 3, 500, fused_collect=fused_collect)
    for _ in range(20):
        src.train()
    src.act_batch(obs, eps)
    sd = src.train_state_dict()
    dst = _filled(torch, 9, 500, fused_collect=fused_collect)
    dst.train()
    first = dst.act_batch(obs, eps)      # its weight image is packed, from its own weights
    dst.load_train_state_dict(sd)
    want, got = src.act_batch(obs, eps), dst.act_batch(obs, eps)
    _same(want, got, "actions")
    assert not torch.equal(first, got)
    if fused_collect:
        assert dst.act_calls == src.act_calls == 2 and (got != src.policy.act_batch(obs)).any()      # ... and some rows did explore
