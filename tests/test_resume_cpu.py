"""Checkpoint and resume without a GPU: the replay ring's and the agent's `state_dict()` / `load_state_dict()` continue bit for bit, `train_iqn --resume`
finds, checks and refuses what it should, and the snapshot kernel (csrc/mn_state.hip) is exported and compiles for gfx950 without scratch."""
import ctypes
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "distributional_rl_navigation_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"


def _rows(k, seed=0):
    """k synthetic transitions: (states, actions, rewards, next_states, dones)."""
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(k, 26, generator=g), torch.randint(0, 9, (k,), generator=g), torch.rand(k, generator=g) - 0.5, torch.rand(k, 26, generator=g),
            (torch.rand(k, generator=g) < 0.1).float())


def _ring(n_step=1, seed=5):
    from distributional_rl_navigation_amd.iqn.replay_buffer import ReplayBuffer
    return ReplayBuffer(64, 8, "cpu", seed, 0.99, n_step=n_step)


def _same_ring(a, b):
    assert (a.ptr, a.size, a.version) == (b.ptr, b.size, b.version)
    for name in ("states", "next_states", "actions", "rewards", "dones"):
        assert torch.equal(getattr(a, name), getattr(b, name)), name


def test_ring_round_trip_past_the_wrap_around():
    rows = _rows(150)
    a = _ring()
    for lo in range(0, 150, 10):      # 150 rows into 64 slots: the ring wraps twice
        a.add_batch(*(t[lo:lo + 10] for t in rows))
    assert a.size == 64 and a.ptr == 150 % 64
    sd = a.state_dict()
    assert sd["states"].shape[0] == 64
    b = _ring(seed=99)
    b.load_state_dict(sd)
    _same_ring(a, b)
    for _ in range(3):
        assert torch.equal(a.sample_indices(8), b.sample_indices(8))
    for x, y in zip(a.sample(), b.sample()):
        assert torch.equal(x, y)


def test_ring_state_holds_only_the_rows_in_use():
    a = _ring()
    a.add_batch(*_rows(10))
    sd = a.state_dict()
    assert sd["states"].shape == (10, 26) and sd["size"] == 10
    b = _ring(seed=1)
    b.load_state_dict(sd)
    _same_ring(a, b)
    with pytest.raises(ValueError):
        from distributional_rl_navigation_amd.iqn.replay_buffer import ReplayBuffer
        ReplayBuffer(32, 8, "cpu", 0, 0.99).load_state_dict(sd)


def test_ring_round_trip_inside_the_n_step_window():
    rows = _rows(4 * 6)
    step = lambda ring, i: ring.add_batch(*(t[4 * i:4 * i + 4] for t in rows))      # 4 parallel streams
    a = _ring(n_step=3)
    step(a, 0); step(a, 1)
    assert a.size == 0 and a._hist["count"] == 2      # the window holds two rows per stream, nothing emitted yet
    b = _ring(n_step=3, seed=77)
    b.load_state_dict(a.state_dict())
    for i in range(2, 6):
        step(a, i); step(b, i)
        _same_ring(a, b)
    assert a.size == 16
    fresh = _ring(n_step=3)      # ... and the window matters: without it the next add emits nothing
    step(fresh, 2)
    assert fresh.size == 0


def _agent(seed):
    from distributional_rl_navigation_amd.iqn.agent import IQNAgent
    ag = IQNAgent(26, 9, BATCH_SIZE=8, BUFFER_SIZE=64, device="cpu", seed=seed)
    return ag


def _flat(params):
    return torch.cat([p.detach().reshape(-1) for p in params])


def _train(ag, k):
    loss = None
    for _ in range(k):
        loss = ag.train_from_memory()
        if ag.grad_steps % 4 == 0:
            ag._sync_target()
    return loss


def _agent_bits(ag, loss):
    m, v, step = ag._adam_state()
    return dict(local=_flat(ag.qnetwork_local.parameters()), target=_flat(ag.qnetwork_target.parameters()), exp_avg=m, exp_avg_sq=v, adam_step=step,
                counters={k: getattr(ag, k) for k in ag._COUNTERS}, loss=loss)


def test_agent_round_trip_5_plus_7_equals_12():
    rows = _rows(48, seed=3)
    a = _agent(0)
    a.memory.add_batch(*rows)
    straight = _agent_bits(a, _train(a, 12))
    assert straight["adam_step"] == 12 and straight["counters"]["grad_steps"] == 12 and straight["counters"]["_last_sync_at"] == 12

    b = _agent(0)
    b.memory.add_batch(*rows)
    _train(b, 5)
    agent_sd, ring_sd = b.state_dict(), b.memory.state_dict()
    c = _agent(1234)      # another seed: other initial weights, other generators -- everything must come from the state
    assert not torch.equal(_flat(c.qnetwork_local.parameters()), _flat(b.qnetwork_local.parameters()))
    c.memory.load_state_dict(ring_sd)
    c.load_state_dict(agent_sd)
    resumed = _agent_bits(c, _train(c, 7))
    for k in ("local", "target", "exp_avg", "exp_avg_sq", "loss"):
        assert torch.equal(straight[k], resumed[k]), k
    assert straight["adam_step"] == resumed["adam_step"] and straight["counters"] == resumed["counters"]
    assert float(straight["exp_avg_sq"].abs().sum()) > 0


def test_agent_state_carries_the_evaluation_record_and_counters():
    a = _agent(0)
    a.current_timestep, a.learning_timestep = 4096, 17
    a.eval_timesteps["greedy"].append(400); a.eval_rewards["greedy"].append([1.0, 2.0])
    a.best_eval = dict(score=(2, 1.5), timestep=400, grad_steps=3, vector_step=9)
    b = _agent(7)
    b.load_state_dict(a.state_dict())
    assert (b.current_timestep, b.learning_timestep) == (4096, 17) and b.eval_timesteps == a.eval_timesteps and b.eval_rewards == a.eval_rewards
    assert b.best_eval == a.best_eval and b.best_eval is not a.best_eval
    assert b.linear_eps(10 ** 5) == a.linear_eps(10 ** 5)


# ---- train_iqn --resume ------------------------------------------------------------------------------------------------------------------
TOY = ["--env-budget", "reference", "--n-envs", "16", "--reference", "learning_starts=400", "target_update_interval=400"]


def _cli(tmp_path, *args):
    cfg = tmp_path / "config.json"
    if not cfg.exists():
        cfg.write_text(json.dumps(dict(agent="IQN", seed=[3, 4, 5], total_timesteps=4000, eval_freq=400, save_dir=str(tmp_path / "runs"))))
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    return subprocess.run([sys.executable, "-m", "distributional_rl_navigation_amd.train_iqn", "-C", str(cfg), *args], cwd=ROOT, env=env, capture_output=True,
                          text=True, timeout=300)


def _prepared_run(tmp_path, n_envs=16):
    """A run directory as a stopped run leaves it: seed 3 complete, seed 4 with a checkpoint at vector step 30, seed 5 untouched."""
    from distributional_rl_navigation_amd import train_iqn as T
    run = tmp_path / "runs" / "training_toy"
    for s in (3, 4):
        os.makedirs(run / f"seed_{s}")
    (run / "seed_3" / T.COMPLETED_FILE).write_text("{}")
    p = dict(agent="IQN", seed=4, total_timesteps=4000, eval_freq=400, save_dir=str(tmp_path / "runs"), training_time="toy")
    ne, b, r, plan = T.plan_trial(p, n_envs, env_budget="reference", reference=dict(learning_starts=400, target_update_interval=400))
    state = dict(format=T.CHECKPOINT_FORMAT, vector_step=30, params=p, plan=T.trial_shape(plan, ne, 1, b, r), args={})
    torch.save(state, run / "seed_4" / T.CHECKPOINT_FILE)
    return run, state


def test_dry_run_resume_prints_the_resume_point_of_every_seed(tmp_path):
    run, _ = _prepared_run(tmp_path)
    r = _cli(tmp_path, "--dry-run", "--resume", str(run), *TOY)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{") and '"resume"' in l]
    assert [(l["seed"], l["resume"], l["vector_step"], l["checkpoint"]) for l in lines] == [
        (3, "completed", None, None), (4, "checkpoint", 30, "checkpoint.pt"), (5, "start", None, None)]
    assert all(l["vector_steps"] == 250 for l in lines)


def test_resume_under_another_plan_is_refused_and_names_the_key(tmp_path):
    run, _ = _prepared_run(tmp_path)
    r = _cli(tmp_path, "--dry-run", "--resume", str(run), "--env-budget", "reference", "--n-envs", "8", "--reference", "learning_starts=400", "target_update_interval=400")
    assert r.returncode != 0
    assert "n_envs was 16" in r.stderr and "is 8" in r.stderr, r.stderr[-1000:]
    from distributional_rl_navigation_amd import train_iqn as T
    assert T.first_difference(dict(a=1, n_envs=2), dict(a=2, n_envs=3), T.SHAPE_KEYS_FIRST)[0] == "n_envs"
    assert T.first_difference(dict(a=1), dict(a=1)) is None


def test_resume_together_is_refused(tmp_path):
    from distributional_rl_navigation_amd.train_iqn import CHECKPOINT_REFUSALS
    run, _ = _prepared_run(tmp_path)
    for extra in (["--together"], ["--together", "--stack-envs"]):
        r = _cli(tmp_path, "--resume", str(run), *extra)
        assert r.returncode != 0 and CHECKPOINT_REFUSALS["together"] in r.stderr, r.stderr[-1000:]
    r = _cli(tmp_path, "--checkpoint-every", "10", "--shared-learner")
    assert r.returncode != 0 and CHECKPOINT_REFUSALS["shared"] in r.stderr
    assert "checkpoint yet" in CHECKPOINT_REFUSALS["together"]


def test_truncated_checkpoint_falls_back_to_the_previous_one(tmp_path):
    from distributional_rl_navigation_amd import train_iqn as T
    run, state = _prepared_run(tmp_path)
    d = run / "seed_4"
    os.replace(d / T.CHECKPOINT_FILE, d / T.CHECKPOINT_PREV_FILE)
    torch.save(dict(state, vector_step=55), d / T.CHECKPOINT_FILE)
    blob = (d / T.CHECKPOINT_FILE).read_bytes()
    (d / T.CHECKPOINT_FILE).write_bytes(blob[:len(blob) // 2])
    lines = []
    got, name = T.load_checkpoint(str(d), log=lines.append)
    assert name == T.CHECKPOINT_PREV_FILE and got["vector_step"] == 30
    assert len(lines) == 1 and "unreadable" in lines[0] and T.CHECKPOINT_PREV_FILE in lines[0]
    r = _cli(tmp_path, "--dry-run", "--resume", str(run), *TOY)      # ... and through the command line
    assert r.returncode == 0 and "continuing from checkpoint.prev.pt" in r.stdout, r.stderr[-1000:]
    assert '"checkpoint": "checkpoint.prev.pt"' in r.stdout
    os.remove(d / T.CHECKPOINT_PREV_FILE)
    with pytest.raises(ValueError):
        T.load_checkpoint(str(d), log=lines.append)
    assert T.load_checkpoint(str(run / "seed_3")) == (None, None)


def test_checkpoint_file_is_replaced_atomically_and_keeps_the_previous_one(tmp_path):
    from distributional_rl_navigation_amd import train_iqn as T
    T.write_checkpoint(str(tmp_path), dict(format=1, vector_step=1))
    assert sorted(os.listdir(tmp_path)) == [T.CHECKPOINT_FILE]
    T.write_checkpoint(str(tmp_path), dict(format=1, vector_step=2))
    assert sorted(os.listdir(tmp_path)) == sorted([T.CHECKPOINT_FILE, T.CHECKPOINT_PREV_FILE])
    assert T.load_checkpoint(str(tmp_path))[0]["vector_step"] == 2
    assert torch.load(tmp_path / T.CHECKPOINT_PREV_FILE, weights_only=False)["vector_step"] == 1


# ---- the snapshot kernel -------------------------------------------------------------------------------------------------------------------
def test_library_exports_the_snapshot_calls():
    from distributional_rl_navigation_amd import _capi
    if not os.path.exists(_capi.LIB_PATH):
        _capi.build()
    lib = ctypes.CDLL(_capi.LIB_PATH)
    bound = {s[0] for s in _capi.SIGNATURES}
    header = open(os.path.join(ROOT, "include", "marinenav_hip.h")).read()
    for name in ("mn_state_bytes", "mn_state_save", "mn_state_load"):
        assert hasattr(lib, name) and name in bound and re.search(rf"\b{name}\s*\(", header), name


def test_snapshot_kernels_compile_for_gfx950_without_scratch():
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-I../../include", "-I.", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage",
           "-c", "-o", "/dev/null", "mn_state.hip"]
    r = subprocess.run(cmd, cwd=CSRC, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    usage, cur = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            cur = usage.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+)", line)
        if m and cur is not None:
            cur[m.group(1).strip()] = int(m.group(2))
    kernels = {k: v for k, v in usage.items() if "mn_state_kernel" in k}
    assert len(kernels) == 2, list(usage)      # <SAVE = true>, <SAVE = false>
    for k, v in kernels.items():
        assert v["ScratchSize"] == 0 and v["LDS Size"] == 0 and v["VGPRs"] <= 64, (k, v)
    rule = open(os.path.join(CSRC, "Makefile")).read()
    assert "mn_state.o: mn_state.hip" in rule and rule.count("mn_state.o") >= 4      # its own rule, and both link lines
