"""Checkpoint and resume of a DQN training run, the parts that need no GPU: the learner's train state (`DQNAgent.train_state_dict` /
`load_train_state_dict`) on the eager path, the states of the deferred evaluations and of `train_dqn.TrialRun`'s own words, the refusals of the command
line, `--dry-run --resume` on hand-made run directories, and the `--dry-run` lines without the new flags.  Every comparison of tensors is by bytes."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- 1. the learner ------------------------------------------------------------------------------------------------------------------------
def _rows(n, seed):
    g = np.random.default_rng(seed)
    f = lambda *shape: torch.from_numpy(g.standard_normal(shape).astype(np.float32))
    return (f(n, 26), torch.from_numpy(g.integers(0, 9, n)), f(n), f(n, 26), torch.from_numpy((g.random(n) < 0.1).astype(np.float32)))


def _agent(seed):
    from distributional_rl_navigation_amd.dqn.agent import DQNAgent
    return DQNAgent(device="cpu", batch_size=32, buffer_size=512, seed=seed)


def _bits(t):
    return t.detach().cpu().contiguous().view(-1).numpy().tobytes()


def _learner_bits(ag):
    flat = lambda ps: torch.cat([p.detach().reshape(-1) for p in ps])
    m, v, step = ag._adam_state()
    ring = ag.memory.state_dict()
    return dict(q_net=_bits(flat(ag.q_net.parameters())), target=_bits(flat(ag.q_net_target.parameters())), exp_avg=_bits(m), exp_avg_sq=_bits(v), step=step,
                n_updates=ag.n_updates, ring_gen=_bits(ring["gen"]), ring=(ring["size"], ring["ptr"]), gen=_bits(ag.gen.get_state()))


def _go_on(ag):
    """7 eager steps, one target copy, one exploring act (the agent's own generator)."""
    for _ in range(7):
        ag.train()
    ag.sync_target()
    return _bits(ag.act_batch(_rows(16, seed=9)[0], 0.5))


@pytest.mark.parametrize("into", ["fresh", "trained"])
def test_agent_train_state_round_trip_5_plus_7(into):
    rows = _rows(300, seed=3)
    a = _agent(0)
    a.memory.add_batch(*rows)
    for _ in range(5):
        a.train()
    a.num_timesteps, a.act_calls = 4096, 17
    a.act_batch(rows[0][:8], 0.5)      # (moves the agent's generator)
    agent_sd, ring_sd = a.train_state_dict(), a.memory.state_dict()
    assert agent_sd["adam_step"] == 5 and agent_sd["n_updates"] == 5 and float(agent_sd["exp_avg_sq"].abs().sum()) > 0
    assert list(a.state_dict()) == ["q_net." + k for k in agent_sd["q_net"]] + ["q_net_target." + k for k in agent_sd["q_net_target"]]      # policy.pth keeps its keys
    buf = __import__("io").BytesIO()
    torch.save(dict(agent=agent_sd, ring=ring_sd), buf)      # ... and through a file
    buf.seek(0)
    saved = torch.load(buf, map_location="cpu", weights_only=False)

    b = _agent(1234)      # another seed: other initial weights, other generators -- everything must come from the state
    assert _bits(next(b.q_net.parameters())) != _bits(next(a.q_net.parameters()))
    if into == "trained":      # a dirty Adam state and moved counters
        b.memory.add_batch(*_rows(100, seed=5))
        for _ in range(3):
            b.train()
        b.act_batch(rows[0][:8], 0.5)
    torch.manual_seed(99)
    b.memory.load_state_dict(saved["ring"])
    b.load_train_state_dict(saved["agent"])
    assert (b.num_timesteps, b.act_calls, b.act_seed, b.n_updates) == (4096, 17, a.act_seed, 5)
    assert _bits(torch.get_rng_state()) == _bits(agent_sd["torch_cpu_rng"])
    assert _learner_bits(a) == _learner_bits(b)
    acts_a, acts_b = _go_on(a), _go_on(b)
    bits_a, bits_b = _learner_bits(a), _learner_bits(b)
    assert acts_a == acts_b
    for k in bits_a:
        assert bits_a[k] == bits_b[k], k
    assert bits_a["step"] == 12 and bits_a["n_updates"] == 12 and bits_a["q_net"] == bits_a["target"]


def test_train_state_before_the_first_step_is_an_empty_adam_state():
    a = _agent(0)
    sd = a.train_state_dict()
    assert sd["adam_step"] == 0 and float(sd["exp_avg"].abs().sum()) == 0 and sd["train_rng"].tolist() == [0, 0]
    b = _agent(7)
    b.load_train_state_dict(sd)
    rows = _rows(64, seed=1)
    for ag in (a, b):
        ag.memory.add_batch(*rows)
    b.memory.load_state_dict(a.memory.state_dict())
    a.train(); b.train()
    assert _learner_bits(a) == _learner_bits(b)


# ---- 2. the deferred evaluations and TrialRun's words -------------------------------------------------------------------------------------
def _through_a_file(sd, tmp_path):
    torch.save(sd, tmp_path / "sd.pt")
    return torch.load(tmp_path / "sd.pt", map_location="cpu", weights_only=False)


def _same_log(x, y):
    assert x.keys() == y.keys()
    for k in x:
        assert len(x[k]) == len(y[k]), k
        for a, b in zip(x[k], y[k]):
            if isinstance(a, list):
                assert len(a) == len(b) and all(np.asarray(p).tobytes() == np.asarray(q).tobytes() for p, q in zip(a, b)), k
            else:
                assert np.asarray(a).dtype == np.asarray(b).dtype and np.asarray(a).tobytes() == np.asarray(b).tobytes(), k


def _a_log():
    return dict(timesteps=[500, 1000], rewards=[np.array([1.0, -2.5, 3.0]), np.array([0.5, 0.25, -1.0])], times=[np.array([2.0, 4.0, 6.0])] * 2,
                energies=[np.array([0.1, 0.2, 0.3])] * 2, successes=[np.array([True, False, True])] * 2,
                actions=[[np.array([1, 2], dtype=np.int8), np.array([3], dtype=np.int8), np.array([], dtype=np.int8)]] * 2)


def test_deferred_evaluations_state_round_trip_without_a_device(tmp_path):
    from distributional_rl_navigation_amd.dqn.deferred_eval import DeferredEvaluations
    worlds = {"0": dict(robot=dict(a=[0.0], w=[0.0], dt=0.05, N=10))}
    d = DeferredEvaluations(_agent(0), worlds, str(tmp_path), verbose=False)
    d.log, d.best, d.launches, d.steps_run = _a_log(), 0.5, 2, [40, 33]
    sd = _through_a_file(d.state_dict(), tmp_path)      # (flushes first: nothing is pending, nothing is launched)
    assert sd["n_taken"] == 2 and sd["best"] == 0.5
    e = DeferredEvaluations(_agent(1), worlds, str(tmp_path), verbose=False)
    e.load_state_dict(sd)
    _same_log(d.log, e.log)
    assert (e.best, e.launches, e.steps_run, e.pending) == (0.5, 2, [40, 33], [])
    assert e.log is not sd["log"]
    with pytest.raises(ValueError):
        e.load_state_dict(dict(sd, n_taken=3))
    assert DeferredEvaluations(_agent(1), worlds, str(tmp_path)).state_dict()["best"] == -np.inf


def test_trial_run_words_round_trip_without_a_device(tmp_path):
    from distributional_rl_navigation_amd.train_dqn import TrialRun
    obs = torch.from_numpy(np.random.default_rng(0).standard_normal((16, 26)).astype(np.float32))
    a = TrialRun.__new__(TrialRun)
    a.obs, a.grad_steps_done, a.n_points, a.log, a.best = obs, 320, 2, _a_log(), -7.25
    sd = _through_a_file(a.own_state(), tmp_path)
    assert sorted(sd) == ["best", "grad_steps_done", "log", "n_points", "obs"]
    b = TrialRun.__new__(TrialRun)
    b.obs = torch.zeros(16, 26)
    b.load_own_state(sd)
    assert _bits(b.obs) == _bits(obs) and (b.grad_steps_done, b.n_points, b.best) == (320, 2, -7.25)
    _same_log(a.log, b.log)


# ---- 3. - 5. the command line --------------------------------------------------------------------------------------------------------------
LEARNER = ["--n-envs", "256", "--batch", "32", "--replay", "8192", "--grad-steps", "1", "--total-grad-steps", "60", "--n-evals", "3"]
CONFIG = dict(agent="DQN", total_timesteps=2000, eval_freq=500)


def _cli(tmp_path, *args, seed=(3, 4, 5), config=CONFIG):
    cfg = tmp_path / "config.json"
    cfg.write_text(json.dumps(dict(config, seed=list(seed), save_dir=str(tmp_path / "runs"))))
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""), CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="")
    return subprocess.run([sys.executable, "-m", "distributional_rl_navigation_amd.train_dqn", "-C", str(cfg), *args], cwd=ROOT, env=env, capture_output=True,
                          text=True, timeout=300)


def test_refusals_write_nothing(tmp_path):
    from distributional_rl_navigation_amd import train_dqn as T
    assert "--together without --stack-envs" in T.CHECKPOINT_REFUSALS["stack_envs"] and "one" in T.CHECKPOINT_REFUSALS["stack_envs"]
    assert T.TOGETHER_REFUSALS["stack_envs"] == "--stack-envs stacks the envs of seeds that train together in one handle; it needs --together"
    r = _cli(tmp_path, "--stack-envs", "--together", "--stop-after", "5")
    assert r.returncode != 0 and T.CHECKPOINT_REFUSALS["stack_envs"] in r.stderr, r.stderr[-1000:]
    r = _cli(tmp_path, "--checkpoint-every", "0")
    assert r.returncode != 0 and "at least 1" in r.stderr, r.stderr[-1000:]
    r = _cli(tmp_path, "--stop-after", "-3")
    assert r.returncode != 0 and "at least 1" in r.stderr, r.stderr[-1000:]
    os.makedirs(tmp_path / "elsewhere")
    for path in (tmp_path / "nowhere", tmp_path / "elsewhere"):      # no directory; a directory that is no training_<time>
        r = _cli(tmp_path, "--resume", str(path))
        assert r.returncode != 0 and "takes a run directory" in r.stderr, r.stderr[-1000:]
    os.makedirs(tmp_path / "other" / "training_toy")
    r = _cli(tmp_path, "--resume", str(tmp_path / "other" / "training_toy"))
    assert r.returncode != 0 and "does not lead to that directory" in r.stderr, r.stderr[-1000:]
    two = [dict(CONFIG, seed=s, training_time="t", save_dir=str(tmp_path / "runs")) for s in (0, 1)]
    for kw in (dict(stop_after=5), dict(checkpoint_every=5), dict(resume=True)):
        with pytest.raises(ValueError) as e:
            T.run_trials_together("cuda:0", two, 16, stack_envs=True, **kw)      # (before it needs a device)
        assert str(e.value) == T.CHECKPOINT_REFUSALS["stack_envs"]
    with pytest.raises(ValueError, match="at least 1"):
        T.run_trial("cuda:0", two[0], 16, checkpoint_every=0)
    assert not os.path.exists(tmp_path / "runs")      # refused before a trial directory was made


def _state(T, tmp_path, seed, vector_step, n_envs=256):
    p = dict(CONFIG, seed=seed, save_dir=str(tmp_path / "runs"), training_time="toy")
    ne, b, r, plan = T.plan_trial(p, n_envs, batch=32, replay=8192, grad_steps=1, total_grad_steps=60, n_evals=3)
    return dict(format=T.CHECKPOINT_FORMAT, vector_step=vector_step, params=p, plan=T.trial_shape(plan, ne, 1, b, r), args=T.run_shaping_args())


def _resume_lines(r):
    return [(l["seed"], l["resume"], l["vector_step"], l["checkpoint"]) for l in (json.loads(x) for x in r.stdout.splitlines() if x.startswith("{") and '"resume"' in x)]


def test_dry_run_resume_on_a_hand_made_run_directory(tmp_path):
    from distributional_rl_navigation_amd import train_dqn as T
    run = tmp_path / "runs" / "training_toy"
    for s in (3, 4, 5):
        os.makedirs(run / f"seed_{s}")
    (run / "seed_3" / T.COMPLETED_FILE).write_text(json.dumps(dict(vector_steps=60, grad_steps=21)))
    torch.save(_state(T, tmp_path, 5, 45), run / "seed_5" / T.CHECKPOINT_FILE)
    r = _cli(tmp_path, "--dry-run", "--resume", str(run), *LEARNER)
    assert r.returncode == 0, r.stderr[-2000:]
    assert _resume_lines(r) == [(3, "completed", None, None), (4, "start", None, None), (5, "checkpoint", 45, "checkpoint.pt")]
    plans = [json.loads(x) for x in r.stdout.splitlines() if x.startswith("{") and '"plan"' in x]
    assert len(plans) == 3 and all(p["plan"]["vector_steps"] == 60 and p["plan"]["learning_starts_vector_steps"] == 40 for p in plans)
    assert all(list(json.loads(x)) == ["seed", "resume", "vector_step", "checkpoint"] for x in r.stdout.splitlines() if '"resume"' in x)

    # a checkpoint of another n_envs: refused, naming the key and both values; other run-shaping arguments likewise
    r = _cli(tmp_path, "--dry-run", "--resume", str(run), *["128" if a == "256" else a for a in LEARNER])
    assert r.returncode != 0 and "n_envs was 256" in r.stderr and "is 128" in r.stderr, r.stderr[-1000:]
    state = _state(T, tmp_path, 5, 45)
    with pytest.raises(ValueError, match="fused_collect was False there and is True"):
        T.resume_point(str(run / "seed_5"), state["plan"], T.run_shaping_args(fused_collect=True))
    saved = dict(T.run_shaping_args(), torch_train=False, train_steps_per_call="auto")      # recorded by the run, not compared: not among the run-shaping arguments
    torch.save(dict(state, args=saved), run / "seed_5" / T.CHECKPOINT_FILE)
    assert T.resume_point(str(run / "seed_5"), state["plan"], T.run_shaping_args(torch_train=True, train_steps_per_call="multi"))[0] == "checkpoint"
    assert sorted(T.run_shaping_args()) == ["env_budget", "episode_log", "eval_deferred", "eval_one_launch", "eval_worlds", "fused_collect", "max_eval_steps", "reference"]

    # an unreadable checkpoint.pt beside a good checkpoint.prev.pt
    d = run / "seed_5"
    os.replace(d / T.CHECKPOINT_FILE, d / T.CHECKPOINT_PREV_FILE)
    torch.save(_state(T, tmp_path, 5, 50), d / T.CHECKPOINT_FILE)
    blob = (d / T.CHECKPOINT_FILE).read_bytes()
    (d / T.CHECKPOINT_FILE).write_bytes(blob[:len(blob) // 2])
    r = _cli(tmp_path, "--dry-run", "--resume", str(run), *LEARNER)
    assert r.returncode == 0 and _resume_lines(r)[2] == (5, "checkpoint", 45, "checkpoint.prev.pt"), r.stderr[-1000:]
    said = [x for x in r.stdout.splitlines() if "continuing from checkpoint.prev.pt" in x]
    assert len(said) == 1 and said[0].startswith("[train_dqn]") and "unreadable" in said[0]


def test_dry_run_resume_together_refuses_seeds_at_different_steps(tmp_path):
    from distributional_rl_navigation_amd import train_dqn as T
    run = tmp_path / "runs" / "training_toy"
    for s, k in ((3, 30), (4, 45)):
        os.makedirs(run / f"seed_{s}")
        torch.save(_state(T, tmp_path, s, k), run / f"seed_{s}" / T.CHECKPOINT_FILE)
    r = _cli(tmp_path, "--dry-run", "--resume", str(run), "--together", *LEARNER, seed=(3, 4))
    assert r.returncode != 0 and "seed 3 at vector step 30" in r.stderr and "seed 4 at vector step 45" in r.stderr and "without --together" in r.stderr, r.stderr[-1000:]
    r = _cli(tmp_path, "--dry-run", "--resume", str(run), *LEARNER, seed=(3, 4))      # ... the sequential resume takes them
    assert r.returncode == 0 and _resume_lines(r) == [(3, "checkpoint", 30, "checkpoint.pt"), (4, "checkpoint", 45, "checkpoint.pt")]
    torch.save(_state(T, tmp_path, 3, 45), run / "seed_3" / T.CHECKPOINT_FILE)      # the same step: fine; a completed seed leaves the group
    os.makedirs(run / "seed_5")
    (run / "seed_5" / T.COMPLETED_FILE).write_text("{}")
    r = _cli(tmp_path, "--dry-run", "--resume", str(run), "--together", *LEARNER, seed=(3, 4, 5))
    assert r.returncode == 0 and [x[1:3] for x in _resume_lines(r)] == [("checkpoint", 45), ("checkpoint", 45), ("completed", None)], r.stderr[-1000:]
    with pytest.raises(ValueError, match=r"seed 1 at vector step 0 \(no checkpoint\)"):
        T.check_lockstep([(0, "checkpoint", dict(vector_step=7)), (1, "start", None)])
    assert T.check_lockstep([]) == 0 and T.check_lockstep([(0, "checkpoint", dict(vector_step=7))]) == 7


def test_dry_run_lines_are_unchanged_without_the_new_flags(tmp_path):
    lines = lambda r: [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
    plain = ["seed", "n_envs", "batch", "replay", "fused", "eval_one_launch", "eval_deferred", "eps_start", "eps_end", "plan"]
    r = _cli(tmp_path, "--dry-run")
    assert r.returncode == 0 and [list(t) for t in lines(r)] == [plain] * 3, r.stderr[-1000:]
    r = _cli(tmp_path, "--dry-run", "--env-budget", "reference", config=dict(agent="DQN", total_timesteps=3_000_000, eval_freq=10_000))      # (the shipped run)
    assert lines(r)[0]["plan"]["total_grad_steps"] == 2_990_000 and lines(r)[0]["n_envs"] == 80
    assert r.returncode == 0 and [list(t) for t in lines(r)] == [plain[:7] + ["env_budget", "episode_log"] + plain[7:]] * 3, r.stderr[-1000:]
    assert "resume" not in r.stdout and "checkpoint" not in r.stdout
    r = _cli(tmp_path, "--dry-run", "--together")
    assert r.returncode == 0 and lines(r)[-1] == dict(together=[dict(group=0, seeds=[3, 4, 5], one_launch_per_gradient_step=True)])
    # the toy reference plan of the GPU tests: 60 vector steps, 16 gradient steps behind each from vector step 11 on, a target copy every 10 vector steps
    r = _cli(tmp_path, "--dry-run", "--env-budget", "reference", "--n-envs", "16", "--reference", "learning_starts=160", "target_update_interval=160", "replay=4096",
             config=dict(agent="DQN", total_timesteps=960, eval_freq=320))
    plan = lines(r)[0]["plan"]
    assert r.returncode == 0 and lines(r)[0]["replay"] == 4096, r.stderr[-1000:]
    assert (plan["vector_steps"], plan["grad_steps_per_vector_step"], plan["learning_starts_vector_steps"], plan["target_sync_grad_steps"]) == (60, 16, 11, 160)
