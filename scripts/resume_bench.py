"""What checkpoint and resume cost (train_iqn --checkpoint-every / --stop-after / --resume; csrc/mn_state.hip), on one GPU.  Measured and written down, not
asserted.

checkpoint  One checkpoint at three sizes -- the reference budget with its ring full (80 envs, 1 M rows), the shipped default (4 096 envs, ring 100 000) and
            65 536 envs (ring 100 000) -- in its parts: the snapshot launch of the env handle (HIP events), the env's, the ring's and the agent's
            `state_dict()` (device-to-host copies included), and `torch.save` + fsync + rename of the lot.  Medians of `--reps` with their ranges.
interval    The wall time of a train_iqn run between two checkpoints: the same run with and without `--checkpoint-every K`, K chosen from the measured
            vector-step rate so that a checkpoint falls about every `--seconds` (30) seconds; alternating, `--reps` each.
bench       `python bench.py` (plain and `--eps 0.05`) in this tree against `--parent DIR` (a checkout of the parent commit, built), alternating,
            `--reps` runs each: the options are off there, so the two must agree within the run-to-run spread the README records for that line.

    python scripts/resume_bench.py [--parts checkpoint,interval,bench] [--parent DIR] [--reps 3] [--out profiles/resume_bench.txt]
    python scripts/resume_bench.py --agent dqn --out profiles/dqn_resume_bench.txt      # the `checkpoint` part for a train_dqn checkpoint
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LINES = []
SIZES = (("reference budget, ring full", 80, 1_000_000, 32), ("shipped default", 4096, 100_000, 256), ("65 536 envs", 65536, 100_000, 256))


def say(s=""):
    print(s, flush=True)
    LINES.append(s)


def med(ts):
    ts = sorted(ts)
    return ts[len(ts) // 2], ts[0], ts[-1]


def fmt(ts, unit="ms"):
    m, lo, hi = med(ts)
    return f"{m:9.2f} {unit} [{lo:.2f} .. {hi:.2f}]"


def part_checkpoint(reps, device):
    import torch
    from distributional_rl_navigation_amd.iqn.agent import IQNAgent
    from distributional_rl_navigation_amd.marinenav_env.vec_env import VecMarineNavEnv
    from distributional_rl_navigation_amd.train_iqn import TRAINING_SCHEDULE, write_checkpoint
    say("== one checkpoint, in its parts (medians [min .. max])")
    for name, n, ring, batch in SIZES:
        env = VecMarineNavEnv(n, seed=3, schedule=TRAINING_SCHEDULE, device=device, precision="f64")
        agent = IQNAgent(26, 9, BATCH_SIZE=batch, BUFFER_SIZE=ring, device=device, seed=103, learning_starts=0, UPDATE_EVERY=1)
        agent.learn_vec(total_vector_steps=max(16, 2 * batch // n + 2), train_env=env, verbose=False)      # (a few real steps: trainer, act stream, ring rows)
        agent.memory.size = agent.memory.capacity      # the ring counted as full: every row is copied
        blob = torch.empty(env.state_bytes(), dtype=torch.uint8, device=device)
        t = dict(launch=[], env=[], ring=[], agent=[], write=[])
        nbytes = 0
        with tempfile.TemporaryDirectory() as tmp:
            for r in range(reps + 1):
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(); env.save_state(blob); e1.record(); torch.cuda.synchronize()
                t0 = time.perf_counter(); sd_env = env.state_dict(); t1 = time.perf_counter()
                sd_ring = agent.memory.state_dict(); t2 = time.perf_counter()
                sd_agent = agent.state_dict(); t3 = time.perf_counter()
                path = write_checkpoint(tmp, dict(format=1, vector_step=r, env=sd_env, ring=sd_ring, agent=sd_agent)); t4 = time.perf_counter()
                nbytes = os.path.getsize(path)
                if r:      # (the first pass warms the allocators up)
                    for k, v in (("launch", e0.elapsed_time(e1)), ("env", 1e3 * (t1 - t0)), ("ring", 1e3 * (t2 - t1)), ("agent", 1e3 * (t3 - t2)), ("write", 1e3 * (t4 - t3))):
                        t[k].append(v)
        say(f"-- {name}: {n} envs, ring {ring} rows; blob {env.state_bytes() / 1e6:.2f} MB, checkpoint.pt {nbytes / 1e6:.1f} MB")
        say(f"   snapshot launch (device)         {fmt(t['launch'])}")
        say(f"   env.state_dict()                 {fmt(t['env'])}")
        say(f"   ring.state_dict()                {fmt(t['ring'])}")
        say(f"   agent.state_dict()               {fmt(t['agent'])}")
        say(f"   torch.save + fsync + rename      {fmt(t['write'])}")
        say(f"   sum                              {med([sum(x) for x in zip(t['env'], t['ring'], t['agent'], t['write'])])[0]:9.2f} ms")
        env.close()
        del agent, env, blob
        torch.cuda.empty_cache()


DQN_SIZES = (("reference DQN shape, ring full", 80, 1_000_000, 32), ("learner default", 4096, 100_000, 256))


def part_checkpoint_dqn(reps, device):
    """`--agent dqn`: one train_dqn checkpoint in its parts -- the env's, the ring's and the learner's state (`DQNAgent.train_state_dict`: both networks, the
    one Adam state, the draw counters, the generators) and the file -- at the reference DQN shape with its 1 M-row ring full, and at the learner default."""
    import torch
    from distributional_rl_navigation_amd.dqn.agent import DQNAgent
    from distributional_rl_navigation_amd.marinenav_env.vec_env import VecMarineNavEnv
    from distributional_rl_navigation_amd.train_iqn import TRAINING_SCHEDULE, write_checkpoint
    say("== one train_dqn checkpoint, in its parts (medians [min .. max])")
    for name, n, ring, batch in DQN_SIZES:
        env = VecMarineNavEnv(n, seed=3, schedule=TRAINING_SCHEDULE, device=device, precision="f64")
        agent = DQNAgent(26, 9, buffer_size=ring, batch_size=batch, learning_starts=0, train_freq=1, device=device, seed=103, fused_train=True)
        agent.learn_vec(total_vector_steps=max(16, 2 * batch // n + 2), train_env=env)      # (a few real steps: trainer, ring rows, Adam history)
        agent.memory.size = agent.memory.capacity      # the ring counted as full: every row is copied
        blob = torch.empty(env.state_bytes(), dtype=torch.uint8, device=device)
        t = dict(launch=[], env=[], ring=[], agent=[], write=[])
        nbytes = 0
        with tempfile.TemporaryDirectory() as tmp:
            for r in range(reps + 1):
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(); env.save_state(blob); e1.record(); torch.cuda.synchronize()
                t0 = time.perf_counter(); sd_env = env.state_dict(); t1 = time.perf_counter()
                sd_ring = agent.memory.state_dict(); t2 = time.perf_counter()
                sd_agent = agent.train_state_dict(); t3 = time.perf_counter()
                path = write_checkpoint(tmp, dict(format=1, vector_step=r, env=sd_env, ring=sd_ring, agent=sd_agent)); t4 = time.perf_counter()
                nbytes = os.path.getsize(path)
                if r:      # (the first pass warms the allocators up)
                    for k, v in (("launch", e0.elapsed_time(e1)), ("env", 1e3 * (t1 - t0)), ("ring", 1e3 * (t2 - t1)), ("agent", 1e3 * (t3 - t2)), ("write", 1e3 * (t4 - t3))):
                        t[k].append(v)
        say(f"-- {name}: {n} envs, ring {ring} rows, batch {batch}; blob {env.state_bytes() / 1e6:.2f} MB, checkpoint.pt {nbytes / 1e6:.1f} MB")
        say(f"   snapshot launch (device)         {fmt(t['launch'])}")
        say(f"   env.state_dict()                 {fmt(t['env'])}")
        say(f"   ring.state_dict()                {fmt(t['ring'])}")
        say(f"   agent.train_state_dict()         {fmt(t['agent'])}")
        say(f"   torch.save + fsync + rename      {fmt(t['write'])}")
        sums = [sum(x) for x in zip(t['env'], t['ring'], t['agent'], t['write'])]
        say(f"   sum                              {fmt(sums)}")
        env.close()
        del agent, env, blob
        torch.cuda.empty_cache()
    say("   (the run between two checkpoints, `interval`, and the lockstep loop's per-seed checkpoints: not measured)")


def _train(cwd, args, timeout=3000):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    t0 = time.perf_counter()
    r = subprocess.run([sys.executable, "-m", "distributional_rl_navigation_amd.train_iqn", "-C", "config.json", *args], cwd=cwd, env=env, capture_output=True,
                       text=True, timeout=timeout)
    if r.returncode != 0:
        raise RuntimeError(r.stderr[-2000:])
    return time.perf_counter() - t0


def part_interval(reps, seconds, total_timesteps):
    say(f"== the run between two checkpoints: with and without --checkpoint-every K (K ~ one checkpoint per {seconds:.0f} s), alternating, {reps} runs each")
    for name, extra in (("reference budget", ["--env-budget", "reference"]), ("shipped default", []), ("65 536 envs", ["--n-envs", "65536"])):
        with tempfile.TemporaryDirectory() as tmp:
            with open(os.path.join(tmp, "config.json"), "w") as f:
                json.dump(dict(agent="IQN", seed=3, total_timesteps=total_timesteps, eval_freq=10_000, save_dir="runs"), f)
            plan = json.loads(subprocess.run([sys.executable, "-m", "distributional_rl_navigation_amd.train_iqn", "-C", "config.json", "--dry-run", *extra], cwd=tmp,
                                             env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True, timeout=300).stdout.splitlines()[0])["plan"]
            warm = _train(tmp, ["--run-name", "warm", *extra])
            K = max(1, int(plan["vector_steps"] * seconds / warm))
            off, on = [], []
            for r in range(reps):
                off.append(_train(tmp, ["--run-name", f"off{r}", *extra]))
                on.append(_train(tmp, ["--run-name", f"on{r}", "--checkpoint-every", str(K), *extra]))
            n_ck = plan["vector_steps"] // K
            say(f"-- {name}: {plan['vector_steps']} vector steps, K = {K} ({n_ck} checkpoints per run)")
            say(f"   without {fmt(off, 's')}    with {fmt(on, 's')}    per checkpoint {1e3 * (med(on)[0] - med(off)[0]) / max(1, n_ck):.1f} ms")


def part_bench(reps, parent, steps, warmup):
    say(f"== bench.py in this tree against the parent commit ({parent}), alternating, {reps} runs each: the options are off there")
    for name, extra in (("plain", []), ("--eps 0.05", ["--eps", "0.05"])):
        res = dict(this=[], parent=[])
        for r in range(reps):
            for who, cwd in (("parent", parent), ("this", ROOT)):
                out = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup), *extra], cwd=cwd, capture_output=True,
                                     text=True, timeout=3000).stdout
                line = [l for l in out.splitlines() if l.startswith("{")][-1]
                res[who].append(json.loads(line))
        key = next(k for k in ("env_steps_per_s", "value", "steps_per_s") if k in res["this"][0])
        say(f"-- {name}: {key}  this tree {fmt([x[key] for x in res['this']], '')}   parent {fmt([x[key] for x in res['parent']], '')}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="checkpoint")
    ap.add_argument("--agent", default="iqn", choices=["iqn", "dqn"],
                    help="dqn: the `checkpoint` part for a train_dqn checkpoint (the reference DQN shape with its ring full, the learner default); write it with "
                         "--out profiles/dqn_resume_bench.txt")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--seconds", type=float, default=30.0)
    ap.add_argument("--total-timesteps", type=int, default=3_000_000)
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit (part `bench`)")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "resume_bench.txt"))
    args = ap.parse_args()
    parts = args.parts.split(",")
    say("# scripts/resume_bench.py " + " ".join(sys.argv[1:]))
    if args.agent == "dqn" and parts != ["checkpoint"]:
        raise SystemExit("resume_bench: --agent dqn measures the `checkpoint` part only")
    if "checkpoint" in parts:
        (part_checkpoint_dqn if args.agent == "dqn" else part_checkpoint)(args.reps, args.device)
    if "interval" in parts:
        part_interval(args.reps, args.seconds, args.total_timesteps)
    if "bench" in parts:
        if not args.parent:
            raise SystemExit("resume_bench: part `bench` needs --parent DIR (a built checkout of the parent commit)")
        part_bench(args.reps, args.parent, args.steps, args.warmup)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
