"""Measurements of the reference-budget mode (train_iqn / train_dqn --env-budget reference) and of the training-episode log on one MI355X.

    python scripts/reference_budget_bench.py [--parts learner,run,n,ladder,log,dqn] [--out profiles/reference_budget.txt]

Every GPU step is a process of its own under `timeout -k 10 <limit>`; the steps are chained: the first one that fails (a fault, an abort,
a time limit) ends the script, and what was measured up to there is in the output file.

Parts:
  learner  back-to-back one-launch gradient steps at batch 32 beside batch 256 (scripts/learner_bench.py)
  run      train_iqn --env-budget reference on seeds 0-4: wall time, final greedy / adaptive successes of 30, mean return
  n        the same run at N = 16 / 80 / 400 env steps per vector step (seed 0; 80 twice more for the run-to-run spread)
  ladder   learner budget fixed (93 750 steps of batch 256), --n-envs 32 / 256 / 1 024 / 4 096 = 3 M / 24 M / 96 M / 384 M env steps, 3 seeds
  log      the 4 096-env default with and without --episode-log, alternated, medians of 5
  dqn      one train_dqn --env-budget reference run
`--one` (internal): one trial in this process, one JSON line.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)


def one(args):
    """One trial; prints one JSON line: wall time of run_trial and the last evaluation."""
    import numpy as np
    import torch
    spec = json.loads(args.one)
    driver = spec.pop("driver", "iqn")
    params = dict(agent=driver.upper(), seed=spec.pop("seed", 0), total_timesteps=3_000_000, eval_freq=10_000, save_dir=tempfile.mkdtemp(prefix="refbudget_"),
                  training_time="bench")
    n_envs = spec.pop("n_envs", None)
    torch.cuda.set_device(0)
    torch.zeros(1, device="cuda:0")
    if driver == "iqn":
        from distributional_rl_navigation_amd.train_iqn import run_trial
        spec.setdefault("eval_deferred", dict(verbose=False))
    else:
        from distributional_rl_navigation_amd.train_dqn import run_trial
    t0 = time.perf_counter()
    d = run_trial("cuda:0", params, n_envs, verbose=False, **spec)
    wall = time.perf_counter() - t0
    out = dict(driver=driver, seed=params["seed"], n_envs=n_envs, wall_s=round(wall, 2))
    for policy, name in (("greedy", "greedy_evaluations.npz"), ("adaptive", "adaptive_evaluations.npz"), ("greedy", "evaluations.npz")):
        f = os.path.join(d, name)
        if os.path.exists(f):
            z = np.load(f, allow_pickle=True)
            out[policy] = dict(points=int(len(z["timesteps"])), last_timestep=int(z["timesteps"][-1]), successes=int(np.sum(z["successes"][-1])),
                               mean_return=round(float(np.mean(z["rewards"][-1])), 2))
    f = os.path.join(d, "training_log.npz")
    if os.path.exists(f):
        z = np.load(f)
        out["training_log"] = dict(rows=int(len(z["episodes"])), episodes=int(z["episodes"].sum()), last_row_return_mean=round(float(z["return_mean"][-1]), 2))
    print("RESULT " + json.dumps(out), flush=True)


class Chain:
    def __init__(self, out):
        self.out = out
        os.makedirs(os.path.dirname(os.path.abspath(out)) or ".", exist_ok=True)
        self.f = open(out, "w")

    def say(self, line=""):
        print(line, flush=True)
        self.f.write(line + "\n")
        self.f.flush()

    def step(self, limit, argv):
        """One GPU process under its own time limit; anything but exit status 0 ends the script."""
        import threading
        over = threading.Event()

        def heartbeat():      # (a line a minute: a long step is not a silent one)
            t0 = time.time()
            while not over.wait(60):
                print(f"  ... {time.time() - t0:.0f} s", flush=True)
        threading.Thread(target=heartbeat, daemon=True).start()
        try:
            r = subprocess.run(["timeout", "-k", "10", str(limit)] + argv, cwd=ROOT, capture_output=True, text=True)
        finally:
            over.set()
        if r.returncode != 0:
            self.say(f"STEP FAILED (exit status {r.returncode}): {' '.join(argv)}")
            self.say(r.stdout[-1500:] + r.stderr[-1500:])
            self.say("stopping here: nothing more is started on the GPU")
            sys.exit(1)
        return r.stdout

    def trial(self, limit, **spec):
        out = self.step(limit, [sys.executable, os.path.abspath(__file__), "--one", json.dumps(spec)])
        return json.loads([l for l in out.splitlines() if l.startswith("RESULT ")][-1][7:])


def fmt(r):
    s = f"wall {r['wall_s']:7.1f} s"
    for p in ("greedy", "adaptive"):
        if p in r:
            s += f"   {p} {r[p]['successes']:2d}/30, mean return {r[p]['mean_return']:6.2f} ({r[p]['points']} points, last at {r[p]['last_timestep']})"
    if "training_log" in r:
        s += f"   log: {r['training_log']['episodes']} episodes in {r['training_log']['rows']} rows"
    return s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="learner,run,n,ladder,log,dqn")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "reference_budget.txt"))
    ap.add_argument("--one", default=None)
    ap.add_argument("--seeds", default="0,1,2,3,4")
    args = ap.parse_args()
    if args.one:
        return one(args)
    parts = args.parts.split(",")
    c = Chain(args.out)
    c.say("# reference-budget mode and training-episode log, one MI355X (scripts/reference_budget_bench.py); parts: " + args.parts)
    c.say("# reference (tests/golden/ref_iqn_seed3_greedy_curve.npz, seed 3): final greedy 26/30, mean return 69.25")
    c.say("# learner-budget default (profiles/r06_learning_curve.txt, 4 096 envs, 24 runs): final greedy 26.1 +- 1.4 of 30")
    if "learner" in parts:
        c.say("\n## 1. batch-32 gradient step, back to back (scripts/learner_bench.py <reps> <batch>; first lines: mode 0 with 1 / 2 / 3 launches per step)")
        for b in (32, 256):
            out = c.step(240, [sys.executable, "scripts/learner_bench.py", "4000", str(b)])
            for l in out.splitlines()[:3]:
                c.say(f"batch {b:3d}: {l}")
    if "run" in parts:
        c.say("\n## 2. train_iqn --env-budget reference (N = 80: 37 500 vector steps x 20 batch-32 gradient steps, 300 deferred evaluation points, episode log on)")
        for s in (int(x) for x in args.seeds.split(",")):
            c.say(f"seed {s}: " + fmt(c.trial(600, seed=s, env_budget="reference")))
    if "n" in parts:
        c.say("\n## 3. env steps per vector step N (seed 0)")
        for n in (16, 80, 400, 80, 80):
            c.say(f"N = {n:3d}: " + fmt(c.trial(900, seed=0, n_envs=n, env_budget="reference")))
    if "ladder" in parts:
        c.say("\n## 4. env-step budget at a fixed learner budget (93 750 gradient steps of batch 256, one per vector step; 30 deferred evaluation points)")
        for n in (32, 256, 1024, 4096):
            for s in (0, 1, 2):
                c.say(f"--n-envs {n:4d} ({n * 93_750 / 1e6:5.0f} M env steps) seed {s}: " + fmt(c.trial(600, seed=s, n_envs=n, grad_steps=1, total_grad_steps=93_750)))
    if "log" in parts:
        c.say("\n## 5. cost of the episode log at the 4 096-env default (93 750 vector steps; alternated, 5 runs each)")
        walls = dict(off=[], on=[])
        for _ in range(5):
            for k in ("off", "on"):
                walls[k].append(c.trial(600, seed=0, n_envs=4096, episode_log=(k == "on"))["wall_s"])
        for k in ("off", "on"):
            c.say(f"episode log {k:3s}: median {statistics.median(walls[k]):6.2f} s   runs {walls[k]}")
        d = statistics.median(walls["on"]) - statistics.median(walls["off"])
        c.say(f"difference of the medians: {d:+.2f} s = {1e6 * d / 93_750:+.2f} us per vector step")
    if "dqn" in parts:
        c.say("\n## 6. train_dqn --env-budget reference (N = 80: 2 990 000 batch-32 gradient steps), seed 0")
        c.say("seed 0: " + fmt(c.trial(1100, driver="dqn", seed=0, env_budget="reference")))
    c.say("\ndone")


if __name__ == "__main__":
    main()
