"""Does the reference's per-sample max matter on this task?  `train_iqn` for a set of seeds at the trainer's defaults (learner budget: 4 096 envs, batch 256, ring
100 000; 3 000 000 timesteps, 30 evaluation points) under one target rule per invocation:

    python scripts/target_rule_learning.py --rule max|mean|double [--seeds 8] [--out profiles/target_rule_learning.txt]

Per run: the final evaluation (greedy, the 30 evaluation worlds: successes /30 and mean return), the run's best evaluation and the wall time; per rule: mean
+- sd (ddof = 1) over the seeds -- what profiles/munchausen_learning.txt records, whose `uniform` section holds the figures of "max".  The section of the rule is
appended to the report.  Nothing is claimed in advance; the default stays "max" whatever the outcome.  Without a GPU the script fails."""
import argparse
import contextlib
import io
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rule", required=True, choices=("max", "mean", "double"))
    ap.add_argument("--seeds", type=int, default=8)
    ap.add_argument("--first-seed", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "target_rule_learning.txt"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("target_rule_learning: no GPU visible -- training runs on the device only")
    from distributional_rl_navigation_amd.train_iqn import run_trial
    form = dict(target_rule=args.rule) if args.rule != "max" else {}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    out = open(args.out, "a")

    def say(line):
        print(line, flush=True)
        out.write(line + "\n")
        out.flush()

    seeds = range(args.first_seed, args.first_seed + args.seeds)
    say(f"# scripts/target_rule_learning.py --rule {args.rule} --seeds {args.seeds}: train_iqn at its defaults ({form}), seeds {seeds[0]}..{seeds[-1]}, "
        f"{torch.cuda.get_device_name(0)}")
    finals, bests, walls = [], [], []
    for seed in seeds:
        with tempfile.TemporaryDirectory() as tmp:
            params = dict(seed=seed, total_timesteps=3_000_000, eval_freq=10_000, save_dir=tmp, training_time="run")
            t0 = time.time()
            with contextlib.redirect_stdout(io.StringIO()):
                d = run_trial("cuda:0", params, None, verbose=False, **form)
            torch.cuda.synchronize()
            walls.append(time.time() - t0)
            ev = np.load(os.path.join(d, "greedy_evaluations.npz"), allow_pickle=True)
            succ = np.asarray(ev["successes"]).astype(np.int64).sum(axis=1)
            ret = np.asarray(ev["rewards"], dtype=np.float64).mean(axis=1)
            best = json.load(open(os.path.join(d, "best_evaluation.json")))
            finals.append((int(succ[-1]), float(ret[-1])))
            bests.append((best["successes"], best["mean_return"]))
            say(f"  seed {seed}: {walls[-1]:6.1f} s; final evaluation {succ[-1]:2d}/30 {ret[-1]:7.2f}; best of {len(succ)} evaluations {best['successes']}/30 {best['mean_return']:7.2f}")
    f, b, w = np.array(finals, dtype=np.float64), np.array(bests, dtype=np.float64), np.array(walls)
    sd = lambda x: x.std(ddof=1) if len(x) > 1 else float("nan")
    say(f"  target rule {args.rule}: final evaluation over {len(f)} runs: successes {f[:, 0].mean():.2f} +- {sd(f[:, 0]):.2f} /30, mean return {f[:, 1].mean():.2f} +- "
        f"{sd(f[:, 1]):.2f}; best evaluation: successes {b[:, 0].mean():.2f} +- {sd(b[:, 0]):.2f} /30, mean return {b[:, 1].mean():.2f} +- {sd(b[:, 1]):.2f}; "
        f"wall time per run {w.mean():.1f} +- {sd(w):.1f} s")


if __name__ == "__main__":
    main()
