"""Times IQNAgent.evaluation_vec on one GPU: the per-step loop against one mn_rollout_iqn launch (one_launch=True), on the 30 evaluation worlds
(tests/golden/eval_config_seed3.json) with the shipped checkpoint (greedy, adaptive) and with a seeded untrained network (episodes run to the
1 000-step limit).  Both forms are checked to return the same evaluation.  --train: one default train_iqn seed at --n-evals 300 with and
without --eval-one-launch (wall time of the whole run).

    python scripts/eval_rollout_bench.py [--reps 5] [--train]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
G = os.path.join(ROOT, "tests", "golden")


def _time_eval(agent, env, cfg, greedy, one, reps):
    import torch
    ts, res = [], None
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = agent.evaluation_vec(env, cfg, greedy=greedy, one_launch=one)
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
        res = r if res is None else res
    return (sorted(ts)[len(ts) // 2], min(ts), max(ts)), r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--train", action="store_true")
    args = ap.parse_args()
    import contextlib
    import io
    import torch
    from distributional_rl_navigation_amd.iqn.agent import IQNAgent
    from distributional_rl_navigation_amd.marinenav_env.vec_env import VecMarineNavEnv
    with open(os.path.join(G, "eval_config_seed3.json")) as f:
        cfg = json.load(f)
    print(f"device: {torch.cuda.get_device_name(0)}; 30 evaluation worlds, f64 env; {args.reps} evaluations each: median [min .. max]")
    print(f"{'network':<22}{'policy':<10}{'steps':>6}{'loop ms':>28}{'one launch ms':>28}{'speed-up':>10}{'us/step (one)':>15}  same")
    ms = lambda t: f"{t[0] * 1e3:.2f} [{t[1] * 1e3:.2f} .. {t[2] * 1e3:.2f}]"
    for name in ("shipped checkpoint", "untrained (seed 7)"):
        for greedy in (True, False):
            out = {}
            for one in (False, True):
                agent = IQNAgent(26, 9, device="cuda:0", seed=7 if name.startswith("untrained") else 3)
                if name.startswith("shipped"):
                    agent.load_model(os.path.join(G, "pretrained_IQN_seed3"), "cuda:0")
                env = VecMarineNavEnv(len(cfg), seed=0, device="cuda:0", precision="f64")
                with contextlib.redirect_stdout(io.StringIO()):
                    _time_eval(agent, env, cfg, greedy, one, 1)                       # warm-up (weight image, first launches)
                    agent = IQNAgent(26, 9, device="cuda:0", seed=7 if name.startswith("untrained") else 3)
                    if name.startswith("shipped"):
                        agent.load_model(os.path.join(G, "pretrained_IQN_seed3"), "cuda:0")
                    out[one] = _time_eval(agent, env, cfg, greedy, one, args.reps)
                env.close()
            steps = max(len(a) for a in out[True][1]["actions"])
            lo, hi = out[False][0][0] * 1e3, out[True][0][0] * 1e3
            print(f"{name:<22}{'greedy' if greedy else 'adaptive':<10}{steps:>6}{ms(out[False][0]):>28}{ms(out[True][0]):>28}{lo / hi:>9.1f}x{hi * 1e3 / steps:>15.2f}  "
                  f"{out[False][1] == out[True][1]}")
    if args.train:
        import subprocess
        import tempfile
        for flag in ([], ["--eval-one-launch"]):
            with tempfile.TemporaryDirectory() as d:
                conf = os.path.join(d, "config.json")
                with open(os.path.join(ROOT, "scripts", "config_IQN_example.json")) as f:
                    c = json.load(f)
                c["save_dir"] = d
                with open(conf, "w") as f:
                    json.dump(c, f)
                t0 = time.perf_counter()
                subprocess.run([sys.executable, "-m", "distributional_rl_navigation_amd.train_iqn", "-C", conf, "--n-evals", "300"] + flag,
                               cwd=ROOT, check=True, stdout=subprocess.DEVNULL)
                print(f"train_iqn default seed, --n-evals 300 {' '.join(flag) or '(loop)':<20}: {time.perf_counter() - t0:.1f} s wall")


if __name__ == "__main__":
    main()
