"""Measures the grouped DQN episode launch (mn_rollout_dqn_groups, dqn/deferred_eval.py) against the single-checkpoint path it replaces, on one GPU,
in one process, every shape warmed up, the forms alternating, medians of `--reps` with their ranges.  The yardstick is never the new launch: it is
`train_dqn.evaluate(one_launch=True)`'s launch (one mn_rollout_dqn launch per checkpoint on the 30 evaluation worlds).

1. Launch time.  The checkpoints are the evaluation points of a real default train_dqn run (4 096 envs, --eval-deferred --n-evals 300).  C = 30, 64
   and 300 of them, as ONE grouped launch (C x 30 rows, 4 C workgroups) against C single launches (the checkpoint's weights copied into the policy
   before its launch, the worlds reloaded before each).  Wall time until the traces are complete on the device, the device time of the launches from
   HIP events, and the longest episode per group.  Before timing the two forms are compared: every group's columns against its single launch.
2. Wall time of train_dqn at the default config: inline 30 points (--eval-one-launch), deferred 30, deferred 300; final evaluations side by side.

    python scripts/eval_dqn_groups_bench.py [--reps 5] [--train-reps N] [--out profiles/eval_dqn_groups_bench.txt] [--skip-train | --skip-launch --append]

A default train_dqn run is about a minute (375 000 fused gradient steps), so part 2 is 3 x `--train-reps` minutes; `--skip-launch --append` runs it
as a second process and appends to the file part 1 wrote.
"""
import argparse
import contextlib
import io
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LINES = []


def say(s=""):
    print(s, flush=True)
    LINES.append(s)


def med(ts):
    ts = sorted(ts)
    return ts[len(ts) // 2], ts[0], ts[-1]


def fmt(ts, scale=1e3, unit="ms"):
    m, lo, hi = med(ts)
    return f"{m * scale:.1f} [{lo * scale:.1f} .. {hi * scale:.1f}] {unit}"


def params_of(seed, save_dir):      # the reference's config_DQN.json
    return dict(agent="DQN", seed=seed, total_timesteps=3_000_000, eval_freq=10_000, save_dir=save_dir, training_time="bench")


def train(save_dir, **kw):
    import torch
    from distributional_rl_navigation_amd import train_dqn
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    with contextlib.redirect_stdout(io.StringIO()):
        d = train_dqn.run_trial("cuda:0", params_of(0, save_dir), 4096, verbose=False, **kw)
    torch.cuda.synchronize()
    return time.perf_counter() - t0, d


def final_scores(d):
    z = np.load(os.path.join(d, "evaluations.npz"), allow_pickle=True)
    return f"{int(np.sum(z['successes'][-1]))}/30, return {float(np.mean(z['rewards'][-1])):.1f} ({len(z['timesteps'])} points)"


def snapshot_run(tmp):
    """A default train_dqn run with --eval-deferred --n-evals 300 whose evaluation points are kept: (images, local parameters, eval_config)."""
    from distributional_rl_navigation_amd.dqn import deferred_eval
    kept = {}

    class Keep(deferred_eval.DeferredEvaluations):
        def flush(self):
            if self.pending and "images" not in kept:
                n = len(self.pending)
                kept.update(images=self._images[:n].clone(), params=self._local[:n].clone(), cfg=self.eval_config)
            return super().flush()

    orig, deferred_eval.DeferredEvaluations = deferred_eval.DeferredEvaluations, Keep
    try:
        secs, d = train(tmp, n_evals=300, eval_deferred=dict(max_pending=512, verbose=False))
    finally:
        deferred_eval.DeferredEvaluations = orig
    return kept, secs, d


def launch_times(kept, C, reps):
    import torch
    from distributional_rl_navigation_amd.dqn import DQNPolicy
    from distributional_rl_navigation_amd.dqn.fused_train import flatten_network
    from distributional_rl_navigation_amd.dqn.policy import rollout_dqn_groups
    from distributional_rl_navigation_amd.episodes import EPISODE_TRACES, steps_run
    from distributional_rl_navigation_amd.iqn.deferred_eval import GroupEnvs
    from distributional_rl_navigation_amd.marinenav_env.vec_env import VecMarineNavEnv
    dev, T = "cuda:0", 1000
    n_all = kept["images"].shape[0]
    pick = [int(round(x)) for x in np.linspace(0, n_all - 1, C)]
    images, params = kept["images"][pick].contiguous(), kept["params"][pick].contiguous()
    cfg = kept["cfg"]
    genvs = GroupEnvs(cfg, False, dev, "f64")
    R, r0 = genvs.R, genvs.robot
    pol = DQNPolicy(device=dev)
    flat = flatten_network(pol.q_net)
    env1 = VecMarineNavEnv(R, device=dev, precision="f64")
    env1.set_attrs(N=r0["N"], dt=r0["dt"])
    ev = lambda: torch.cuda.Event(enable_timing=True)

    def group():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        env = genvs.loaded(C)
        e0, e1 = ev(), ev()
        e0.record()
        tr = rollout_dqn_groups(images, env, T, R, trace=EPISODE_TRACES)
        e1.record()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, e0.elapsed_time(e1) * 1e-3, tr

    def single(check=None):
        evs = []
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for j in range(C):
            flat.copy_(params[j])
            pol.weights_changed()
            env1.load_worlds(genvs.worlds)
            e0, e1 = ev(), ev()
            e0.record()
            tr = pol.rollout(env1, T, trace=EPISODE_TRACES)      # evaluate(one_launch=True)'s launch, incl. the repack in front of it
            e1.record()
            evs.append((e0, e1))
            if check is not None:
                check(j, tr)
        torch.cuda.synchronize()
        each = [a.elapsed_time(b) * 1e-3 for a, b in evs]
        return time.perf_counter() - t0, sum(each), each

    # warm-up of both shapes, and the comparison of their results
    _, _, gtr = group()
    gtr = {k: gtr[k].clone() for k in EPISODE_TRACES}
    bad = []
    single(check=lambda j, tr: None if all(torch.equal(gtr[k][:, j * R:(j + 1) * R], tr[k]) for k in EPISODE_TRACES) else bad.append(j))
    done = gtr["done"].cpu().numpy()
    steps = np.array([steps_run(done[:, j * R:(j + 1) * R]) for j in range(C)])
    wpg = -(-R // 8)
    say(f"C = {C} checkpoints ({C * wpg} workgroups grouped; {C} single launches of {wpg} workgroups)")
    say(f"  results equal (every group's {R} columns vs the checkpoint's single launch): {'yes' if not bad else 'NO: ' + str(bad[:8])}")
    say(f"  longest episode per group: min {steps.min()}, median {int(np.median(steps))}, max {steps.max()}; groups at the {T}-step limit: {int((steps == T).sum())}")
    res = dict(group=([], []), single=([], []))
    each_all = []
    for _ in range(reps):      # alternating
        w, d, _ = group()
        res["group"][0].append(w); res["group"][1].append(d)
        w, d, each = single()
        res["single"][0].append(w); res["single"][1].append(d)
        each_all.append(each)
    each = np.median(np.array(each_all), axis=0)
    say(f"  (wall: from loading the worlds until the traces are complete on the device)")
    say(f"  one grouped launch : wall {fmt(res['group'][0])}, device (HIP events) {fmt(res['group'][1])}")
    say(f"  {C:>3} single launches: wall {fmt(res['single'][0])}, device (HIP events, summed) {fmt(res['single'][1])}; one launch: mean {each.mean() * 1e3:.2f} ms, "
        f"slowest {each.max() * 1e3:.2f} ms")
    say(f"  ratio single / grouped (medians): wall {med(res['single'][0])[0] / med(res['group'][0])[0]:.2f}x, device {med(res['single'][1])[0] / med(res['group'][1])[0]:.2f}x; "
        f"grouped launch / slowest single launch (device): {med(res['group'][1])[0] / each.max():.2f}")
    for kind in (0, 1):
        sep = min(res["single"][kind]) > max(res["group"][kind])
        say(f"  {'wall' if kind == 0 else 'device'}: the grouped form is {'faster, the ranges do not overlap' if sep else 'NOT faster beyond the run-to-run spread (the ranges overlap)'}")
    genvs.close()
    env1.close()
    return not bad


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "eval_dqn_groups_bench.txt"))
    ap.add_argument("--train-reps", type=int, default=None, help="repetitions of part 2 (default: --reps)")
    ap.add_argument("--skip-train", action="store_true")
    ap.add_argument("--skip-launch", action="store_true")
    ap.add_argument("--append", action="store_true", help="append to --out instead of replacing it")
    args = ap.parse_args()
    import torch
    say(f"device: {torch.cuda.get_device_name(0)}, {torch.cuda.get_device_properties(0).multi_processor_count} CUs; 30 evaluation worlds, f64 env kernels; "
        f"medians [min .. max]; forms alternate within one process")
    train_reps = args.train_reps or args.reps
    with tempfile.TemporaryDirectory() as tmp:
        if not args.skip_launch:
            kept, secs, d = snapshot_run(os.path.join(tmp, "snap"))
            say(f"checkpoints: the {kept['images'].shape[0]} evaluation points of one default train_dqn run (4 096 envs, seed 0, --eval-deferred --n-evals 300; {secs:.1f} s incl. warm-up)")
            say()
            say(f"== launch time: one grouped launch against C single launches (evaluate(one_launch=True)'s launch); medians of {args.reps} ==")
            for C in (30, 64, 300):
                launch_times(kept, C, args.reps)
        if not args.skip_train:
            say()
            say(f"== wall time of train_dqn, default config (4 096 envs, seed 0), whole run_trial incl. env and agent construction; medians of {train_reps} ==")
            forms = (("inline 30 (--eval-one-launch)", dict(eval_one_launch=True)),
                     ("deferred 30 (--eval-deferred)", dict(eval_deferred=True)),
                     ("deferred 300 (--eval-deferred --n-evals 300)", dict(eval_deferred=True, n_evals=300)))
            for i, (name, kw) in enumerate(forms):      # warm-up of every form: a short run (every kernel, every file, the allocator)
                train(os.path.join(tmp, f"warm{i}"), total_grad_steps=6000, **kw)
            times, last = {name: [] for name, _ in forms}, {}
            for r in range(train_reps):
                for i, (name, kw) in enumerate(forms):
                    s, dd = train(os.path.join(tmp, f"r{r}_{i}"), **kw)
                    times[name].append(s)
                    last[name] = dd
                print(f"  rep {r} done", flush=True)
            for name, _ in forms:
                say(f"  {name:<46}: {fmt(times[name], 1.0, 's')}   final evaluation: {final_scores(last[name])}")
            za, zb = (np.load(os.path.join(last[forms[k][0]], "evaluations.npz"), allow_pickle=True) for k in (0, 1))
            same = all(za[k].tolist() == zb[k].tolist() for k in za.files)
            say(f"  evaluations.npz of deferred 30 equals inline 30's, array by array: {'yes' if same else 'NO'}")
            a, b = times[forms[0][0]], times[forms[1][0]]
            spread = max(a) - min(a)
            diff = med(b)[0] - med(a)[0]
            say(f"  deferred 30 - inline 30 (medians): {diff:+.2f} s; spread of the repeated inline runs: {spread:.2f} s -> "
                f"{'deferred 30 is not slower than inline 30 beyond the spread' if diff <= spread else 'CONDITION FAILED: deferred 30 is slower than inline 30 beyond the spread'}")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a" if args.append else "w") as f:
        f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
