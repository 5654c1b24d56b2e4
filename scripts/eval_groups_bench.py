"""Measures the grouped IQN episode launch (mn_rollout_iqn_groups, iqn/deferred_eval.py) against the single-checkpoint path it replaces, on one GPU,
in one process, every shape warmed up, the forms alternating, medians of `--reps` with their ranges.  The yardstick is never the new launch: it is
`evaluation_vec(one_launch=True)`'s launch (one mn_rollout_iqn launch per checkpoint and policy on the 30 evaluation worlds).

1. Launch time.  The checkpoints are the evaluation points of a real default train_iqn run (4 096 envs, --eval-deferred --n-evals 300): early ones
   time out, late ones mostly succeed.  C = 30 and C = 300 of them, as ONE grouped launch (C x 60 rows) against 2 C single launches (greedy, adaptive;
   the checkpoint's weights copied into the network before its two launches, the worlds reloaded before each).  Wall time until the traces are
   complete on the device, the device time of the launches from HIP events, and the longest episode per group.  Before timing the two forms are compared:
   the grouped launch's greedy columns against the single greedy launches, and all 60 columns of every group against one 60-row launch per checkpoint.
2. Wall time of train_iqn at the default config: inline 30 points (--eval-one-launch), deferred 30, deferred 300; final evaluations side by side.

    python scripts/eval_groups_bench.py [--reps 5] [--out profiles/eval_groups_bench.txt] [--skip-train]
"""
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


def params_of(seed, save_dir):
    with open(os.path.join(ROOT, "scripts", "config_IQN_example.json")) as f:
        c = json.load(f)
    return dict(agent=c["agent"], seed=seed, total_timesteps=c["total_timesteps"], eval_freq=c["eval_freq"], save_dir=save_dir, training_time="bench")


def train(save_dir, **kw):
    import torch
    from distributional_rl_navigation_amd import train_iqn
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    with contextlib.redirect_stdout(io.StringIO()):
        d = train_iqn.run_trial("cuda:0", params_of(0, save_dir), 4096, verbose=False, **kw)
    torch.cuda.synchronize()
    return time.perf_counter() - t0, d


def final_scores(d):
    out = []
    for policy in ("greedy", "adaptive"):
        z = np.load(os.path.join(d, f"{policy}_evaluations.npz"), allow_pickle=True)
        out.append(f"{policy} {int(np.sum(z['successes'][-1]))}/30, return {float(np.mean(z['rewards'][-1])):.1f} ({len(z['timesteps'])} points)")
    return "; ".join(out)


def snapshot_run(tmp):
    """A default train_iqn run with --eval-deferred --n-evals 300 whose evaluation points are kept: (images, params, seeds, eval_config)."""
    from distributional_rl_navigation_amd.iqn import deferred_eval
    kept = {}

    class Keep(deferred_eval.DeferredEvaluations):
        def flush(self):
            if self.pending and "images" not in kept:
                n = len(self.pending)
                kept.update(images=self._images[:n].clone(), params=self._params[:n].clone(), seeds=[m["seed"] for m in self.pending], cfg=self.eval_config)
            return super().flush()

    orig, deferred_eval.DeferredEvaluations = deferred_eval.DeferredEvaluations, Keep
    try:
        secs, d = train(tmp, n_evals=300, eval_deferred=dict(max_pending=512, verbose=False))
    finally:
        deferred_eval.DeferredEvaluations = orig
    return kept, secs, d


def launch_times(kept, C, reps):
    import torch
    from distributional_rl_navigation_amd.episodes import EPISODE_TRACES
    from distributional_rl_navigation_amd.iqn.deferred_eval import GroupEnvs
    from distributional_rl_navigation_amd.iqn.fused_act import ActRng, rollout_iqn, rollout_iqn_groups, weights_changed
    from distributional_rl_navigation_amd.iqn.fused_train import flatten_network
    from distributional_rl_navigation_amd.iqn.model import ObsEncoder
    from distributional_rl_navigation_amd.marinenav_env.vec_env import VecMarineNavEnv
    dev, T = "cuda:0", 1000
    n_all = kept["images"].shape[0]
    pick = [int(round(x)) for x in np.linspace(0, n_all - 1, C)]
    images, params = kept["images"][pick].contiguous(), kept["params"][pick].contiguous()
    seeds = [kept["seeds"][j] for j in pick]
    cfg = kept["cfg"]
    W = len(cfg)
    genvs = GroupEnvs(cfg, True, dev, "f64")
    net = ObsEncoder(26, 9, seed=0, device=dev)
    flat = flatten_network(net)
    r0 = genvs.robot
    singles = {}
    for rows in (W, 2 * W):
        e = singles[rows] = VecMarineNavEnv(rows, device=dev, precision="f64")
        e.set_attrs(N=r0["N"], dt=r0["dt"])
    cv1, ad1 = genvs.rows(1)
    ev = lambda: torch.cuda.Event(enable_timing=True)

    def group():
        states = torch.tensor([[s, 0] for s in seeds], dtype=torch.int64, device=dev)
        cv, ad = genvs.rows(C)
        cv, ad = cv.to(dev), ad.to(dev)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        env = genvs.loaded(C)
        e0, e1 = ev(), ev()
        e0.record()
        tr = rollout_iqn_groups(images, env, T, states, genvs.R, cvar_rows=cv, adaptive_rows=ad, trace=EPISODE_TRACES)
        e1.record()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, e0.elapsed_time(e1) * 1e-3, tr

    def single(check=None):
        rngs = [ActRng(s, dev) for s in seeds]
        env = singles[W]
        evs = []
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for j in range(C):
            flat.copy_(params[j])
            weights_changed(net)
            for greedy in (True, False):
                env.load_worlds(genvs.worlds)
                e0, e1 = ev(), ev()
                e0.record()
                tr = rollout_iqn(net, env, T, rngs[j], cvar=1.0, adaptive=not greedy, trace=EPISODE_TRACES)
                e1.record()
                evs.append((e0, e1))
                if check is not None and greedy:
                    check(j, tr)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, sum(a.elapsed_time(b) for a, b in evs) * 1e-3

    # warm-up of both shapes, and the comparison of their results
    _, _, gtr = group()
    gtr = {k: gtr[k].clone() for k in EPISODE_TRACES + ("steps_run",)}
    R = genvs.R
    bad = []

    def same_greedy(j, tr):
        if not all(torch.equal(gtr[k][:, j * R:j * R + W], tr[k]) for k in EPISODE_TRACES):
            bad.append(("greedy columns", j))
    single(check=same_greedy)
    env60 = singles[2 * W]
    for j in range(C):      # every group against one launch of its own in the group's layout
        flat.copy_(params[j])
        weights_changed(net)
        env60.load_worlds(genvs.worlds, repeat=2)
        rng = ActRng(seeds[j], dev)
        tr = rollout_iqn(net, env60, T, rng, cvar_rows=cv1, adaptive_rows=ad1, trace=EPISODE_TRACES)
        if not (all(torch.equal(gtr[k][:, j * R:(j + 1) * R], tr[k]) for k in EPISODE_TRACES) and int(gtr["steps_run"][j]) == tr["steps_run"]):
            bad.append(("group", j))
    steps = gtr["steps_run"].cpu().numpy()
    say(f"C = {C} checkpoints ({C * R} workgroups grouped; {2 * C} single launches of {W} workgroups)")
    say(f"  results equal (greedy columns vs single greedy launches; all {R} columns vs a {R}-row launch per checkpoint): {'yes' if not bad else 'NO: ' + str(bad[:8])}")
    say(f"  longest episode per group: min {steps.min()}, median {int(np.median(steps))}, max {steps.max()}; groups at the {T}-step limit: {int((steps == T).sum())}")
    say(f"  steps_run per group: {' '.join(str(int(s)) for s in (steps if C <= 30 else steps[::10]))}" + ("" if C <= 30 else "  (every 10th)"))
    res = dict(group=([], []), single=([], []))
    for _ in range(reps):      # alternating
        w, d, _ = group()
        res["group"][0].append(w); res["group"][1].append(d)
        w, d = single()
        res["single"][0].append(w); res["single"][1].append(d)
    say(f"  (wall: from loading the worlds until the traces are complete on the device)")
    say(f"  one grouped launch : wall {fmt(res['group'][0])}, device (HIP events) {fmt(res['group'][1])}")
    say(f"  {2 * C:>3} single launches: wall {fmt(res['single'][0])}, device (HIP events, summed) {fmt(res['single'][1])}")
    say(f"  ratio single / grouped (medians): wall {med(res['single'][0])[0] / med(res['group'][0])[0]:.2f}x, device {med(res['single'][1])[0] / med(res['group'][1])[0]:.2f}x")
    genvs.close()
    for e in singles.values():
        e.close()
    return not bad


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "eval_groups_bench.txt"))
    ap.add_argument("--skip-train", action="store_true")
    args = ap.parse_args()
    import torch
    say(f"device: {torch.cuda.get_device_name(0)}, {torch.cuda.get_device_properties(0).multi_processor_count} CUs; 30 evaluation worlds, f64 env kernels; "
        f"medians of {args.reps} [min .. max]; forms alternate within one process")
    with tempfile.TemporaryDirectory() as tmp:
        kept, secs, d = snapshot_run(os.path.join(tmp, "snap"))
        say(f"checkpoints: the {kept['images'].shape[0]} evaluation points of one default train_iqn run (4 096 envs, seed 0, --eval-deferred --n-evals 300; {secs:.1f} s incl. warm-up)")
        say()
        say("== launch time: one grouped launch against 2 C single launches (evaluation_vec(one_launch=True)'s launch) ==")
        for C in (30, 300):
            launch_times(kept, C, args.reps)
        if not args.skip_train:
            say()
            say("== wall time of train_iqn, default config (4 096 envs, seed 0), whole run_trial incl. env and agent construction ==")
            forms = (("inline 30 (--eval-one-launch)", dict(eval_one_launch=True)),
                     ("deferred 30 (--eval-deferred)", dict(eval_deferred=True)),
                     ("deferred 300 (--eval-deferred --n-evals 300)", dict(eval_deferred=True, n_evals=300)))
            for i, (name, kw) in enumerate(forms):      # warm-up of every form
                train(os.path.join(tmp, f"warm{i}"), **kw)
            times, last = {name: [] for name, _ in forms}, {}
            for r in range(args.reps):
                for i, (name, kw) in enumerate(forms):
                    s, dd = train(os.path.join(tmp, f"r{r}_{i}"), **kw)
                    times[name].append(s)
                    last[name] = dd
                print(f"  rep {r} done", flush=True)
            for name, _ in forms:
                say(f"  {name:<46}: {fmt(times[name], 1.0, 's')}   final evaluation: {final_scores(last[name])}")
            a, b = times[forms[0][0]], times[forms[1][0]]
            spread = max(max(a) - min(a), max(b) - min(b))
            diff = med(b)[0] - med(a)[0]
            say(f"  deferred 30 - inline 30 (medians): {diff:+.2f} s; run-to-run spread (the larger range of the two): {spread:.2f} s -> "
                f"{'deferred 30 is not slower than inline 30 beyond the spread' if diff <= spread else 'CONDITION FAILED: deferred 30 is slower than inline 30 beyond the spread'}")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
