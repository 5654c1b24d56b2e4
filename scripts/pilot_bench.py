"""Times the field pilot on one MI355X and writes profiles/pilot_bench.txt.

    python scripts/pilot_bench.py [--out FILE] [--reps 5] [--parent DIR] [--bench-steps 200] [--bench-warmup 20]

Medians of `--reps` timed windows after a warm-up window, the cases alternating in one process, every call synchronised; wall time with the range.
  * the 30 worlds of tests/golden/eval_config_seed3.json, 64 x 64 fields, H = 2, 60 steps: VecMarineNavEnv.rollout_pilot (one launch) against its own
    loop of (get_state, pilot_act, step); each window reloads the worlds first (not timed);
  * pilot_act at 65 536 and 1 048 576 random poses in world 10, beside step_at (the what-if step) on the same poses x 9 actions -- the work a
    horizon-1 pilot call contains;
  * with --parent DIR (a built checkout of the parent commit): `python bench.py --gpus 1 --steps K --warmup W` here and there, alternating, three runs
    each -- bench.py runs none of the pilot's code, so the ranges should overlap.  Without it that part is marked as not measured.
Nothing is asserted."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
G = os.path.join(ROOT, "tests", "golden")


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pilot_bench.txt"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--parent", default=None, metavar="DIR")
    ap.add_argument("--bench-steps", type=int, default=200)
    ap.add_argument("--bench-warmup", type=int, default=20)
    ap.add_argument("--device", default="cuda:0")
    args = ap.parse_args(argv)
    import numpy as np
    import torch
    from distributional_rl_navigation_amd.marinenav_env.vec_env import VecMarineNavEnv
    with open(os.path.join(G, "eval_config_seed3.json")) as f:
        cfg = json.load(f)
    worlds = [VecMarineNavEnv.world_from_eval_config(cfg[f"env_{k}"]) for k in range(len(cfg))]
    n, H, steps = len(worlds), 2, 60
    env = VecMarineNavEnv(n, device=args.device, precision="f64")
    env.load_worlds(worlds)
    T, _, _, _ = env.time_field(np.arange(n, dtype=np.int32), 64, 64, want_dir=False, want_sweeps=False)
    idx = torch.arange(n, dtype=torch.int32, device=env.device)
    sync = lambda: torch.cuda.synchronize(env.device)

    def launch():
        env.rollout_pilot(steps, T, horizon=H)

    def loop():
        for _ in range(steps):
            s, ep, _ = env.get_state()
            a = env.pilot_act(s, T, env=idx, field_of_query=idx, horizon=H, episode_timesteps=ep, want=("action",))["action"]
            env.step(a)

    rng = np.random.default_rng(0)
    poses = {}
    for q in (65536, 1048576):
        st = np.zeros((q, 6))
        st[:, 0], st[:, 1] = rng.uniform(0, 50, q), rng.uniform(0, 50, q)
        st[:, 2], st[:, 3] = rng.uniform(0, 2 * np.pi, q), rng.uniform(0, 2, q)
        st = torch.as_tensor(st, device=env.device)
        poses[q] = (st, st.repeat_interleave(9, dim=0), torch.arange(9, dtype=torch.int32, device=env.device).repeat(q))
    cases = [("rollout_pilot, 30 worlds, 60 steps, H = 2: one launch", launch, True), ("  its loop (get_state, pilot_act, step) x 60", loop, True)]
    for q, (st, st9, a9) in poses.items():
        for h in (1, 2):
            cases.append((f"pilot_act, {q} poses, H = {h}", lambda st=st, h=h: env.pilot_act(st, T[10], env=10, horizon=h), False))
        cases.append((f"  step_at on the same {q} poses x 9 actions", lambda st9=st9, a9=a9: env.step_at(st9, a9, env=10), False))
    times = {label: [] for label, _, _ in cases}
    for rep in range(args.reps + 1):      # (window 0 warms up)
        for label, fn, reload in cases:
            if reload:
                env.load_worlds(worlds)
            sync()
            t0 = time.perf_counter()
            fn()
            sync()
            if rep:
                times[label].append(time.perf_counter() - t0)
    lines = [f"# scripts/pilot_bench.py on {torch.cuda.get_device_name(env.device)}: medians of {args.reps} windows after a warm-up window, cases alternating, "
             "every call synchronised (wall time; range in brackets)"]
    for label, _, _ in cases:
        t = np.array(times[label]) * 1e3
        lines.append(f"{label}: {np.median(t):.3f} ms [{t.min():.3f} .. {t.max():.3f}]")
    env.close()
    if args.parent:
        runs = {"this tree": [], "parent": []}
        for _ in range(3):
            for name, cwd in (("this tree", ROOT), ("parent", args.parent)):
                r = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", str(args.bench_steps), "--warmup", str(args.bench_warmup)], cwd=cwd,
                                   capture_output=True, text=True, timeout=900)
                line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
                runs[name].append(json.loads(line[-1])["value"] if r.returncode == 0 and line else float("nan"))
        for name, v in runs.items():
            lines.append(f"bench.py --gpus 1 --steps {args.bench_steps} --warmup {args.bench_warmup}, {name}: " + ", ".join(f"{x:.4g}" for x in v))
    else:
        lines.append("bench.py against the parent commit: not measured (no --parent checkout given)")
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
