"""What training G IQN learners in grouped launches (mn_iqn_group_train_step, iqn/group_train.py) costs or buys against G single steps.

    python scripts/iqn_group_train_bench.py [--out profiles/iqn_group_train_bench.txt] [--skip-learner] [--end-to-end [--total-timesteps N]]

The grouped step is three launches (forward / backward with both forwards in every workgroup, reduction, clip + Adam) with the learner as a grid dimension;
the single step (`agent.train_from_memory()`, the default form) is one or two launches whose workgroups wait for each other.  No speed-up is promised: G = 1
is expected to lose, and whether G = 5 at batch 32 beats five fused steps is what this file is for.

(a) learner alone, G in {1, 5, 16, 64}, every learner with its own ring, networks and Adam state, at batch 32 and 256: `LearnerGroup.train()` against
    G x `agent.train_from_memory()`.  Two equal sets of agents, one per form; before timing, both run the same number of steps and every learner's
    parameters are compared for equality.  Host clock around a synchronise, both forms in one process, alternating; every shape warmed up; medians of 5
    windows with min-max ranges, a window being as many calls as take about 0.3 s.
(b) --end-to-end: the five-seed IQN config with `--env-budget reference`, sequential against `--together` (wall time of the whole command), and the
    files of both runs compared for equality.  `--total-timesteps` shortens the runs (the reference's: 3 000 000); the file states the value used.
There is no CPU form of either: without a GPU the script fails.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
GS = (1, 5, 16, 64)
WINDOWS, WINDOW_S, CHECK_STEPS = 5, 0.3, 3
CONFIG_IQN = {"agent": "IQN", "seed": [0, 1, 2, 3, 4], "total_timesteps": 3_000_000, "eval_freq": 10_000, "save_dir": "iqn_runs"}
RING = 16_384


def learner_alone(lines):
    import torch
    from distributional_rl_navigation_amd.iqn.agent import IQNAgent
    from distributional_rl_navigation_amd.iqn.group_train import LearnerGroup
    from distributional_rl_navigation_amd.marinenav_env.vec_env import VecMarineNavEnv
    dev = "cuda:0"
    rings = []
    for seed in (5, 6, 7, 8):
        env = VecMarineNavEnv(1024, seed=seed, device=dev)
        ag = IQNAgent(26, 9, BATCH_SIZE=32, BUFFER_SIZE=RING, device=dev, seed=seed)
        obs = env.reset()
        for _ in range(16):
            a = ag.act_batch(obs, 1.0)
            nxt, r, d, _ = env.step(a)
            ag.memory.add_vector_step(obs, a, r, nxt, d)
            obs = env.reset_done()
        env.close()
        m = ag.memory
        rings.append(tuple(t.clone() for t in (m.states, m.actions, m.rewards, m.next_states, m.dones)))

    def agents(batch, n):
        out = []
        for g in range(n):
            ag = IQNAgent(26, 9, BATCH_SIZE=batch, BUFFER_SIZE=RING, device=dev, seed=100 + g)
            m = ag.memory
            for dst, src in zip((m.states, m.actions, m.rewards, m.next_states, m.dones), rings[g % len(rings)]):
                dst.copy_(src)
            m.size, m.ptr = m.capacity, 0
            m.version += 1
            out.append(ag)
        return out

    def window(fn, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n

    def compare(name, G, grouped, single):
        for fn in (grouped, single):      # warm-up: buffers, the act image's flag, the clocks
            for _ in range(3):
                fn()
        n = {id(fn): max(3, int(WINDOW_S / max(window(fn, 3), 1e-6))) for fn in (grouped, single)}
        t = {id(grouped): [], id(single): []}
        for _ in range(WINDOWS):
            for fn in (grouped, single):
                t[id(fn)].append(window(fn, n[id(fn)]))
        row = f"{name:16s} G={G:2d}"
        for label, fn in (("grouped", grouped), ("single", single)):
            us = sorted(1e6 * x for x in t[id(fn)])
            med = statistics.median(us)
            row += f" | {label}: {med:9.1f} us/call [{us[0]:.1f}-{us[-1]:.1f}], {med / G:7.2f} us/learner-step, {n[id(fn)]} calls/window"
        row += f" | single/grouped = {statistics.median(t[id(single)]) / statistics.median(t[id(grouped)]):.2f}x"
        lines.append(row)
        print(row, flush=True)

    lines.append(f"(a) learner alone on {torch.cuda.get_device_name(0)}: medians of {WINDOWS} alternating windows of ~{WINDOW_S} s [min-max]; 'call' = all G learners "
                 f"once; grouped = LearnerGroup.train() (3 launches), single = G x agent.train_from_memory() (default form); before timing, the parameters of "
                 f"both forms after {CHECK_STEPS} steps were compared for equality")
    for batch in (32, 256):
        pool_g, pool_s = agents(batch, max(GS)), agents(batch, max(GS))
        lines.append(f"  batch {batch}: the single step takes {pool_s[0]._fused_trainer().launches_per_step(batch)} launch(es) on this device")
        for G in GS:
            ags_g, ags_s = pool_g[:G], pool_s[:G]
            group = LearnerGroup(ags_g)
            grouped, single = group.train, lambda: [ag.train_from_memory() for ag in ags_s]
            for _ in range(CHECK_STEPS):
                grouped()
                single()
            torch.cuda.synchronize()
            for g, (a, b) in enumerate(zip(ags_g, ags_s)):
                if not torch.equal(a._fused.local.view(torch.int32), b._fused.local.view(torch.int32)) or not bool(torch.isfinite(a._fused.local).all()):
                    raise SystemExit(f"iqn_group_train_bench: batch {batch}, G = {G}: learner {g}'s parameters differ between the grouped and the single form")
                if a._fused.timeouts() or b._fused.timeouts():
                    raise SystemExit(f"iqn_group_train_bench: batch {batch}, G = {G}: learner {g}: a bounded wait of the gradient step ran out")
            compare(f"step, batch {batch}", G, grouped, single)
            group.close()
            # (the sets stay equal for the next G only if both forms have done the same number of steps: bring the lagging one level)
            for a, b in zip(ags_g, ags_s):
                a.memory.version += 1
                b.memory.version += 1
                b._fused.local.copy_(a._fused.local); b._fused.exp_avg.copy_(a._fused.exp_avg); b._fused.exp_avg_sq.copy_(a._fused.exp_avg_sq)
                b._fused.step_dev.copy_(a._fused.step_dev); b._fused.rng_state.copy_(a._fused.rng_state)
        del pool_g, pool_s


def _nested_equal(a, b):
    import numpy as np
    if isinstance(a, (list, tuple)) or (isinstance(a, np.ndarray) and a.dtype == object):
        return isinstance(b, (list, tuple, np.ndarray)) and len(a) == len(b) and all(_nested_equal(x, y) for x, y in zip(a, b))
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=np.asarray(a).dtype.kind == "f")


def _file_equal(fa, fb):
    """(equal, things compared) of one file of the two runs."""
    import numpy as np
    import torch
    if fa.endswith(".npz"):
        za, zb = np.load(fa, allow_pickle=True), np.load(fb, allow_pickle=True)
        return sorted(za.files) == sorted(zb.files) and all(_nested_equal(za[k], zb[k]) for k in za.files), len(za.files)
    if fa.endswith(".pth"):
        sa, sb = torch.load(fa, map_location="cpu"), torch.load(fb, map_location="cpu")
        return list(sa) == list(sb) and all(torch.equal(sa[k].view(torch.int32), sb[k].view(torch.int32)) for k in sa), len(sa)
    if fa.endswith(".json"):
        ja, jb = json.load(open(fa)), json.load(open(fb))
        for j in (ja, jb):      # (the runs' own directories and start times)
            if isinstance(j, dict):
                j.pop("save_dir", None)
                j.pop("training_time", None)
        return ja == jb, 1
    return open(fa, "rb").read() == open(fb, "rb").read(), 1


def end_to_end(lines, total_timesteps):
    lines.append(f"(b) end to end: config_IQN.json (seeds 0-4) with total_timesteps = {total_timesteps} (the reference's: 3 000 000), --env-budget reference; wall time "
                 "of the whole command")
    with tempfile.TemporaryDirectory() as tmp:
        cfg = os.path.join(tmp, "config_IQN.json")
        runs = {}
        for name, extra in (("sequential", []), ("together", ["--together"])):
            save = os.path.join(tmp, name)
            with open(cfg, "w") as f:
                json.dump(dict(CONFIG_IQN, total_timesteps=total_timesteps, save_dir=save), f)
            t0 = time.perf_counter()
            r = subprocess.run([sys.executable, "-m", "distributional_rl_navigation_amd.train_iqn", "-C", cfg, "--env-budget", "reference", *extra], cwd=ROOT,
                               capture_output=True, text=True)
            dt = time.perf_counter() - t0
            if r.returncode:
                lines.append(f"  {name}: FAILED ({r.returncode}): {r.stderr[-400:]}")
                raise SystemExit(lines[-1])
            runs[name] = os.path.join(save, os.listdir(save)[0])
            row = f"  {name:10s}: {dt:8.1f} s"
            lines.append(row)
            print(row, flush=True)
        same, checked = True, 0
        for seed in CONFIG_IQN["seed"]:
            da, db = (os.path.join(runs[n], f"seed_{seed}") for n in ("sequential", "together"))
            if sorted(os.listdir(da)) != sorted(os.listdir(db)):
                same = False
                lines.append(f"  seed {seed}: different files {sorted(os.listdir(da))} / {sorted(os.listdir(db))}")
                continue
            for f in sorted(os.listdir(da)):
                ok, n = _file_equal(os.path.join(da, f), os.path.join(db, f))
                checked += n
                if not ok:
                    same = False
                    lines.append(f"  seed {seed}: {f} differs")
        lines.append(f"  files of both runs, five seeds (npz array by array, network tensors as bytes, JSON without the runs' directory and start time): "
                     f"{'EQUAL' if same else 'DIFFERENT'} ({checked} arrays / tensors / files)")
        print(lines[-1], flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "iqn_group_train_bench.txt"))
    ap.add_argument("--skip-learner", action="store_true")
    ap.add_argument("--end-to-end", action="store_true")
    ap.add_argument("--total-timesteps", type=int, default=3_000_000, help="of the end-to-end runs (the reference's: 3 000 000)")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("iqn_group_train_bench: no GPU visible -- both forms of the gradient step are HIP kernels, there is nothing to measure without one")
    lines = ["# scripts/iqn_group_train_bench.py" + (" --end-to-end --total-timesteps %d" % args.total_timesteps if args.end_to_end else "")]
    if args.skip_learner:
        lines.append("(a) learner alone: not measured in this run (run without --skip-learner)")
    else:
        learner_alone(lines)
    if args.end_to_end:
        end_to_end(lines, args.total_timesteps)
    else:
        lines.append("(b) end to end: not measured in this run (--end-to-end)")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
