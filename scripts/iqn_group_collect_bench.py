"""What collecting for G IQN seeds through ONE stacked env handle (mn_iqn_actor_group_act / _append, iqn/group_collect.py, train_iqn --together --stack-envs)
costs or buys against G per-seed collects.

    python scripts/iqn_group_collect_bench.py [--out profiles/iqn_group_collect_bench.txt] [--gs 1,5,16,64] [--skip-loop] [--end-to-end [--total-timesteps N]]

Nothing is promised: the stacked collect stays opt-in whatever comes out.

(a) the lockstep vector step, G in {1, 5, 16, 64}, at two cadences: n = 80 rows per seed with 20 gradient steps of batch 32 (the reference-budget cadence), and
    n = 4 096 with one gradient step of batch 256 (the learner-budget default).  Both forms in one process on two equal sets of agents and envs, the gradient
    steps of both through a LearnerGroup, one device synchronisation per vector step as in `run_trials_together`; eps = 0.05.  stacked: CollectorGroup.act, one
    mn_step, CollectorGroup.append, one mn_reset_done; per seed: G x (act_batch, mn_step_append, mn_reset_done).  Also the collect phase alone (no gradient steps).
    Before timing both sets run the same steps and every seed's ring, act generator state and parameters are compared for equality.
(b) the workgroups per group of the grouped act launch: the library's rule min(ceil(n / 8), max(1, CUs / G)) against ceil(n / 8) per group (mn_iqn_set_grid on
    the first context), the act call alone.
(c) the per-vector-step synchronise of the stacked loop at G = 5: with it, and with one synchronisation per window.
(d) --end-to-end: the five-seed IQN config with `--env-budget reference`: sequential, `--together`, `--together --stack-envs` (wall time of the whole command),
    and the files of the runs compared for equality.
Host clock around a synchronise; every shape warmed up; medians of 5 alternating windows of ~0.3 s with min-max ranges.  Without a GPU the script fails.
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
WINDOWS, WINDOW_S, CHECK_STEPS, EPS = 5, 0.3, 4, 0.05
CONFIG_IQN = {"agent": "IQN", "seed": [0, 1, 2, 3, 4], "total_timesteps": 3_000_000, "eval_freq": 10_000, "save_dir": "iqn_runs"}
CADENCES = (dict(name="n = 80, 20 x batch 32", n=80, batch=32, grad=20, ring=16_384), dict(name="n = 4096, 1 x batch 256", n=4096, batch=256, grad=1, ring=32_768))
DEV = "cuda:0"


def _window(torch, fn, n, sync_each):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
        if sync_each:
            torch.cuda.synchronize()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n


def _compare(torch, lines, name, forms, sync_each=True):
    """`forms`: [(label, fn)] timed in alternating windows; one row with each form's median and range, and the first form over every other."""
    for _, fn in forms:
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    calls = [max(3, int(WINDOW_S / max(_window(torch, fn, 3, sync_each), 1e-6))) for _, fn in forms]
    t = [[] for _ in forms]
    for _ in range(WINDOWS):
        for k, (_, fn) in enumerate(forms):
            t[k].append(_window(torch, fn, calls[k], sync_each))
    row, med = f"{name:44s}", []
    for k, (label, _) in enumerate(forms):
        us = sorted(1e6 * x for x in t[k])
        med.append(statistics.median(us))
        row += f" | {label}: {med[-1]:9.1f} us [{us[0]:.1f}-{us[-1]:.1f}], {calls[k]} calls/window"
    for k in range(1, len(forms)):
        row += f" | {forms[k][0]} / {forms[0][0]} = {med[k] / med[0]:.2f}x"
    lines.append(row)
    print(row, flush=True)
    return med, t


class Lines(list):
    """The report: every line goes to the file as it is added, so a run that is cut short leaves what it measured."""

    def __init__(self, path):
        super().__init__()
        self.path = path
        os.makedirs(os.path.dirname(path), exist_ok=True)

    def append(self, line):
        super().append(line)
        with open(self.path, "w") as f:
            f.write("\n".join(self) + "\n")


class Seeds:
    """G agents with their replay rings and a LearnerGroup; `stacked`: one env handle and a CollectorGroup, else an env per agent."""

    def __init__(self, torch, G, cad, stacked):
        from distributional_rl_navigation_amd.iqn.agent import IQNAgent
        from distributional_rl_navigation_amd.iqn.group_collect import CollectorGroup
        from distributional_rl_navigation_amd.iqn.group_train import LearnerGroup
        from distributional_rl_navigation_amd.marinenav_env.vec_env import VecMarineNavEnv, stacked_seeds
        self.torch, self.G, self.n, self.grad, self.stacked = torch, G, cad["n"], cad["grad"], stacked
        self.agents = [IQNAgent(26, 9, BATCH_SIZE=cad["batch"], BUFFER_SIZE=cad["ring"], device=DEV, seed=100 + g, UPDATE_EVERY=1, learning_starts=0) for g in range(G)]
        self.group = LearnerGroup(self.agents)
        if stacked:
            self.envs = [VecMarineNavEnv(G * self.n, seeds=stacked_seeds(self.n, range(G)), device=DEV, precision="f64")]
            self.collectors = CollectorGroup(self.agents, self.envs[0])
            self.obs = self.envs[0].reset()
        else:
            self.envs = [VecMarineNavEnv(self.n, seed=g, device=DEV, precision="f64") for g in range(G)]
            self.obs = [e.reset() for e in self.envs]

    def collect(self):
        if self.stacked:
            env = self.envs[0]
            actions = self.collectors.act(self.obs, EPS)
            nxt, reward, done, _ = env.step(actions)
            self.collectors.append(self.obs, actions, reward, nxt, done)
            self.obs = env.reset_done()
        else:
            for g, (ag, env) in enumerate(zip(self.agents, self.envs)):
                actions = ag.act_batch(self.obs[g], EPS)
                env.step_append(actions, self.obs[g], ag.memory)
                self.obs[g] = env.reset_done()

    def step(self):
        self.collect()
        self.group.train_many(self.grad)

    def act_only(self):
        self.collectors.act(self.obs, EPS)

    def close(self):
        self.torch.cuda.synchronize()
        self.group.close()
        if self.stacked:
            self.collectors.close()
        for e in self.envs:
            e.close()


def _check_equal(torch, a, b, where):
    torch.cuda.synchronize()
    for g, (x, y) in enumerate(zip(a.agents, b.agents)):
        same = x.memory.size == y.memory.size and x.memory.ptr == y.memory.ptr and x._act_rng.state.tolist() == y._act_rng.state.tolist()
        for k in ("states", "next_states", "actions", "rewards", "dones"):
            same = same and torch.equal(getattr(x.memory, k)[:x.memory.size], getattr(y.memory, k)[:y.memory.size])
        same = same and torch.equal(x._fused.local.view(torch.int32), y._fused.local.view(torch.int32)) and bool(torch.isfinite(x._fused.local).all())
        if not same:
            raise SystemExit(f"iqn_group_collect_bench: {where}: seed {g} differs between the stacked and the per-seed form")
        if x._fused.timeouts() or y._fused.timeouts():
            raise SystemExit(f"iqn_group_collect_bench: {where}: seed {g}: a bounded wait of the gradient step ran out")


def lockstep(lines, gs):
    import torch
    lines.append(f"(a) lockstep vector step on {torch.cuda.get_device_name(0)}: medians of {WINDOWS} alternating windows of ~{WINDOW_S} s [min-max], host clock, one device "
                 f"synchronisation per vector step; 'call' = one vector step of all G seeds; eps = {EPS}; before timing, rings, act generator states and parameters of "
                 f"both forms after {CHECK_STEPS} steps were compared for equality")
    for cad in CADENCES:
        for G in gs:
            st, ps = Seeds(torch, G, cad, True), Seeds(torch, G, cad, False)
            for _ in range(CHECK_STEPS):
                st.step(); ps.step()
            _check_equal(torch, st, ps, f"{cad['name']}, G = {G}")
            _compare(torch, lines, f"vector step, {cad['name']}, G = {G}", [("stacked", st.step), ("per seed", ps.step)])
            _compare(torch, lines, f"collect alone, {cad['name']}, G = {G}", [("stacked", st.collect), ("per seed", ps.collect)])
            # (b): the act call alone under the library's rule and under ceil(n / 8) workgroups per group
            ctx0 = st.collectors.ctxs[0]
            cus = torch.cuda.get_device_properties(0).multi_processor_count
            rule, full = min((cad["n"] + 7) // 8, max(1, cus // G)), (cad["n"] + 7) // 8

            def act_full():
                ctx0.set_grid(full)
                st.act_only()
                ctx0.set_grid(0)
            lines.append(f"(b) workgroups per group of the grouped act launch, {cad['name']}, G = {G}")
            _compare(torch, lines, "  act call", [(f"rule ({rule} per group)", st.act_only), (f"ceil(n / 8) ({full} per group)", act_full)])
            if G == 5:
                lines.append("(c) the synchronise per vector step, stacked loop, G = 5 (same windows; 'without' = one synchronisation per window)")
                m1, t1 = _compare(torch, lines, f"  with, {cad['name']}", [("stacked", st.step)], sync_each=True)
                m0, t0 = _compare(torch, lines, f"  without, {cad['name']}", [("stacked", st.step)], sync_each=False)
                apart = max(t0[0]) < min(t1[0])
                lines.append(f"  without / with = {m0[0] / m1[0]:.2f}x; ranges {'do not overlap: without is faster' if apart else 'overlap or with is faster: the synchronise stays'}")
            st.close(); ps.close()
            del st, ps
            torch.cuda.empty_cache()


def end_to_end(lines, total_timesteps):
    from iqn_group_train_bench import _file_equal
    lines.append(f"(d) end to end: config_IQN.json (seeds 0-4) with total_timesteps = {total_timesteps} (the reference's: 3 000 000), --env-budget reference; wall time "
                 "of the whole command, one run each")
    with tempfile.TemporaryDirectory() as tmp:
        cfg = os.path.join(tmp, "config_IQN.json")
        runs = {}
        for name, extra in (("sequential", []), ("together", ["--together"]), ("stacked", ["--together", "--stack-envs"])):
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
        for other in ("together", "stacked"):
            same, checked = True, 0
            for seed in CONFIG_IQN["seed"]:
                da, db = (os.path.join(runs[n], f"seed_{seed}") for n in ("sequential", other))
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
            lines.append(f"  files of sequential and {other}, five seeds (npz array by array, network tensors as bytes, JSON without the runs' directory and start time): "
                         f"{'EQUAL' if same else 'DIFFERENT'} ({checked} arrays / tensors / files)")
            print(lines[-1], flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "iqn_group_collect_bench.txt"))
    ap.add_argument("--gs", default="1,5,16,64")
    ap.add_argument("--skip-loop", action="store_true")
    ap.add_argument("--end-to-end", action="store_true")
    ap.add_argument("--total-timesteps", type=int, default=3_000_000, help="of the end-to-end runs (the reference's: 3 000 000)")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("iqn_group_collect_bench: no GPU visible -- both forms of the collect are HIP kernels, there is nothing to measure without one")
    lines = Lines(args.out)
    lines.append("# scripts/iqn_group_collect_bench.py" + (" --end-to-end --total-timesteps %d" % args.total_timesteps if args.end_to_end else ""))
    if args.skip_loop:
        lines.append("(a)-(c) lockstep vector step, workgroups per group, synchronise: not measured in this run (run without --skip-loop)")
    else:
        lockstep(lines, tuple(int(g) for g in args.gs.split(",")))
    if args.end_to_end:
        end_to_end(lines, args.total_timesteps)
    else:
        lines.append("(d) end to end: not measured in this run (--end-to-end)")


if __name__ == "__main__":
    main()
