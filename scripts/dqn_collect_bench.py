"""What the DQN collect on the device (mn_dqn_act_rng + mn_step_append: `DQNAgent(fused_collect=True)`, train_dqn --fused-collect) and its stacked form
(mn_dqn_actor_group_act / _append, dqn/group_collect.py, train_dqn --together --stack-envs) cost or buy against the chain of launches DQN training collects
with by default.

    python scripts/dqn_collect_bench.py [--out profiles/dqn_collect_bench.txt] [--gs 1,5,16,64] [--skip-loop] [--end-to-end [--total-timesteps N] [--learner-total-timesteps N]] [--act-kernels]

Nothing is promised: both switches stay opt-in whatever comes out.

(a) the collect phase of ONE agent -- act, env step, replay append, resets -- at n = 80 / 4 096 / 65 536 rows and eps = 1 / 0.5 / 0.05: today's chain
    (mn_dqn_act, torch.rand / randint / where, mn_step, mn_replay_append, mn_reset_done) against `fused_collect` (mn_dqn_act_rng, mn_step_append,
    mn_reset_done).  The two draw from different generators, so what is compared before timing is the data path: the ring after the same actions through
    either.  And the act call alone at eps = 1, 200 back-to-back calls between two events: with the skip (no Q-value output: no row needs the network) and
    without (Q-value output: every row is evaluated), beside mn_dqn_act's greedy launch.  Where the launch is shorter than the host's call this is the host's
    time; the kernels' own durations come from a trace of `--act-kernels` (the same calls and nothing else):
        rocprofv3 --kernel-trace --stats -d DIR -- python scripts/dqn_collect_bench.py --act-kernels
(b) the lockstep vector step of G seeds, G in {1, 5, 16, 64}, at two cadences: n = 80 rows per seed with 80 gradient steps of batch 32 (the reference-budget
    cadence), and n = 4 096 with one gradient step of batch 256 (the learner-budget default); the gradient steps of every form through a LearnerGroup, one
    launch per step.  stacked: CollectorGroup.act, one mn_step, CollectorGroup.append, one mn_reset_done; per seed, fused: G x (act_batch, mn_step_append,
    mn_reset_done); per seed, chain: G x today's chain.  Also the collect phase alone, and the grouped act call alone under the library's workgroups per
    group, min(ceil(tiles / 8), max(1, CUs / G)), against ceil(tiles / 8).  Before timing, the stacked and the per-seed fused form run the same steps and
    every seed's ring, call counter and parameters are compared for equality.
(c) --end-to-end: the five-seed DQN config, whole command, one run each: sequential, `--together`, `--together --stack-envs`, with `--env-budget reference`
    and with the default learner budget (`--total-timesteps` / `--learner-total-timesteps` shorten them).
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
WINDOWS, WINDOW_S, CHECK_STEPS, EPS = 5, 0.3, 4, 0.05
CONFIG_DQN = {"agent": "DQN", "seed": [0, 1, 2, 3, 4], "total_timesteps": 3_000_000, "eval_freq": 10_000, "save_dir": "dqn_runs"}
CADENCES = (dict(name="n = 80, 80 x batch 32", n=80, batch=32, grad=80, ring=16_384), dict(name="n = 4096, 1 x batch 256", n=4096, batch=256, grad=1, ring=32_768))
DEV = "cuda:0"


def _window(torch, fn, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
        torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n


def _compare(torch, lines, name, forms):
    """`forms`: [(label, fn)] timed in alternating windows, one device synchronisation per call; one row with each form's median and range, and every other form
    over the first."""
    for _, fn in forms:
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    calls = [max(3, int(WINDOW_S / max(_window(torch, fn, 3), 1e-6))) for _, fn in forms]
    t = [[] for _ in forms]
    for _ in range(WINDOWS):
        for k, (_, fn) in enumerate(forms):
            t[k].append(_window(torch, fn, calls[k]))
    row, med = f"{name:46s}", []
    for k, (label, _) in enumerate(forms):
        us = sorted(1e6 * x for x in t[k])
        med.append(statistics.median(us))
        row += f" | {label}: {med[-1]:9.1f} us [{us[0]:.1f}-{us[-1]:.1f}], {calls[k]} calls/window"
    for k in range(1, len(forms)):
        row += f" | {forms[k][0]} / {forms[0][0]} = {med[k] / med[0]:.2f}x"
    lines.append(row)
    print(row, flush=True)
    return med


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


def _agent(seed, batch, ring, fused_collect):
    from distributional_rl_navigation_amd.dqn import DQNAgent
    return DQNAgent(device=DEV, seed=seed, batch_size=batch, buffer_size=ring, learning_starts=0, fused_train=True, fused_collect=fused_collect)


def _collect(agent, env, obs, eps):
    """One agent's collect as `TrialRun.collect` issues it; returns the next observations."""
    a = agent.act_batch(obs, eps)
    if agent.uses_fused_collect():
        env.step_append(a, obs, agent.memory)
    else:
        nxt, reward, done, _ = env.step(a)
        agent.memory.add_vector_step(obs, a, reward, nxt, done)
    return env.reset_done()


def _rings_equal(torch, x, y):
    same = x.memory.size == y.memory.size and x.memory.ptr == y.memory.ptr
    for k in ("states", "next_states", "actions", "rewards", "dones"):
        same = same and torch.equal(getattr(x.memory, k)[:x.memory.size].view(torch.int32), getattr(y.memory, k)[:y.memory.size].view(torch.int32))
    return same


# ---- (a) one agent ----------------------------------------------------------------------------------------------------------------------------------------
def collect_alone(lines):
    import torch
    from distributional_rl_navigation_amd.marinenav_env.vec_env import VecMarineNavEnv
    lines.append(f"(a) collect phase of one agent on {torch.cuda.get_device_name(0)}: medians of {WINDOWS} alternating windows of ~{WINDOW_S} s [min-max], host clock, one "
                 f"device synchronisation per vector step; chain = mn_dqn_act + torch.rand / randint / where + mn_step + mn_replay_append + mn_reset_done, fused = "
                 f"mn_dqn_act_rng + mn_step_append + mn_reset_done; before timing, the rings of both data paths after {CHECK_STEPS} steps of the same actions were "
                 "compared for equality")
    for n in (80, 4096, 65536):
        ring = max(16_384, 2 * n)
        fused, chain, actor = _agent(1, 32, ring, True), _agent(1, 32, ring, False), _agent(1, 32, ring, True)
        env_f, env_c = (VecMarineNavEnv(n, seed=7, device=DEV, precision="f64") for _ in range(2))
        obs_f, obs_c = env_f.reset(), env_c.reset()
        for _ in range(CHECK_STEPS):      # the same actions (equal seeds, equal call counters) through step_append and through step + add_vector_step
            obs_f = _collect(fused, env_f, obs_f, 0.5)
            a = actor.act_batch(obs_c, 0.5)
            nxt, reward, done, _ = env_c.step(a)
            chain.memory.add_vector_step(obs_c, a, reward, nxt, done)
            obs_c = env_c.reset_done()
        torch.cuda.synchronize()
        if not _rings_equal(torch, fused, chain):
            raise SystemExit(f"dqn_collect_bench: (a) n = {n}: the ring differs between step_append and step + add_vector_step")
        state = dict(f=obs_f, c=obs_c)
        for eps in (1.0, 0.5, 0.05):
            def run_fused():
                state["f"] = _collect(fused, env_f, state["f"], eps)

            def run_chain():
                state["c"] = _collect(chain, env_c, state["c"], eps)
            _compare(torch, lines, f"collect, n = {n}, eps = {eps}", [("fused", run_fused), ("chain", run_chain)])
        # the act launch alone at eps = 1: device time between two events
        obs, pol = state["f"], fused.policy
        forms = (("mn_dqn_act_rng, skip (no row needs the network)", lambda: pol.act_rng(obs, 1, 0, 1.0)),
                 ("mn_dqn_act_rng, no skip (Q-value output)", lambda: pol.act_rng(obs, 1, 0, 1.0, want_q=True)),
                 ("mn_dqn_act (greedy)", lambda: pol.act_batch(obs)))
        row = f"act call alone, n = {n}, eps = 1 (per call, 200 back-to-back calls between two events, median of {WINDOWS}; not below the host's time per call)"
        for label, fn in forms:
            for _ in range(20):
                fn()
            us = []
            for _ in range(WINDOWS):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(200):
                    fn()
                e1.record()
                torch.cuda.synchronize()
                us.append(e0.elapsed_time(e1) * 1e3 / 200)
            row += f" | {label}: {statistics.median(us):.2f} us [{min(us):.2f}-{max(us):.2f}]"
        lines.append(row)
        print(row, flush=True)
        env_f.close(); env_c.close()
        del fused, chain, actor
        torch.cuda.empty_cache()


def act_kernels():
    """The act calls of (a) and nothing else, for a kernel trace: per n, 200 x mn_dqn_act_rng at eps = 1 without and with the Q-value output, then at
    eps = 0.05, then 200 x mn_dqn_act."""
    import torch
    from distributional_rl_navigation_amd.dqn import DQNPolicy
    torch.manual_seed(1)
    pol = DQNPolicy(device=DEV)
    for n in (80, 4096, 65536):
        obs = torch.randn(n, 26, device=DEV)
        for fn in (lambda: pol.act_rng(obs, 1, 0, 1.0), lambda: pol.act_rng(obs, 1, 0, 1.0, want_q=True), lambda: pol.act_rng(obs, 1, 0, 0.05),
                   lambda: pol.act_batch(obs)):
            for _ in range(200):
                fn()
            torch.cuda.synchronize()
            torch.zeros(1, device=DEV).add_(1)      # (a marker kernel between the forms, so that the trace can be cut)
            torch.cuda.synchronize()


# ---- (b) G seeds in lockstep --------------------------------------------------------------------------------------------------------------------------------
class Seeds:
    """G agents with their replay rings and a LearnerGroup.  form "stacked": one env handle and a CollectorGroup; "fused" / "chain": an env per agent and the
    agent's own collect, with and without `fused_collect`."""

    def __init__(self, torch, G, cad, form):
        from distributional_rl_navigation_amd.dqn.group_collect import CollectorGroup
        from distributional_rl_navigation_amd.dqn.group_train import LearnerGroup
        from distributional_rl_navigation_amd.marinenav_env.vec_env import VecMarineNavEnv, stacked_seeds
        self.torch, self.G, self.n, self.grad, self.form = torch, G, cad["n"], cad["grad"], form
        self.agents = [_agent(100 + g, cad["batch"], cad["ring"], form != "chain") for g in range(G)]
        self.group = LearnerGroup(self.agents)
        if form == "stacked":
            self.envs = [VecMarineNavEnv(G * self.n, seeds=stacked_seeds(self.n, range(G)), device=DEV, precision="f64")]
            self.collectors = CollectorGroup(self.agents, self.envs[0])
            self.obs = self.envs[0].reset()
        else:
            self.envs = [VecMarineNavEnv(self.n, seed=g, device=DEV, precision="f64") for g in range(G)]
            self.obs = [e.reset() for e in self.envs]

    def collect(self):
        if self.form == "stacked":
            env = self.envs[0]
            actions = self.collectors.act(self.obs, EPS)
            nxt, reward, done, _ = env.step(actions)
            self.collectors.append(self.obs, actions, reward, nxt, done)
            self.obs = env.reset_done()
        else:
            for g, (ag, env) in enumerate(zip(self.agents, self.envs)):
                self.obs[g] = _collect(ag, env, self.obs[g], EPS)

    def step(self):
        self.collect()
        for _ in range(self.grad):
            self.group.train()

    def act_only(self):
        self.collectors.act(self.obs, EPS)

    def close(self):
        self.torch.cuda.synchronize()
        self.group.close()
        if self.form == "stacked":
            self.collectors.close()
        for e in self.envs:
            e.close()


def _check_equal(torch, a, b, where):
    torch.cuda.synchronize()
    for g, (x, y) in enumerate(zip(a.agents, b.agents)):
        same = _rings_equal(torch, x, y) and x.act_calls == y.act_calls
        same = same and torch.equal(x._fused.local.view(torch.int32), y._fused.local.view(torch.int32)) and bool(torch.isfinite(x._fused.local).all())
        if not same:
            raise SystemExit(f"dqn_collect_bench: {where}: seed {g} differs between the stacked and the per-seed fused form")


def lockstep(lines, gs):
    import torch
    lines.append(f"(b) lockstep vector step on {torch.cuda.get_device_name(0)}: medians of {WINDOWS} alternating windows of ~{WINDOW_S} s [min-max], host clock, one device "
                 f"synchronisation per vector step; 'call' = one vector step of all G seeds; eps = {EPS}; before timing, rings, call counters and parameters of the "
                 f"stacked and the per-seed fused form after {CHECK_STEPS} steps were compared for equality (the chain draws from torch.Generator: other actions)")
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    for cad in CADENCES:
        for G in gs:
            st, fu, ch = (Seeds(torch, G, cad, form) for form in ("stacked", "fused", "chain"))
            for _ in range(CHECK_STEPS):
                st.step(); fu.step(); ch.step()
            _check_equal(torch, st, fu, f"{cad['name']}, G = {G}")
            _compare(torch, lines, f"vector step, {cad['name']}, G = {G}", [("stacked", st.step), ("per seed, fused", fu.step), ("per seed, chain", ch.step)])
            _compare(torch, lines, f"collect alone, {cad['name']}, G = {G}", [("stacked", st.collect), ("per seed, fused", fu.collect), ("per seed, chain", ch.collect)])
            tiles = (cad["n"] + 15) // 16
            rule, full = min((tiles + 7) // 8, max(1, cus // G)), (tiles + 7) // 8

            def act_full():
                st.collectors.set_grid(full)
                st.act_only()
                st.collectors.set_grid(0)
            _compare(torch, lines, f"  grouped act call, {cad['name']}, G = {G}", [(f"rule ({rule} per group)", st.act_only), (f"ceil(tiles / 8) ({full} per group)", act_full)])
            for s in (st, fu, ch):
                s.close()
            del st, fu, ch
            torch.cuda.empty_cache()


# ---- (c) the whole command ----------------------------------------------------------------------------------------------------------------------------------
def _file_equal(fa, fb):
    import io
    import zipfile
    import numpy as np
    import torch
    if fa.endswith(".npz"):
        za, zb = np.load(fa, allow_pickle=True), np.load(fb, allow_pickle=True)
        if sorted(za.files) != sorted(zb.files):
            return False

        def eq(a, b):
            if isinstance(a, (list, tuple)) or (isinstance(a, np.ndarray) and a.dtype == object):
                return len(a) == len(b) and all(eq(x, y) for x, y in zip(a, b))
            a, b = np.asarray(a), np.asarray(b)
            return a.dtype == b.dtype and np.array_equal(a, b, equal_nan=a.dtype.kind == "f")
        return all(eq(za[k], zb[k]) for k in za.files)
    if fa.endswith(".zip"):
        sa, sb = (torch.load(io.BytesIO(zipfile.ZipFile(f).read("policy.pth")), map_location="cpu") for f in (fa, fb))
        return list(sa) == list(sb) and all(torch.equal(sa[k].contiguous().view(torch.uint8), sb[k].contiguous().view(torch.uint8)) for k in sa)
    if fa.endswith(".json"):
        ja, jb = json.load(open(fa)), json.load(open(fb))
        for j in (ja, jb):
            if isinstance(j, dict):
                j.pop("save_dir", None); j.pop("training_time", None)
        return ja == jb
    return open(fa, "rb").read() == open(fb, "rb").read()


def end_to_end(lines, budgets):
    lines.append("(c) end to end: config_DQN.json (seeds 0-4), wall time of the whole command, one run each; sequential and --together draw their exploration from "
                 "torch.Generator, --together --stack-envs from the library's generator (other actions, other files); the stacked run's files are compared with those "
                 "of `--together --fused-collect`, which is not timed here")
    with tempfile.TemporaryDirectory() as tmp:
        cfg = os.path.join(tmp, "config_DQN.json")
        for label, total, budget_args in budgets:
            lines.append(f"  {label}, total_timesteps = {total} (the reference's: 3 000 000)")
            runs = {}
            for name, extra in (("sequential", []), ("together", ["--together"]), ("stacked", ["--together", "--stack-envs"]),
                                ("(untimed) fused", ["--together", "--fused-collect"])):
                save = os.path.join(tmp, label.split()[0] + "_" + name.split()[-1])
                with open(cfg, "w") as f:
                    json.dump(dict(CONFIG_DQN, total_timesteps=total, save_dir=save), f)
                t0 = time.perf_counter()
                r = subprocess.run([sys.executable, "-m", "distributional_rl_navigation_amd.train_dqn", "-C", cfg, *budget_args, *extra], cwd=ROOT,
                                   capture_output=True, text=True)
                dt = time.perf_counter() - t0
                if r.returncode:
                    lines.append(f"    {name}: FAILED ({r.returncode}): {r.stderr[-400:]}")
                    raise SystemExit(lines[-1])
                runs[name] = os.path.join(save, os.listdir(save)[0])
                if name.startswith("("):
                    continue
                row = f"    {name:10s}: {dt:8.1f} s"
                lines.append(row)
                print(row, flush=True)
            same, checked = True, 0
            for seed in CONFIG_DQN["seed"]:
                da, db = (os.path.join(runs[n], f"seed_{seed}") for n in ("stacked", "(untimed) fused"))
                if sorted(os.listdir(da)) != sorted(os.listdir(db)):
                    same = False
                    lines.append(f"    seed {seed}: different files {sorted(os.listdir(da))} / {sorted(os.listdir(db))}")
                    continue
                for f in sorted(os.listdir(da)):
                    checked += 1
                    if not _file_equal(os.path.join(da, f), os.path.join(db, f)):
                        same = False
                        lines.append(f"    seed {seed}: {f} differs")
            lines.append(f"    files of --together --stack-envs and --together --fused-collect, five seeds (npz array by array, checkpoint tensors as bytes, JSON without "
                         f"the runs' directory and start time): {'EQUAL' if same else 'DIFFERENT'} ({checked} files)")
            print(lines[-1], flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dqn_collect_bench.txt"))
    ap.add_argument("--gs", default="1,5,16,64")
    ap.add_argument("--skip-loop", action="store_true")
    ap.add_argument("--end-to-end", action="store_true")
    ap.add_argument("--total-timesteps", type=int, default=3_000_000, help="of the end-to-end runs with --env-budget reference (the reference's: 3 000 000)")
    ap.add_argument("--learner-total-timesteps", type=int, default=3_000_000, help="of the end-to-end runs with the default learner budget")
    ap.add_argument("--act-kernels", action="store_true", help="only issue the act calls of (a), for a kernel trace; writes nothing")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("dqn_collect_bench: no GPU visible -- every form of the collect runs HIP kernels, there is nothing to measure without one")
    if args.act_kernels:
        return act_kernels()
    lines = Lines(args.out)
    lines.append("# scripts/dqn_collect_bench.py" + (f" --end-to-end --total-timesteps {args.total_timesteps} --learner-total-timesteps {args.learner_total_timesteps}"
                                                     if args.end_to_end else ""))
    if args.skip_loop:
        lines.append("(a), (b) collect phase, lockstep vector step, workgroups per group: not measured in this run (run without --skip-loop)")
    else:
        collect_alone(lines)
        lockstep(lines, tuple(int(g) for g in args.gs.split(",")))
    if args.end_to_end:
        end_to_end(lines, (("reference budget (--env-budget reference)", args.total_timesteps, ["--env-budget", "reference"]),
                           ("learner budget (the default)", args.learner_total_timesteps, [])))
    else:
        lines.append("(c) end to end: not measured in this run (--end-to-end)")


if __name__ == "__main__":
    main()
