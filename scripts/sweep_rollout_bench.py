"""Times the DQN evaluation and the experiment sweep on one GPU: the per-step loop against whole episodes in one launch each.

  (a) train_dqn.evaluate on the 30 evaluation worlds (tests/golden/eval_config_seed3.json) with the shipped DQN weights;
  (b) the same with a seeded untrained network (episodes run to the 1 000-step limit);
  (c) run_experiment(agent, 8, 6, num=500, policies=ALL_POLICIES, dqn=pol) with the shipped IQN checkpoint: all eight policies, and the IQN group
      and the DQN rows on their own;
  (d) the same sweep with capture=True (every episode's `ep_data`: sub-step trajectory, IQN quantile values and taus): two figures per side -- "traces",
      run_experiment's timings["traces_s"], the time until all traces are complete on the device, and the wall time end to end incl. the host-side
      `ep_data` assembly, which is the same code on both sides.  --capture-only runs (d) alone; --out FILE also writes the table to FILE.

Every case runs with the loop and with the launches (one_launch=True), both warmed up once and then timed alternately (median, minimum and
maximum of --reps wall times each), and both forms are checked to return the same results.  The clock the GPU holds under matrix load
(mn_probe_mfma_clock) is printed before and after.

    python scripts/sweep_rollout_bench.py [--reps 5] [--num 500] [--capture-only] [--out FILE]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
G = os.path.join(ROOT, "tests", "golden")
RECORD_KEYS = ("success", "out_of_area", "time", "energy", "reward", "actions")


def _clock():
    import torch
    from distributional_rl_navigation_amd import _capi
    out = (C.c_double * 5)()
    rc = _capi.lib().mn_probe_mfma_clock(C.c_double(50.0), out, C.c_void_p(torch.cuda.current_stream().cuda_stream))
    return float("nan") if rc else out[1]


def _time_pair(loop_fn, launch_fn, reps):
    """Both forms warmed up once (weight images, first launches), then timed alternately, `reps` times each: a drift of the box hits both alike.
    Returns ((median s, min s, max s, last result) of the loop, the same of the launches)."""
    import torch
    fns = (loop_fn, launch_fn)
    ts, res = ([], []), [fn() for fn in fns]
    for _ in range(reps):
        for i, fn in enumerate(fns):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res[i] = fn()
            torch.cuda.synchronize()
            ts[i].append(time.perf_counter() - t0)
    return tuple((sorted(t)[len(t) // 2], min(t), max(t), r) for t, r in zip(ts, res))


class _Agent:      # what train_dqn.evaluate reads of a DQNAgent
    def __init__(self, policy):
        self.policy, self.device = policy, policy.device


_OUT = []


def _say(line):
    print(line, flush=True)
    _OUT.append(line)


def _row(name, steps, loop, one, same):
    ms = lambda t: f"{t[0] * 1e3:.1f} [{t[1] * 1e3:.1f} .. {t[2] * 1e3:.1f}]"
    _say(f"{name:<48}{steps:>7}{ms(loop):>32}{ms(one):>28}{loop[0] / one[0]:>9.2f}x  {same}")


def _stats(t):
    return sorted(t)[len(t) // 2], min(t), max(t)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--num", type=int, default=500)
    ap.add_argument("--capture-only", action="store_true")
    ap.add_argument("--out", metavar="FILE")
    args = ap.parse_args()
    import numpy as np
    import torch
    from distributional_rl_navigation_amd.dqn import DQNPolicy
    from distributional_rl_navigation_amd.experiments import ALL_POLICIES, run_experiment
    from distributional_rl_navigation_amd.iqn.agent import IQNAgent
    from distributional_rl_navigation_amd.marinenav_env.vec_env import VecMarineNavEnv
    from distributional_rl_navigation_amd.train_dqn import evaluate
    with open(os.path.join(G, "eval_config_seed3.json")) as f:
        cfg = json.load(f)
    _say(f"device: {torch.cuda.get_device_name(0)}; {args.reps} runs of each form, alternating, after one warm-up run each (wall time, synchronised)")
    _say(f"clock under MFMA load before: {_clock():.3f} GHz")
    _say(f"{'case':<48}{'steps':>7}{'loop ms: median [min .. max]':>32}{'launches ms':>28}{'speed-up':>10}  same")

    def shipped():
        return DQNPolicy.load(os.path.join(G, "pretrained_DQN_seed3", "q_net.npz"), device="cuda:0")

    def untrained():
        torch.manual_seed(7)
        return DQNPolicy(device="cuda:0")
    def agent():
        a = IQNAgent(26, 9, device="cuda:0", seed=2, BUFFER_SIZE=1024)
        a.load_model(os.path.join(G, "pretrained_IQN_seed3"), "cuda:0")
        return a

    def evaluate_cases():
        for name, make in (("(a) evaluate, 30 worlds, shipped DQN", shipped), ("(b) evaluate, 30 worlds, untrained DQN (seed 7)", untrained)):
            ags = [_Agent(make()), _Agent(make())]
            envs = [VecMarineNavEnv(len(cfg), device="cuda:0", precision="f64") for _ in range(2)]
            loop, one = _time_pair(lambda: evaluate(ags[0], envs[0], cfg), lambda: evaluate(ags[1], envs[1], cfg, one_launch=True), args.reps)
            for env in envs:
                env.close()
            rl, ro = loop[3], one[3]
            same = rl["actions"] == ro["actions"] and all(np.array_equal(rl[k], ro[k]) for k in ("rewards", "successes", "times", "energies"))
            _row(name, max(len(a) for a in ro["actions"]), loop, one, same)

    def sweep_cases():
        iqn = tuple(p for p in ALL_POLICIES if "IQN" in p)
        for name, pols in ((f"(c) sweep, {args.num} worlds x 8 policies, total", ALL_POLICIES), (f"(c) IQN group only ({len(iqn)} x {args.num} rows)", iqn),
                           (f"(c) DQN only ({args.num} rows)", ("DQN",))):
            # a fresh, identically seeded agent per run: every run draws the same taus, so loop and launches can be compared
            run = lambda one: run_experiment(agent() if pols != ("DQN",) else None, 8, 6, num=args.num, policies=pols, dqn=shipped(), one_launch=one)[0]
            loop, one = _time_pair(lambda: run(False), lambda: run(True), args.reps)
            rl, ro = loop[3], one[3]
            same = all(rl[p][k] == ro[p][k] for p in pols for k in RECORD_KEYS)
            _row(name, max(len(a) for p in pols for a in ro[p]["actions"]), loop, one, same)
    if not args.capture_only:
        evaluate_cases()
        sweep_cases()
    # (d) the captured sweep: per run the time until the traces are complete on the device (timings["traces_s"]) and the wall time end to end
    traces = ([], [])

    def captured(one, k):
        tm = {}
        res = run_experiment(agent(), 8, 6, num=args.num, policies=ALL_POLICIES, dqn=shipped(), capture=True, one_launch=one, timings=tm)[0]
        traces[k].append(tm["traces_s"])
        print(f"  (d) {'launches' if one else 'loop'} run {len(traces[k]) - 1}: traces on device {tm['traces_s']:.2f} s", file=sys.stderr, flush=True)
        return res
    loop, one = _time_pair(lambda: captured(False, 0), lambda: captured(True, 1), args.reps)
    rl, ro = loop[3], one[3]
    same = all(rl[p][k] == ro[p][k] for p in ALL_POLICIES for k in RECORD_KEYS + ("ep_data",))
    steps = max(len(a) for p in ALL_POLICIES for a in ro[p]["actions"])
    tl, to = _stats(traces[0][1:]), _stats(traces[1][1:])      # (the first entry of each is the warm-up run's)
    _row(f"(d) captured sweep, {args.num} x 8: traces on device", steps, tl, to, same)
    _row(f"(d) captured sweep, {args.num} x 8: end to end", steps, loop, one, same)
    _say(f"clock under MFMA load after: {_clock():.3f} GHz")
    _say("(c), (d) end to end include what both forms share: generating the worlds (one reset + read-back per world), loading them, building the agent, the result lists")
    _say("-- in (d) also the host-side `ep_data` assembly (one function for both forms); (d) traces on device = run_experiment's timings[\"traces_s\"].")
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(_OUT) + "\n")


if __name__ == "__main__":
    main()
