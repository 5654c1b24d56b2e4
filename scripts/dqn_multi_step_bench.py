"""How much the multi-step DQN gradient call (mn_dqn_train_steps) buys over the loop of single launches (mn_dqn_train_step), at batch 32.

    python scripts/dqn_multi_step_bench.py [--out profiles/dqn_multi_step_bench.txt] [--end-to-end [--total-timesteps N]]

(a) loop against call: per-step time of `K x agent.train()` and of `agent.train_many(K)` for K = 20, 80, 320 on a ring filled from a real rollout;
    both forms in one process, alternating, medians of 5 after a warm-up, with min-max ranges; the end states must be equal.
(b) shares: the TD-target launch and the chain, each timed alone (K = 80).
(c) --end-to-end: one `train_dqn --env-budget reference` run with `--train-steps-per-call multi` and one with `1`, wall time each.
The kernels' registers, LDS and scratch (the compiler's resource remarks) go into the same file.
"""
import argparse
import json
import os
import re
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
KS = (20, 80, 320)
REPS, BATCH = 5, 32


def resource_remarks():
    hipcc = "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        return ["(no hipcc here: resource remarks not collected)"]
    csrc = os.path.join(ROOT, "distributional_rl_navigation_amd", "csrc")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-I../../include", "-I.", "-ffp-contract=off", "--cuda-device-only",
                        "-Rpass-analysis=kernel-resource-usage", "-c", "-o", os.devnull, "dqn_train.hip"], cwd=csrc, capture_output=True, text=True)
    out, cur = [], None
    for line in r.stderr.splitlines():
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            cur = re.sub(r"^_ZN\d+_GLOBAL__N_1\d+|ENS_.*$", "", m.group(1))
            continue
        m = re.search(r"remark:\s+(VGPRs|AGPRs|TotalSGPRs|ScratchSize \[bytes/lane\]|LDS Size \[bytes/block\]|Occupancy \[waves/SIMD\]): (\d+)", line)
        if m and cur:
            out.append(f"  {cur:28s} {m.group(1):26s} {m.group(2)}")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dqn_multi_step_bench.txt"))
    ap.add_argument("--end-to-end", action="store_true")
    ap.add_argument("--total-timesteps", type=int, default=3_000_000, help="of the end-to-end runs (the reference's: 3 000 000)")
    args = ap.parse_args()
    import torch
    from distributional_rl_navigation_amd.dqn import DQNAgent
    from distributional_rl_navigation_amd.marinenav_env.vec_env import VecMarineNavEnv
    dev = "cuda:0"
    lines = [f"# scripts/dqn_multi_step_bench.py on {torch.cuda.get_device_name(0)}; batch {BATCH}, medians of {REPS} alternating repetitions after a warm-up, us per gradient step"]

    ag = DQNAgent(device=dev, buffer_size=16_384, batch_size=BATCH, seed=3, fused_train=True)
    env = VecMarineNavEnv(1024, seed=5, device=dev)
    obs = env.reset()
    for _ in range(16):
        a = ag.act_batch(obs, 1.0)
        nxt, r, d, _ = env.step(a)
        ag.memory.add_vector_step(obs, a, r, nxt, d)
        obs = env.reset_done()
    env.close()
    ft = ag._fused_trainer()
    ag.train()
    tensors = (ft.local, ft.target, ft.exp_avg, ft.exp_avg_sq, ft.step_dev, ft.rng_state)
    saved = [t.clone() for t in tensors]

    def restore():
        for d_, s_ in zip(tensors, saved):
            d_.copy_(s_)

    def timed(fn):
        restore()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    def loop(K):
        for _ in range(K):
            ag.train()

    auto = None
    lines.append("(a) loop of single launches (K x agent.train()) against one call (agent.train_many(K))")
    lines.append(f"  {'K':>4s} {'loop med':>9s} {'loop min-max':>16s} {'call med':>9s} {'call min-max':>16s} {'loop/call':>9s}")
    for K in KS:
        timed(lambda: loop(K)); timed(lambda: ag.train_many(K))      # warm-up: buffers, code objects
        tl, tc = [], []
        for _ in range(REPS):
            tl.append(timed(lambda: loop(K)) / K * 1e6)
            end_loop = [t.clone() for t in tensors]
            tc.append(timed(lambda: ag.train_many(K)) / K * 1e6)
            assert all(torch.equal(x, y) for x, y in zip(tensors, end_loop)), "end states differ"
        ml, mc = statistics.median(tl), statistics.median(tc)
        lines.append(f"  {K:4d} {ml:9.1f} {min(tl):7.1f}-{max(tl):<8.1f} {mc:9.1f} {min(tc):7.1f}-{max(tc):<8.1f} {ml / mc:9.2f}")
        if K == 80:
            auto = mc < ml and max(tc) < min(tl)
    lines.append("  end states (parameters, moments, step and draw counters) equal after every pair")
    lines.append(f"  rule for --train-steps-per-call auto -> {'the multi-step call' if auto else 'the loop'}: at K = 80 the call's median is {'below' if auto else 'not clearly below'} the loop's"
                 f"{' and the ranges do not overlap' if auto else ''}")

    lines.append("(b) shares at K = 80: each launch of the call alone (device time between two events, median of 5)")
    ring = (ag.memory.states, ag.memory.actions, ag.memory.rewards, ag.memory.next_states, ag.memory.dones)
    for name, parts in (("TD targets of all steps", 1), ("chain (one workgroup)", 2), ("both", 3)):
        ts = []
        for rep in range(REPS + 1):
            restore()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            ft.steps(ring, ag.memory.size, BATCH, 80, parts=parts)
            e1.record()
            torch.cuda.synchronize()
            if rep:
                ts.append(e0.elapsed_time(e1) * 1e3)
        lines.append(f"  {name:26s} {statistics.median(ts):9.1f} us per call = {statistics.median(ts) / 80:6.2f} us per step  ({min(ts):.1f}-{max(ts):.1f})")
    restore()

    lines.append("kernel resources (compiler remarks, gfx950)")
    lines += resource_remarks()

    if args.end_to_end:
        lines.append(f"(c) train_dqn --env-budget reference, total_timesteps {args.total_timesteps}, one seed, wall time of the whole run")
        for mode in ("multi", "1"):
            with tempfile.TemporaryDirectory() as tmp:
                cfg = os.path.join(tmp, "config_DQN.json")
                with open(cfg, "w") as f:
                    json.dump({"agent": "DQN", "seed": [0], "total_timesteps": args.total_timesteps, "eval_freq": 10_000, "save_dir": os.path.join(tmp, "runs")}, f)
                t0 = time.perf_counter()
                r = subprocess.run([sys.executable, "-m", "distributional_rl_navigation_amd.train_dqn", "-C", cfg, "--env-budget", "reference",
                                    "--train-steps-per-call", mode], cwd=ROOT, capture_output=True, text=True)
                dt = time.perf_counter() - t0
                lines.append(f"  --train-steps-per-call {mode:5s} {dt:8.1f} s" + ("" if r.returncode == 0 else f"  FAILED ({r.returncode}): {r.stderr[-300:]}"))
    else:
        lines.append("(c) end to end: not measured in this run (--end-to-end)")
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
