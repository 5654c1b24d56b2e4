"""A / B of the act launch that evaluates only the rows that do not explore (IQNAgent.act_greedy_rows_only) inside ONE process: bench.py's default loop
(65 536 envs, act -> step + append -> reset under the next act -> gradient step every 4th vector step), switch off / on alternating in blocks of
--block vector steps after the warm-up, --blocks blocks each, at the reference schedule's eps (~1 at the start of a run), then 0.5, then 0.05.
Prints every block, the medians and the spread of the off-blocks (the run-to-run noise a difference has to beat).

    python scripts/act_greedy_rows_ab.py [--envs 65536] [--block 200] [--blocks 5]"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--block", type=int, default=200)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=20)
    args = ap.parse_args()

    import torch
    from distributional_rl_navigation_amd.iqn.agent import IQNAgent, UnderActGuard
    from distributional_rl_navigation_amd.iqn.fused_act import late_timeouts
    from distributional_rl_navigation_amd.marinenav_env.vec_env import VecMarineNavEnv

    device = torch.device("cuda:0")
    n = args.envs
    env = VecMarineNavEnv(n, seed=0, device=device, precision="f64")
    env.set_attrs(num_cores=8, num_obs=10, min_start_goal_dis=40.0)
    obs = env.reset()
    agent = IQNAgent(26, 9, BATCH_SIZE=256, BUFFER_SIZE=100_000, device=device, seed=100, learning_starts=0, UPDATE_EVERY=4)
    agent.reset_under_act = True
    total_timesteps = 3_000_000 * n

    def run(k, o, eps):
        for _ in range(k):
            e = agent.linear_eps(total_timesteps) if eps is None else eps
            o, _, _, _, _ = agent.vec_step(env, o, e, 1.0, per_iter=n)
        return o

    obs = run(args.warmup, obs, None)
    guard = UnderActGuard(agent, env, preflight=12, poll_every=0)      # as bench.py: make sure the reset launch runs beside the act kernel on this box
    for i in range(12):
        obs = run(1, obs, None)
        guard.after_step(i)
    guard.close()
    print(f"envs {n}, blocks of {args.block} vector steps, resets {'in front of' if guard.fallback is not None else 'under'} the act kernel", flush=True)

    for eps in (None, 0.5, 0.05):
        ms = {False: [], True: []}
        eps0 = agent.linear_eps(total_timesteps)
        for on in (False, True):      # every form warm at this eps before anything is timed
            agent.act_greedy_rows_only = on
            obs = run(args.warmup, obs, eps)
        for b in range(2 * args.blocks):
            on = bool(b & 1)
            agent.act_greedy_rows_only = on
            torch.cuda.synchronize(device)
            t0 = time.perf_counter()
            obs = run(args.block, obs, eps)
            torch.cuda.synchronize(device)
            ms[on].append(1e3 * (time.perf_counter() - t0) / args.block)
        off, onn = ms[False], ms[True]
        name = f"schedule ({eps0:.4f} -> {agent.linear_eps(total_timesteps):.4f} over these blocks)" if eps is None else f"{eps}"
        print(f"eps {name}", flush=True)
        print("  off ms/step: " + " ".join(f"{x:.4f}" for x in off) + f"   median {statistics.median(off):.4f}  spread {max(off) - min(off):.4f}")
        print("  on  ms/step: " + " ".join(f"{x:.4f}" for x in onn) + f"   median {statistics.median(onn):.4f}  spread {max(onn) - min(onn):.4f}")
        print(f"  on / off {statistics.median(onn) / statistics.median(off):.3f}   difference {statistics.median(off) - statistics.median(onn):+.4f} ms", flush=True)
    env.join_reset()
    print(f"late-row time-outs {late_timeouts(agent.qnetwork_local)}")
    env.close()


if __name__ == "__main__":
    main()
