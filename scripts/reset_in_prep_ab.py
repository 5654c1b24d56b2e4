"""A / B of the rule that leaves a vector step's episode resets to the next act call's preparation launch (mn_reset_done_next_act: MN_RESET_OWED; the launch is
csrc/mn_prep_reset.hip) inside ONE process: bench.py's default loop (65 536 envs, float64 env kernels, act -> step + append -> reset -> gradient step every
4th vector step), arms alternating in blocks of --block vector steps after the warm-up, --blocks blocks each, at the reference schedule's eps (~1 at the start
of a run), then 0.95, 0.8, 0.5 and 0.05.  Arms: `under` = the rule off (resets under the act kernel: the reference arm), `owed` = every reset owed.
Prints every block, the medians, the spread of the reference arm's blocks (the noise a difference has to beat) and the rows an act launch evaluates.

    python scripts/reset_in_prep_ab.py [--envs 65536] [--block 200] [--blocks 5]"""
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
    arms = {"under": -1, "owed": 2 ** 31 - 1}

    def run(k, o, eps):
        for _ in range(k):
            e = agent.linear_eps(total_timesteps) if eps is None else eps
            o, _, _, _, _ = agent.vec_step(env, o, e, 1.0, per_iter=n)
        return o

    env.set_reset_owed_max_rows(-1)
    obs = run(args.warmup, obs, None)
    guard = UnderActGuard(agent, env, preflight=12, poll_every=0)      # as bench.py: make sure the reset launch runs beside the act kernel on this box
    for i in range(12):
        obs = run(1, obs, None)
        guard.after_step(i)
    guard.close()
    print(f"envs {n}, blocks of {args.block} vector steps, reference arm: resets {'in front of' if guard.fallback is not None else 'under'} the act kernel", flush=True)

    for eps in (None, 0.95, 0.8, 0.5, 0.05):
        ms = {k: [] for k in arms}
        eps0 = agent.linear_eps(total_timesteps)
        for k, v in arms.items():      # every form warm at this eps before anything is timed
            env.set_reset_owed_max_rows(v)
            obs = run(args.warmup, obs, eps)
        owed0, launches0 = env.resets_owed, list(env.reset_launches)
        for b in range(2 * args.blocks):
            k = "owed" if b & 1 else "under"
            env.set_reset_owed_max_rows(arms[k])
            torch.cuda.synchronize(device)
            t0 = time.perf_counter()
            obs = run(args.block, obs, eps)
            torch.cuda.synchronize(device)
            ms[k].append(1e3 * (time.perf_counter() - t0) / args.block)
        und, owe = ms["under"], ms["owed"]
        e1 = agent.linear_eps(total_timesteps) if eps is None else eps
        name = f"schedule ({eps0:.4f} -> {e1:.4f} over these blocks)" if eps is None else f"{eps}"
        print(f"eps {name}: an act launch evaluates ~{(1.0 - e1) * n:.0f} rows; resets owed {env.resets_owed - owed0} of "
              f"{sum(env.reset_launches) - sum(launches0)} (under the act kernel {env.reset_launches[1] - launches0[1]})", flush=True)
        print("  under ms/step: " + " ".join(f"{x:.4f}" for x in und) + f"   median {statistics.median(und):.4f}  spread {max(und) - min(und):.4f}")
        print("  owed  ms/step: " + " ".join(f"{x:.4f}" for x in owe) + f"   median {statistics.median(owe):.4f}  spread {max(owe) - min(owe):.4f}")
        print(f"  owed / under {statistics.median(owe) / statistics.median(und):.3f}   difference {statistics.median(und) - statistics.median(owe):+.4f} ms", flush=True)
    env.join_reset()
    print(f"late-row time-outs {late_timeouts(agent.qnetwork_local)}")
    env.close()


if __name__ == "__main__":
    main()
