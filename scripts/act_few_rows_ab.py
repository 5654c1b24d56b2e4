"""A / B of the few-rows act kernel (csrc/iqn_act_few.h; mn_iqn_set_few_rows_max) against the listed form it stands in for, inside ONE process: bench.py's
default loop (65 536 envs, float64 env kernels, act -> step + append -> reset -> gradient step every 4th vector step) with every reset owed to the next act
call, so that the act launch is the listed form without late rows at every list length.  Arms alternate in blocks of --block vector steps after the warm-up,
--blocks blocks each, at fixed eps = 1 - rows / envs for --rows list lengths.  Arms: `listed` = threshold -1 (never: the reference arm), `few` = threshold
2^31 - 1 (always).  Prints every block, the medians, the spread of the reference arm's blocks (the noise a difference has to beat), the launches each arm
really made and the mean time of an act call's launches (preparation + act, from the context's profiling events).

    python scripts/act_few_rows_ab.py [--envs 65536] [--block 200] [--blocks 5] [--rows 20,100,500,2000,8000]"""
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
    ap.add_argument("--rows", default="20,100,500,2000,8000")
    args = ap.parse_args()

    import torch
    from distributional_rl_navigation_amd.iqn.agent import IQNAgent
    from distributional_rl_navigation_amd.iqn.fused_act import act_context
    from distributional_rl_navigation_amd.marinenav_env.vec_env import VecMarineNavEnv

    device = torch.device("cuda:0")
    n = args.envs
    env = VecMarineNavEnv(n, seed=0, device=device, precision="f64")
    env.set_attrs(num_cores=8, num_obs=10, min_start_goal_dis=40.0)
    obs = env.reset()
    agent = IQNAgent(26, 9, BATCH_SIZE=256, BUFFER_SIZE=100_000, device=device, seed=100, learning_starts=0, UPDATE_EVERY=4)
    agent.reset_under_act = True
    env.set_reset_owed_max_rows(2 ** 31 - 1)
    ctx = act_context(agent.qnetwork_local)
    arms = {"listed": -1, "few": ctx.FEW_ROWS_ALWAYS}

    def run(k, o, eps):
        for _ in range(k):
            o, _, _, _, _ = agent.vec_step(env, o, eps, 1.0, per_iter=n)
        return o

    obs = run(args.warmup, obs, 1.0 - 20.0 / n)
    print(f"envs {n}, blocks of {args.block} vector steps, every reset owed to the next act call", flush=True)
    for rows in [int(r) for r in args.rows.split(",")]:
        eps = 1.0 - rows / n
        ms, act_ms, launches = {k: [] for k in arms}, {k: [] for k in arms}, {k: 0 for k in arms}
        for k, v in arms.items():      # both kernels warm at this eps before anything is timed
            ctx.set_few_rows_max(v)
            obs = run(args.warmup, obs, eps)
        for b in range(2 * args.blocks):
            k = "few" if b & 1 else "listed"
            ctx.set_few_rows_max(arms[k])
            before = ctx.few_rows_launches()
            ctx.profile_begin(args.block)
            torch.cuda.synchronize(device)
            t0 = time.perf_counter()
            obs = run(args.block, obs, eps)
            torch.cuda.synchronize(device)
            ms[k].append(1e3 * (time.perf_counter() - t0) / args.block)
            act_ms[k].append(ctx.profile_end()[0])
            launches[k] += ctx.few_rows_launches() - before
        lst, few = ms["listed"], ms["few"]
        print(f"~{rows} listed rows (eps {eps:.6f}); few-rows launches: listed arm {launches['listed']}, few arm {launches['few']} of {args.block * args.blocks}", flush=True)
        print("  listed ms/step: " + " ".join(f"{x:.4f}" for x in lst) + f"   median {statistics.median(lst):.4f}  spread {max(lst) - min(lst):.4f}")
        print("  few    ms/step: " + " ".join(f"{x:.4f}" for x in few) + f"   median {statistics.median(few):.4f}  spread {max(few) - min(few):.4f}")
        print(f"  few / listed {statistics.median(few) / statistics.median(lst):.3f}   difference {statistics.median(lst) - statistics.median(few):+.4f} ms")
        print(f"  act call's launches (events), mean ms: listed {statistics.median(act_ms['listed']):.4f}  few {statistics.median(act_ms['few']):.4f}", flush=True)
    ctx.set_few_rows_max(None)
    env.join_reset()
    env.close()


if __name__ == "__main__":
    main()
