"""One world's flow field and a policy's map over it, as one .npz (no plotting).

    python scripts/policy_map.py --iqn tests/golden/pretrained_IQN_seed3 --eval-config tests/golden/eval_config_seed3.json --world 0 --out map.npz
    python scripts/policy_map.py --planner APF --seed 7 --nx 64 --ny 64 --thetas 8 --out apf.npz
    python scripts/policy_map.py --dqn tests/golden/pretrained_DQN_seed3/q_net.npz --eval-config tests/golden/eval_config_seed3.json --lookahead --out look.npz
    python scripts/policy_map.py --bench      # time the queries against the step kernel -> profiles/query_bench.txt, profiles/query_step_bench.txt

The world is entry `--world i` of an eval_config.json, or the one `--seed` generates.  The policy is an IQN checkpoint directory (`--iqn`, with
`--cvar` or `--adaptive`), a DQN checkpoint (`--dqn`: an sb3 .zip, a policy.pth or the .npz of the q_net tensors) or a classical planner.
The .npz holds: xs, ys, thetas, speed; flow_xs, flow_ys, flow_v [flow_n][flow_n][2] (the grid of env_visualizer.plot_graph); the policy's maps
([thetas][ys][xs]...: action, and for IQN cvar, q, with --quantiles quantiles and taus) and flags; the world (cores, obstacles, start, goal).

--lookahead (IQN / DQN: a policy with Q-values) adds maps.lookahead_map's arrays: backup, residual, lookahead_action, reward_next, done_next, info_next
(the one-step Bellman backup of every action through the what-if step, VecMarineNavEnv.step_at).

--bench: medians of 5 timed windows of 20 calls after a warm-up window, the three cases alternating in one process: the observation query for 65 536 and for 1 048 576 poses of one
world (float32 rows and flags out), and mn_step on 65 536 float64 envs that all hold that same world.  The yardstick is the step kernel: a query does
one field evaluation and one sonar scan where a step does N = 10 field evaluations plus the scan.  A second part, written to
profiles/query_step_bench.txt, times the what-if step in the same way -- step_at for 65 536 and 1 048 576 poses x 9 actions of that world against mn_step on
the 65 536 envs -- and the 36-episode replay of tests/golden/g6_pretrained_replay.npz as one rollout_at against a loop of one mn_step per step.  No speed
is claimed for it: one lane per query in literal float64 is expected to be slower per step than mn_step.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
G = os.path.join(ROOT, "tests", "golden")


def _world(args, VecMarineNavEnv):
    """A one-env handle holding the requested world."""
    env = VecMarineNavEnv(1, seed=args.seed, device=args.device, precision="f64")
    if args.eval_config:
        with open(args.eval_config) as f:
            cfg = json.load(f)
        env.load_worlds([VecMarineNavEnv.world_from_eval_config(cfg[f"env_{args.world}"])])
    else:
        env.set_attrs(num_cores=args.cores, num_obs=args.obstacles)
        env.reset()
    return env


def _bench(args):
    import numpy as np
    import torch
    from distributional_rl_navigation_amd.marinenav_env.vec_env import VecMarineNavEnv
    with open(os.path.join(G, "eval_config_seed3.json")) as f:
        world = VecMarineNavEnv.world_from_eval_config(json.load(f)[f"env_{args.world}"])
    n_step = 65536
    env = VecMarineNavEnv(n_step, device=args.device, precision="f64")
    env.load_worlds([world], repeat=n_step)
    rng = np.random.RandomState(0)
    w, h = float(env.params.width), float(env.params.height)

    def poses(q):
        return torch.from_numpy(np.stack([rng.uniform(0, w, q), rng.uniform(0, h, q), rng.uniform(0, 2 * np.pi, q), rng.uniform(0, 2, q)], axis=1)).to(env.device)

    small, large = poses(65536), poses(1 << 20)
    # the envs step from spread-out poses too (all at the start pose, every lane would scan the same obstacles)
    st = np.zeros((n_step, 6)); st[:, :4] = small.cpu().numpy()
    env.set_state(st, np.zeros(n_step, np.int32))
    actions = torch.from_numpy(rng.randint(9, size=n_step).astype(np.int32)).to(env.device)
    cases = (("observation_at, 65 536 poses", lambda: env.observation_at(small, env=0, return_flags=True), 65536),
             ("observation_at, 1 048 576 poses", lambda: env.observation_at(large, env=0, return_flags=True), 1 << 20),
             ("mn_step, 65 536 f64 envs", lambda: env.step(actions), n_step))
    times = [[] for _ in cases]
    for rep in range(args.reps + 1):      # the first round warms up
        for i, (_, fn, _) in enumerate(cases):
            env.set_state(st)      # every timed window of steps starts from the same poses
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.inner):      # a window of several launches: one launch alone is a fraction of a millisecond
                fn()
            torch.cuda.synchronize()
            if rep:
                times[i].append((time.perf_counter() - t0) / args.inner)
    lines = [f"device: {torch.cuda.get_device_name(0)}; world {args.world} of tests/golden/eval_config_seed3.json "
             f"({len(world['cores'])} cores, {len(world['obstacles'])} obstacles); medians of {args.reps} windows of {args.inner} calls after a warm-up window, the cases alternating; wall time per call, synchronised",
             f"{'case':<36}{'median ms':>12}{'min':>9}{'max':>9}{'ns per pose / env':>20}"]
    for (name, _, count), t in zip(cases, times):
        med = sorted(t)[len(t) // 2]
        lines.append(f"{name:<36}{med * 1e3:>12.3f}{min(t) * 1e3:>9.3f}{max(t) * 1e3:>9.3f}{med / count * 1e9:>20.2f}")
    text = "\n".join(lines)
    print(text, flush=True)
    out = args.out or os.path.join(ROOT, "profiles", "query_bench.txt")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write(text + "\n")
    _bench_step(args, env, st, small, large, actions, os.path.join(os.path.dirname(os.path.abspath(out)), "query_step_bench.txt"))
    env.close()


def _bench_step(args, env, st, small, large, actions, out):
    """The what-if step against mn_step on the same handle, alternating, and the G6 replay as one rollout_at against the per-step loop."""
    import numpy as np
    import torch
    from distributional_rl_navigation_amd.marinenav_env.vec_env import VecMarineNavEnv
    n_step = env.n_envs
    fan = lambda p: (p.repeat_interleave(9, dim=0), torch.arange(9, dtype=torch.int32, device=p.device).repeat(p.shape[0]))
    s9, a9 = fan(small)
    l9, al9 = fan(large)
    cases = (("step_at, 65 536 poses x 9 actions", lambda: env.step_at(s9, a9, env=0), 65536 * 9),
             ("step_at, 1 048 576 poses x 9 actions", lambda: env.step_at(l9, al9, env=0), (1 << 20) * 9),
             ("mn_step, 65 536 f64 envs", lambda: env.step(actions), n_step))
    times = [[] for _ in cases]
    for rep in range(args.reps + 1):
        for i, (_, fn, _) in enumerate(cases):
            env.set_state(st)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.inner):
                fn()
            torch.cuda.synchronize()
            if rep:
                times[i].append((time.perf_counter() - t0) / args.inner)
    lines = [f"device: {torch.cuda.get_device_name(0)}; medians of {args.reps} windows of {args.inner} calls after a warm-up window, the cases alternating; wall time per call, synchronised",
             f"{'case':<40}{'median ms':>12}{'min':>9}{'max':>9}{'ns per step':>16}"]
    for (name, _, count), t in zip(cases, times):
        med = sorted(t)[len(t) // 2]
        lines.append(f"{name:<40}{med * 1e3:>12.3f}{min(t) * 1e3:>9.3f}{max(t) * 1e3:>9.3f}{med / count * 1e9:>16.2f}")
    # the G6 replay: 36 stored episodes, one rollout_at against one mn_step per step on a handle that holds their worlds
    with open(os.path.join(G, "eval_config_seed3.json")) as f:
        cfg = json.load(f)
    z = np.load(os.path.join(G, "g6_pretrained_replay.npz"))
    ids = np.concatenate([z["greedy_ids"], z["adaptive_ids"]]); length = np.concatenate([z["greedy_len"], z["adaptive_len"]])
    acts = np.concatenate([z["greedy_actions"], z["adaptive_actions"]])
    worlds = [VecMarineNavEnv.world_from_eval_config(cfg[f"env_{k}"]) for _, k in ids]
    g6 = VecMarineNavEnv(len(worlds), device=args.device, precision="f64")
    g6.load_worlds(worlds)
    start = np.array([[w["start"][0], w["start"][1], w["init_theta"], w["init_speed"]] for w in worlds])
    H = int(length.max())
    a_dev = torch.from_numpy(np.where(acts[:, :H] >= 0, acts[:, :H], 0).astype(np.int32)).to(g6.device)
    a_steps = a_dev.t().contiguous()
    idx = torch.arange(len(worlds), dtype=torch.int32, device=g6.device)

    def loop():
        g6.load_worlds(worlds)
        for t in range(H):
            g6.step(a_steps[t])
    replay = (("G6 replay, one rollout_at (36 episodes)", lambda: g6.rollout_at(start, a_dev, lengths=length, env=idx, trace=("reward", "done", "info", "action"))),
              ("G6 replay, one mn_step per step", loop))
    rt = [[] for _ in replay]
    for rep in range(args.reps + 1):
        for i, (_, fn) in enumerate(replay):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if rep:
                rt[i].append(time.perf_counter() - t0)
    lines.append(f"G6: {len(worlds)} episodes, {int(length.sum())} steps in all, the longest {H}; medians of {args.reps} runs after a warm-up run, alternating")
    for (name, _), t in zip(replay, rt):
        lines.append(f"{name:<40}{sorted(t)[len(t) // 2] * 1e3:>12.3f}{min(t) * 1e3:>9.3f}{max(t) * 1e3:>9.3f}")
    g6.close()
    text = "\n".join(lines)
    print(text, flush=True)
    with open(out, "w") as f:
        f.write(text + "\n")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    pol = ap.add_mutually_exclusive_group()
    pol.add_argument("--iqn", metavar="DIR", help="IQN checkpoint directory (network_params.pth, constructor_params.json)")
    pol.add_argument("--dqn", metavar="FILE", help="DQN checkpoint (.zip / policy.pth / q_net .npz)")
    pol.add_argument("--planner", choices=("APF", "BA"))
    ap.add_argument("--cvar", type=float, default=1.0)
    ap.add_argument("--adaptive", action="store_true")
    ap.add_argument("--quantiles", action="store_true", help="IQN: also store the 32 x 9 quantile samples and the taus of every pose")
    ap.add_argument("--eval-config", metavar="JSON")
    ap.add_argument("--world", type=int, default=0)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--cores", type=int, default=8)
    ap.add_argument("--obstacles", type=int, default=5)
    ap.add_argument("--nx", type=int, default=100)
    ap.add_argument("--ny", type=int, default=100)
    ap.add_argument("--thetas", type=int, default=8, help="headings, evenly spaced over [0, 2 pi)")
    ap.add_argument("--speed", type=float, default=1.0)
    ap.add_argument("--flow-n", type=int, default=100, help="flow-field grid points per axis")
    ap.add_argument("--margin", type=float, default=0.0, help="flow-field grid margin (--margin 2.5 --flow-n 110: the visualiser's second form)")
    ap.add_argument("--chunk", type=int, default=65536)
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--out", metavar="FILE")
    ap.add_argument("--lookahead", action="store_true", help="IQN / DQN: add the one-step Bellman backup of every action (maps.lookahead_map)")
    ap.add_argument("--gamma", type=float, default=None, help="--lookahead: the discount (default: the env's)")
    ap.add_argument("--bench", action="store_true")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--inner", type=int, default=20, help="--bench: calls per timed window")
    args = ap.parse_args()
    if args.bench:
        return _bench(args)
    if not (args.iqn or args.dqn or args.planner):
        ap.error("one of --iqn, --dqn, --planner (or --bench)")
    import numpy as np
    from distributional_rl_navigation_amd import maps
    from distributional_rl_navigation_amd.marinenav_env.vec_env import VecMarineNavEnv
    env = _world(args, VecMarineNavEnv)
    if args.iqn:
        from distributional_rl_navigation_amd.iqn.agent import IQNAgent
        agent = IQNAgent(26, 9, device=args.device, seed=args.seed, BUFFER_SIZE=1024)
        agent.load_model(args.iqn, args.device)
        policy = maps.iqn_policy(agent, cvar=args.cvar, adaptive=args.adaptive, quantiles=args.quantiles)
    elif args.dqn:
        from distributional_rl_navigation_amd.dqn import DQNPolicy
        policy = maps.dqn_policy(DQNPolicy.load(args.dqn, device=args.device), q=args.lookahead)
    else:
        policy = maps.planner_policy(args.planner, env.params)
    xs = np.linspace(0.0, float(env.params.width), args.nx)
    ys = np.linspace(0.0, float(env.params.height), args.ny)
    thetas = np.arange(args.thetas) * (2 * np.pi / args.thetas)
    fx, fy, fv = maps.flow_field(env, 0, args.flow_n, args.flow_n, args.margin)
    res = maps.policy_map(policy, env, 0, xs, ys, thetas, args.speed, chunk=args.chunk)
    if args.lookahead:
        if args.planner:
            ap.error("--lookahead needs a policy with Q-values (--iqn or --dqn)")
        look = maps.lookahead_map(policy, env, 0, xs, ys, thetas, args.speed, gamma=args.gamma, chunk=args.chunk)
        res.update({k: look[k] for k in ("backup", "residual", "lookahead_action", "reward_next", "done_next", "info_next")})
    w = env.get_worlds()[0]
    env.close()
    out = args.out or "policy_map.npz"
    np.savez_compressed(out, xs=xs, ys=ys, thetas=thetas, speed=args.speed, flow_xs=fx, flow_ys=fy, flow_v=fv, cores=w["cores"], obstacles=w["obstacles"],
                        start=w["start"], goal=w["goal"], **res)
    print(f"{out}: {len(thetas)} x {len(ys)} x {len(xs)} poses; " + ", ".join(f"{k} {v.shape}" for k, v in res.items()))


if __name__ == "__main__":
    main()
