"""Policies x observation-noise levels on an evaluation config: how every policy degrades when the robot knows less than it would like.

Every cell is one episode launch per policy on the config's worlds with an `obs_noise.ObsNoise` attached to the env (VecMarineNavEnv.set_obs_noise): the
policy is fed what the robot perceives, the env and the tallies stay those of the true state.  The grid is the product of --sigma-sonar, --miss and
--sigma-vel (with --sigma-goal for every cell); the all-zero cell is the clean run.  Per cell and policy: successes, the share of episodes that end in
a collision, and the median of time / T(start) over the successful episodes (T: the world's minimum-time-to-goal field, scripts/time_field.py).  The
field pilot (--pilot) reads no observation: one row, the noise-free ceiling of every cell.
    python scripts/robustness_sweep.py --eval-config tests/golden/eval_config_seed3.json --iqn tests/golden/pretrained_IQN_seed3 \\
        --dqn tests/golden/pretrained_DQN_seed3/q_net.npz --planner APF BA --pilot --sigma-sonar 0,0.02,0.05,0.1 --miss 0,0.05,0.2 --out robustness"""
import argparse
import itertools
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

IQN_ROWS = (("adaptive IQN", 1.0, True), ("IQN 0.25", 0.25, False), ("IQN 0.5", 0.5, False), ("IQN 0.75", 0.75, False), ("IQN 1.0", 1.0, False))
TRACE = ("reward", "done", "info", "action")


def _floats(s):
    return [float(v) for v in s.split(",") if v != ""]


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--eval-config", required=True)
    ap.add_argument("--iqn", metavar="DIR", help="an IQN checkpoint: adaptive CVaR and the fixed levels 0.25 / 0.5 / 0.75 / 1.0, one launch per cell")
    ap.add_argument("--dqn", metavar="FILE")
    ap.add_argument("--planner", nargs="*", choices=("APF", "BA"), default=())
    ap.add_argument("--pilot", action="store_true", help="the field pilot: reads no observation, the ceiling")
    ap.add_argument("--pilot-horizon", type=int, default=2)
    ap.add_argument("--sigma-sonar", type=_floats, default=[0.0, 0.02, 0.05, 0.1], help="relative range errors, comma separated")
    ap.add_argument("--miss", type=_floats, default=[0.0], help="probabilities that a return is lost")
    ap.add_argument("--sigma-vel", type=_floats, default=[0.0], help="DVL errors in m/s")
    ap.add_argument("--sigma-goal", type=float, default=0.0, help="goal error in m, every cell")
    ap.add_argument("--noise-seed", type=int, default=1)
    ap.add_argument("--max-steps", type=int, default=1000)
    ap.add_argument("--nx", type=int, default=128)
    ap.add_argument("--ny", type=int, default=128)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--out", metavar="STEM", help="writes STEM.txt (the table) and STEM.npz")
    args = ap.parse_args(argv)

    import numpy as np
    import torch
    from distributional_rl_navigation_amd import maps
    from distributional_rl_navigation_amd.marinenav_env.vec_env import VecMarineNavEnv
    from distributional_rl_navigation_amd.obs_noise import ObsNoise
    with open(args.eval_config) as f:
        cfg = json.load(f)
    worlds = [VecMarineNavEnv.world_from_eval_config(cfg[f"env_{k}"]) for k in range(len(cfg))]
    num = len(worlds)
    env = VecMarineNavEnv(num, device=args.device, precision="f64")
    env.load_worlds(worlds)
    T, d, status, sweeps = env.time_field(torch.arange(num, dtype=torch.int32), args.nx, args.ny)
    W, H = float(env.params.width), float(env.params.height)
    starts = torch.tensor(np.array([w["start"] for w in worlds], dtype=np.float64), device=env.device)
    t_start = torch.stack([maps.time_at(maps.field_dict(T[i], d[i], W, H, int(status[i]), int(sweeps[i])), starts[i:i + 1])[0] for i in range(num)])
    step_s = env.params.dt * env.params.N

    def tally(tr, rows):
        """(successes, collisions, median time / T(start)) of the episodes in columns `rows` of a launch's traces."""
        done, info = tr["done"][:, rows].bool(), tr["info"][:, rows]
        last = done.to(torch.uint8).argmax(dim=0)
        end = info[last, torch.arange(done.shape[1], device=done.device)]
        success = done.any(dim=0) & (end == 4)
        ok = success & torch.isfinite(t_start)
        ratio = ((last + 1).double() * step_s / t_start)[ok]
        return int(success.sum()), int((done.any(dim=0) & (end == 3)).sum()), float(ratio.median()) if ratio.numel() else float("nan")

    agent = dqn = iqn_env = None
    if args.iqn:
        from distributional_rl_navigation_amd.iqn.agent import IQNAgent
        from distributional_rl_navigation_amd.iqn.fused_act import ActRng, rollout_iqn
        agent = IQNAgent(26, 9, device=args.device, seed=args.seed, BUFFER_SIZE=1024)
        agent.load_model(args.iqn, args.device)
        iqn_env = VecMarineNavEnv(num * len(IQN_ROWS), device=args.device, precision="f64")      # the five IQN policies side by side: one launch per cell
        cvar_rows = torch.tensor([r[1] for r in IQN_ROWS]).repeat_interleave(num)
        adaptive_rows = torch.tensor([r[2] for r in IQN_ROWS]).repeat_interleave(num)
    if args.dqn:
        from distributional_rl_navigation_amd.dqn import DQNPolicy
        dqn = DQNPolicy.load(args.dqn, device=args.device)

    cells = [ObsNoise(args.noise_seed, vs, args.sigma_goal, ss, mp) for ss, mp, vs in itertools.product(args.sigma_sonar, args.miss, args.sigma_vel)]
    names = ([r[0] for r in IQN_ROWS] if agent else []) + (["DQN"] if dqn else []) + list(args.planner)
    table = {name: [] for name in names}
    for noise in cells:
        nz = None if noise.is_off else noise
        if agent:      # (row p * num + i of the launch is global env p * num + i of the noise key: every policy and world its own draws)
            iqn_env.load_worlds(worlds, repeat=len(IQN_ROWS))
            iqn_env.set_obs_noise(nz, first_index=0)
            tr = rollout_iqn(agent.qnetwork_local, iqn_env, args.max_steps, ActRng(args.seed, iqn_env.device), cvar_rows=cvar_rows, adaptive_rows=adaptive_rows,
                             trace=TRACE)
            if tr is None:
                raise SystemExit("the IQN episode launch refused this form")
            for p, row in enumerate(IQN_ROWS):
                table[row[0]].append(tally(tr, slice(p * num, (p + 1) * num)))
        for name in (["DQN"] if dqn else []) + list(args.planner):
            env.load_worlds(worlds)
            env.set_obs_noise(nz, first_index=0)
            tr = dqn.rollout(env, args.max_steps, trace=TRACE) if name == "DQN" else env.rollout_policy(args.max_steps, name, trace=TRACE)
            if tr is None:
                raise SystemExit("the DQN episode launch does not run this network")
            table[name].append(tally(tr, slice(0, num)))
    pilot = None
    if args.pilot:
        env.load_worlds(worlds)
        env.set_obs_noise(None)
        pilot = tally(env.rollout_pilot(args.max_steps, T, horizon=args.pilot_horizon, trace=TRACE), slice(0, num))

    head = [f"sonar {n.sonar_rel_sigma:g} miss {n.sonar_miss_p:g} vel {n.vel_sigma:g}" for n in cells]
    lines = [f"{num} worlds of {args.eval_config}; goal sigma {args.sigma_goal:g} m, noise seed {args.noise_seed}; per cell: successes / collisions / median time / T(start)",
             "policy".ljust(14) + " | " + " | ".join(h.ljust(30) for h in head)]
    for name in names:
        lines.append(name.ljust(14) + " | " + " | ".join(f"{s:3d} / {c:3d} / {r:6.3f}".ljust(30) for s, c, r in table[name]))
    if pilot is not None:
        lines.append(f"PILOT horizon {args.pilot_horizon} (no observation: every cell): {pilot[0]} / {pilot[1]} / {pilot[2]:.3f}")
    print("\n".join(lines))
    if args.out:
        with open(args.out + ".txt", "w") as f:
            f.write("\n".join(lines) + "\n")
        np.savez(args.out + ".npz", policies=np.array(names), cells=np.array([[n.sonar_rel_sigma, n.sonar_miss_p, n.vel_sigma, n.goal_sigma] for n in cells]),
                 table=np.array([table[name] for name in names], dtype=np.float64), pilot=np.array(pilot if pilot is not None else [np.nan] * 3),
                 T_start=t_start.cpu().numpy())
    env.close()
    if iqn_env is not None:
        iqn_env.close()


if __name__ == "__main__":
    main()
