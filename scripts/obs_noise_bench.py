"""What observation noise costs an episode launch: each of the launches that has a noisy form -- the five IQN policies side by side, DQN, APF, BA -- on
the worlds of an evaluation config, with a description attached and with it detached, alternating, the same tree; the median and range of --repeats
timings each (HIP events around the launch).  The two runs are different episodes (the noise changes the actions, hence the lengths): the launch time
per step run is printed beside the launch time.
    python scripts/obs_noise_bench.py --eval-config tests/golden/eval_config_seed3.json --iqn tests/golden/pretrained_IQN_seed3 \\
        --dqn tests/golden/pretrained_DQN_seed3/q_net.npz"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--eval-config", required=True)
    ap.add_argument("--iqn", metavar="DIR")
    ap.add_argument("--dqn", metavar="FILE")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--max-steps", type=int, default=1000)
    ap.add_argument("--sigma-sonar", type=float, default=0.05)
    ap.add_argument("--miss", type=float, default=0.05)
    ap.add_argument("--sigma-vel", type=float, default=0.05)
    ap.add_argument("--sigma-goal", type=float, default=0.5)
    ap.add_argument("--device", default="cuda:0")
    args = ap.parse_args(argv)

    import numpy as np
    import torch
    from distributional_rl_navigation_amd.episodes import steps_run
    from distributional_rl_navigation_amd.marinenav_env.vec_env import VecMarineNavEnv
    from distributional_rl_navigation_amd.obs_noise import ObsNoise
    with open(args.eval_config) as f:
        cfg = json.load(f)
    worlds = [VecMarineNavEnv.world_from_eval_config(cfg[f"env_{k}"]) for k in range(len(cfg))]
    num = len(worlds)
    noise = ObsNoise(1, args.sigma_vel, args.sigma_goal, args.sigma_sonar, args.miss)
    trace = ("reward", "done", "info", "action")
    launches = []
    if args.iqn:
        from distributional_rl_navigation_amd.iqn.agent import IQNAgent
        from distributional_rl_navigation_amd.iqn.fused_act import ActRng, rollout_iqn
        agent = IQNAgent(26, 9, device=args.device, seed=0, BUFFER_SIZE=1024)
        agent.load_model(args.iqn, args.device)
        cv = torch.tensor([1.0, 0.25, 0.5, 0.75, 1.0]).repeat_interleave(num)
        ad = torch.tensor([True, False, False, False, False]).repeat_interleave(num)
        launches.append(("IQN x 5", 5, lambda env: rollout_iqn(agent.qnetwork_local, env, args.max_steps, ActRng(0, env.device), cvar_rows=cv, adaptive_rows=ad,
                                                             trace=trace)))
    if args.dqn:
        from distributional_rl_navigation_amd.dqn import DQNPolicy
        pol = DQNPolicy.load(args.dqn, device=args.device)
        launches.append(("DQN", 1, lambda env: pol.rollout(env, args.max_steps, trace=trace)))
    for name in ("APF", "BA"):
        launches.append((name, 1, lambda env, name=name: env.rollout_policy(args.max_steps, name, trace=trace)))
    print(f"{num} worlds; noise {noise}; {args.repeats} launches each way, alternating; median (min .. max) ms per launch, steps run, us per step run")
    for label, copies, run in launches:
        env = VecMarineNavEnv(num * copies, device=args.device, precision="f64")
        ms = {False: [], True: []}
        steps = {}
        for rep in range(args.repeats + 1):      # (the first pair warms up and is dropped)
            for on in (False, True):
                env.load_worlds(worlds, repeat=copies)
                env.set_obs_noise(noise if on else None)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                tr = run(env)
                e1.record()
                torch.cuda.synchronize()
                if rep:
                    ms[on].append(e0.elapsed_time(e1))
                steps[on] = steps_run(tr["done"].cpu().numpy())
        for on in (False, True):
            m = np.array(ms[on])
            print(f"{label:8s} {'noise attached' if on else 'detached      '}: {np.median(m):8.3f} ({m.min():.3f} .. {m.max():.3f}) ms, {steps[on]:4d} steps, "
                  f"{1e3 * np.median(m) / steps[on]:7.2f} us / step")
        env.close()


if __name__ == "__main__":
    main()
