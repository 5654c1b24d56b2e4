"""The reference's full comparison (run_experiments.py:213-282: 8 policies x 500 worlds, exp_setup_5) on one GPU with the
reference's shipped IQN and DQN checkpoints (tests/golden/pretrained_*).

    python scripts/experiment_sweep.py [num] [n_obs] [n_cores] [--one-launch] [--capture] [--dump FILE]

--one-launch: whole episodes in one HIP launch per policy group (four launches) instead of one Python iteration per step; same results.
--capture   : every policy's `ep_data` as well (episode_data() per episode: sub-step trajectory, and for IQN the per-action CVaR level, quantile values, taus).
--dump FILE : write the result -- the reference's exp_data JSON (run_experiments.py:262-282) -- to FILE."""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from distributional_rl_navigation_amd.dqn import DQNPolicy
from distributional_rl_navigation_amd.experiments import ALL_POLICIES, run_experiment
from distributional_rl_navigation_amd.iqn.agent import IQNAgent

ap = argparse.ArgumentParser()
ap.add_argument("num", type=int, nargs="?", default=500)
ap.add_argument("n_obs", type=int, nargs="?", default=10)
ap.add_argument("n_cores", type=int, nargs="?", default=8)
ap.add_argument("--one-launch", action="store_true")
ap.add_argument("--capture", action="store_true")
ap.add_argument("--dump", metavar="FILE")
args = ap.parse_args()
num, n_obs, n_cores = args.num, args.n_obs, args.n_cores
kw = dict(policies=ALL_POLICIES, capture=args.capture, one_launch=args.one_launch)
G = os.path.join(ROOT, "tests", "golden")
agent = IQNAgent(26, 9, device="cuda:0", seed=0, BUFFER_SIZE=1024)
agent.load_model(os.path.join(G, "pretrained_IQN_seed3"), "cuda:0")
dqn = DQNPolicy.load(os.path.join(G, "pretrained_DQN_seed3", "q_net.npz"), device="cuda:0")
run_experiment(agent, n_obs, n_cores, num=8, dqn=dqn, **kw)      # warm-up
torch.cuda.synchronize(); t0 = time.perf_counter()
res, _ = run_experiment(agent, n_obs, n_cores, num=num, seed=15, dqn=dqn, **kw)
torch.cuda.synchronize(); dt = time.perf_counter() - t0
print(f"# run_experiment(pretrained IQN seed_3 + DQN seed_3, n_obs={n_obs}, n_cores={n_cores}, num={num}, seed=15, capture={args.capture}, one_launch={args.one_launch}): "
      f"{num} worlds x {len(ALL_POLICIES)} policies = {num * len(ALL_POLICIES)} episodes side by side on one MI355X: {dt:.2f} s wall-clock")
for name, r in res.items():
    ok = np.array(r["success"])
    print(f"{name:13s} success {ok.mean():.2f}  out_of_area {np.mean(r['out_of_area']):.2f}  "
          f"avg_time {np.mean(np.array(r['time'])[ok]) if ok.any() else float('nan'):.1f}  "
          f"avg_energy {np.mean(np.array(r['energy'])[ok]) if ok.any() else float('nan'):.1f}")
if args.dump:
    with open(args.dump, "w") as f:
        json.dump(res, f)
    print(f"# wrote {args.dump} ({os.path.getsize(args.dump) / 1e6:.1f} MB)")
