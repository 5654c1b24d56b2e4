"""Evaluates N saved IQN (or, --agent dqn, DQN) networks on the evaluation worlds in ONE launch (iqn/deferred_eval.evaluate_checkpoints -> mn_rollout_iqn_groups): greedy
and adaptive-CVaR episodes of every network side by side, one group of rows per network.

    python scripts/evaluate_checkpoints.py DIR [DIR ...] [--eval-config eval_config.json] [--seed 0] [--no-adaptive] [--prefix best_] [--json out.json]

DIR holds network_params.pth + constructor_params.json (a train_iqn trial directory).  Without --eval-config the worlds are the 30 of
train_iqn.create_eval_configs (the reference's seed 348), or DIR/eval_config.json of the first directory if it is there.

    python scripts/evaluate_checkpoints.py --agent dqn A.zip B.zip ... [--eval-config eval_config.json] [--json out.json]

The DQN baseline (dqn/deferred_eval.evaluate_checkpoints -> mn_rollout_dqn_groups): every argument is what DQNPolicy.load reads -- best_model.zip /
latest_model.zip of a train_dqn trial, a policy.pth, the q_net .npz --; one policy, `greedy`, no seeds (the greedy DQN draws nothing).  Arguments that
all end in .zip / .pth / .npz select it without --agent.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("dirs", nargs="+", metavar="DIR")
    ap.add_argument("--agent", default=None, choices=["iqn", "dqn"], help="default: dqn if every argument ends in .zip / .pth / .npz, else iqn")
    ap.add_argument("--eval-config", default=None)
    ap.add_argument("-D", "--device", default="cuda:0")
    ap.add_argument("--seed", type=int, default=0, help="tau-stream seed, the same for every network (a network's result does not depend on its place in the list)")
    ap.add_argument("--no-adaptive", action="store_true")
    ap.add_argument("--max-steps", type=int, default=1000)
    ap.add_argument("--prefix", default="", help='checkpoint file prefix ("best_": the best evaluation of a run)')
    ap.add_argument("--precision", default="f64", choices=["f64", "mixed"])
    ap.add_argument("--json", default=None, metavar="FILE", help="also write the records (without the action lists) as JSON")
    args = ap.parse_args(argv)
    dqn = args.agent == "dqn" or (args.agent is None and all(d.endswith((".zip", ".pth", ".npz")) for d in args.dirs))
    path = args.eval_config or (os.path.join(args.dirs[0], "eval_config.json") if os.path.exists(os.path.join(args.dirs[0], "eval_config.json")) else None)
    if path is not None:
        with open(path) as f:
            cfg = json.load(f)
    else:
        from distributional_rl_navigation_amd.train_iqn import create_eval_configs
        cfg = create_eval_configs(args.device)
    mean_ok = lambda xs, ok: sum(x for x, o in zip(xs, ok) if o) / max(1, sum(ok)) if any(ok) else float("nan")
    header = f"{'checkpoint':<48}{'policy':<10}{'success':>9}{'mean return':>13}{'mean time s':>13}{'mean energy':>13}{'longest':>9}"
    if dqn:
        from distributional_rl_navigation_amd.dqn.deferred_eval import evaluate_checkpoints as evaluate_dqn_checkpoints
        recs = evaluate_dqn_checkpoints(args.dirs, cfg, args.device, max_steps=args.max_steps, precision=args.precision)
        print(f"{len(recs)} networks x {len(cfg)} worlds x 1 policy: one launch")
        print(header)
        for d, r in zip(args.dirs, recs):
            print(f"{d[-47:]:<48}{'greedy':<10}{r['n_successes']:>6}/{r['n_worlds']:<2}{r['mean_return']:>13.2f}{mean_ok(r['times'], r['successes']):>13.2f}"
                  f"{mean_ok(r['energies'], r['successes']):>13.2f}{r['steps_run']:>9}")
        if args.json:
            with open(args.json, "w") as f:
                json.dump([dict(checkpoint=d, steps_run=r["steps_run"],
                                greedy=dict(successes=r["n_successes"], n_worlds=r["n_worlds"], mean_return=r["mean_return"], rewards=r["rewards"].tolist(),
                                            success=r["successes"].tolist(), times=r["times"].tolist(), energies=r["energies"].tolist()))
                           for d, r in zip(args.dirs, recs)], f)
        return recs
    from distributional_rl_navigation_amd.iqn.deferred_eval import evaluate_checkpoints
    from distributional_rl_navigation_amd.iqn.model import ObsEncoder
    nets = [ObsEncoder.load(d, args.device, prefix=args.prefix) for d in args.dirs]
    recs = evaluate_checkpoints(nets, cfg, args.device, adaptive=not args.no_adaptive, seeds=[args.seed] * len(nets), max_steps=args.max_steps,
                                precision=args.precision)
    policies = ("greedy",) if args.no_adaptive else ("greedy", "adaptive")
    print(f"{len(nets)} networks x {len(cfg)} worlds x {len(policies)} policies: one launch")
    print(header)
    for d, r in zip(args.dirs, recs):
        for p in policies:
            e = r[p]
            print(f"{d[-47:]:<48}{p:<10}{e['successes']:>6}/{e['n_worlds']:<2}{e['mean_return']:>13.2f}{mean_ok(e['times'], e['success']):>13.2f}"
                  f"{mean_ok(e['energies'], e['success']):>13.2f}{r['steps_run']:>9}")
    if args.json:
        with open(args.json, "w") as f:
            json.dump([dict(checkpoint=d, steps_run=r["steps_run"], **{p: {k: v for k, v in r[p].items() if k != "actions"} for p in policies})
                       for d, r in zip(args.dirs, recs)], f)
    return recs


if __name__ == "__main__":
    main()
