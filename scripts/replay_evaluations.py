"""Replay the action lists a training run stored in its *_evaluations.npz, all of them in ONE launch, and compare with what it stored.

    python scripts/replay_evaluations.py --config eval_config.json --evaluations greedy_evaluations.npz --out replay.npz
    python scripts/replay_evaluations.py --config eval_config.json --evaluations greedy_evaluations.npz --ids 0,150,299 --substeps
    python scripts/replay_evaluations.py --config tests/golden/eval_config_seed3.json --evaluations tests/golden/g6_pretrained_replay.npz --subset greedy

A training run of the reference evaluates its agent every so often on the worlds of eval_config.json and appends to *_evaluations.npz, per evaluation
and world, the action list, the discounted return, the success flag, the time and the energy (`actions`, `rewards`, `successes`, `times`, `energies`:
object arrays [evaluation][world]).  This is what env_visualizer's load_episode_from_eval_files replays one episode at a time.  Here the worlds are
loaded once into one handle and every stored list is one query of ONE `VecMarineNavEnv.rollout_at` call -- a world index and a length per query, no
handle row per episode, nothing stepped.  `--subset NAME` reads the flattened subset form of tests/golden/g6_pretrained_replay.npz instead
(`NAME_actions` [n][1000] padded with -1, `NAME_len`, `NAME_reward`, `NAME_success`, `NAME_ids` = (evaluation, world)).

The .npz written holds per replayed episode: ids (evaluation, world), length, steps (what the replay ran), info (the terminal code), success, time,
energy, ret (the discounted return recomputed by episodes.tally), stored_ret / stored_success, xy [n][H][2] (the position after every step, NaN behind
the end) and with --substeps traj [n][H * N][2].  Printed: the largest |recomputed - stored return| and every success flag that differs.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def load_lists(path, ids=None, subset=None):
    """(ids [n][2] = evaluation, world; actions: n lists; stored return [n]; stored success [n]) from an evaluations file."""
    import numpy as np
    z = np.load(path, allow_pickle=subset is None)
    if subset is not None:
        length = z[f"{subset}_len"]
        acts = [z[f"{subset}_actions"][i][:int(length[i])].tolist() for i in range(len(length))]
        keep = [i for i in range(len(length)) if ids is None or int(z[f"{subset}_ids"][i][0]) in ids]
        return (np.asarray(z[f"{subset}_ids"])[keep].reshape(-1, 2), [acts[i] for i in keep], np.asarray(z[f"{subset}_reward"], dtype=np.float64)[keep],
                np.asarray(z[f"{subset}_success"], dtype=bool)[keep])
    evals = range(len(z["actions"])) if ids is None else ids
    out_ids, acts, ret, succ = [], [], [], []
    for e in evals:
        for k in range(len(z["actions"][e])):
            out_ids.append((e, k)); acts.append([int(a) for a in z["actions"][e][k]])
            ret.append(float(z["rewards"][e][k])); succ.append(bool(z["successes"][e][k]))
    return np.array(out_ids, dtype=np.int64).reshape(-1, 2), acts, np.array(ret, dtype=np.float64), np.array(succ, dtype=bool)


def replay(cfg, ids, acts, device="cuda:0", substeps=False):
    """Every action list in one rollout_at call, in the worlds of `cfg` (an eval_config.json as a dict).  Returns a dict of numpy arrays."""
    import numpy as np
    import torch
    from distributional_rl_navigation_amd import _capi
    from distributional_rl_navigation_amd.episodes import energy_table, tally
    from distributional_rl_navigation_amd.marinenav_env.vec_env import VecMarineNavEnv
    worlds = [VecMarineNavEnv.world_from_eval_config(cfg[f"env_{k}"]) for k in range(len(cfg))]
    env = VecMarineNavEnv(len(worlds), device=device, precision="f64")
    robot_n = {int(cfg[f"env_{k}"]["robot"]["N"]) for k in range(len(cfg))}
    if len(robot_n) != 1:
        raise ValueError(f"the worlds of the config disagree on robot.N: {sorted(robot_n)}")
    env.set_attrs(N=robot_n.pop())
    env.load_worlds(worlds)      # once: every query names its world by index
    n = len(acts)
    length = np.array([len(a) for a in acts], dtype=np.int32)
    H = int(length.max(initial=0))
    if H > _capi.QUERY_MAX_STEPS:
        raise ValueError(f"an action list of {H} steps is longer than MN_QUERY_MAX_STEPS = {_capi.QUERY_MAX_STEPS}")
    padded = np.zeros((n, H), dtype=np.int32)
    for i, a in enumerate(acts):
        padded[i, :len(a)] = a
    world = np.asarray(ids)[:, 1].astype(np.int32)
    start = np.array([[worlds[k]["start"][0], worlds[k]["start"][1], worlds[k]["init_theta"], worlds[k]["init_speed"]] for k in world]).reshape(n, 4)
    trace = ("reward", "done", "info", "action", "state") + (("traj",) if substeps else ())
    out = env.rollout_at(start, padded, lengths=length, env=world, trace=trace, dtype=torch.float64)
    host = {k: v.cpu().numpy() for k, v in out.items()}
    t = tally(host["reward_trace"], host["done_trace"], host["info_trace"], host["action_trace"], float(env.discount),
              energy_table([float(v) for v in env.params.a], [float(v) for v in env.params.w]))
    steps = host["steps"].astype(np.int64)
    xy = np.ascontiguousarray(host["state_trace"][:, :, :2].transpose(1, 0, 2))      # [n][H][2]
    xy[np.arange(H)[None, :] >= steps[:, None]] = np.nan
    res = dict(ids=np.asarray(ids), length=length.astype(np.int64), steps=steps, info=host["info"], success=host["info"] == 4,
               time=float(env.params.dt) * int(env.params.N) * steps, energy=t["energy"], ret=t["ret"], xy=xy)
    if substeps:
        res["traj"] = np.ascontiguousarray(host["traj_trace"].transpose(1, 0, 2, 3)).reshape(n, -1, 2)
    env.close()
    return res


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--config", required=True, metavar="JSON", help="eval_config.json")
    ap.add_argument("--evaluations", required=True, metavar="NPZ", help="*_evaluations.npz")
    ap.add_argument("--ids", help="comma-separated evaluation indices (default: all)")
    ap.add_argument("--subset", metavar="NAME", help="read the flattened subset form (tests/golden/g6_pretrained_replay.npz: greedy | adaptive)")
    ap.add_argument("--substeps", action="store_true", help="also store the sub-step trajectories")
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--out", metavar="FILE", default="replay_evaluations.npz")
    args = ap.parse_args(argv)
    import numpy as np
    with open(args.config) as f:
        cfg = json.load(f)
    ids = [int(v) for v in args.ids.split(",")] if args.ids else None
    eid, acts, stored_ret, stored_succ = load_lists(args.evaluations, ids, args.subset)
    res = replay(cfg, eid, acts, device=args.device, substeps=args.substeps)
    res["stored_ret"], res["stored_success"] = stored_ret, stored_succ
    np.savez_compressed(args.out, **res)
    diff = np.abs(res["ret"] - stored_ret)
    worst = int(diff.argmax()) if len(diff) else -1
    print(f"{args.out}: {len(acts)} episodes, {int(res['steps'].sum())} steps in one launch; steps differ from the stored length in "
          f"{int((res['steps'] != res['length']).sum())}")
    print(f"largest |recomputed - stored return| = {diff.max(initial=0.0):.3e}" + (f" (evaluation {eid[worst][0]}, world {eid[worst][1]}, {res['length'][worst]} steps)" if worst >= 0 else ""))
    flips = np.nonzero(res["success"] != stored_succ)[0]
    print(f"success flags that differ: {len(flips)}" + "".join(f"\n  evaluation {eid[i][0]}, world {eid[i][1]}: replayed {bool(res['success'][i])}, stored {bool(stored_succ[i])}" for i in flips))
    return res


if __name__ == "__main__":
    main()
