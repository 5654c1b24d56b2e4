"""Episode bookkeeping of every evaluation: the one place where per-step results become per-episode numbers.

Evaluation episodes are produced either by one HIP launch (VecMarineNavEnv.rollout_policy, iqn.fused_act.rollout_iqn, DQNPolicy.rollout) or by
the per-step Python loop (`loop_episodes`).  Both give the same `[T][n]` traces -- reward, done, info, action, with a finished env idling at
reward 0, done 1, its terminal info code and action -1; for captured episodes also traj and, for IQN, cvar / quantiles / taus (`capture_lists`) -- and `tally` turns traces into the discounted return, energy, length, last info code and
action list of every env.  The consumers (IQNAgent.evaluation_vec, train_dqn.evaluate, experiments.run_experiment) only format what it returns.
Plain numpy and torch: nothing here needs the HIP library, so all of it runs on a machine without a GPU.
"""
import numpy as np
import torch

EPISODE_TRACES = ("reward", "done", "info", "action")

# trace name -> (shape behind [T][n], dtype, initial fill; None = uninitialised: the producer writes every row it reports)
_TRACES = dict(obs=(("obs_dim",), torch.float32, 0.0),
               reward=((), torch.float32, None),
               done=((), torch.uint8, None),
               info=((), torch.uint8, None),
               action=((), torch.int32, None),
               cvar=((), torch.float32, float("nan")),
               q=(("n_actions",), torch.float32, float("nan")),
               # what an IQN action was chosen from (act_eval's quantile values and taus: rollout_iqn(want_quantiles=True)) and the sub-step positions of a step
               quantiles=(("n_taus", "n_actions"), torch.float32, float("nan")),
               taus=(("n_taus",), torch.float32, float("nan")),
               traj=(("n_substeps", "xy"), torch.float64, float("nan")))


def trace_buffers(T, n, device, names, fill=True, obs_dim=26, n_actions=9, n_taus=32, n_substeps=None):
    """The `[T][n]` trace tensors `names` of one episode producer.  The entries a finished env never writes start as obs 0, cvar / q / quantiles /
    taus / traj NaN; with `fill=False` nothing is initialised (VecMarineNavEnv.rollout resets its envs and writes every row).  "traj"
    ([T][n][n_substeps][2] float64) needs `n_substeps`, the robot's N."""
    dims = dict(obs_dim=obs_dim, n_actions=n_actions, n_taus=n_taus, n_substeps=n_substeps, xy=2)
    assert "traj" not in names or n_substeps, "the traj trace needs n_substeps"
    out = {}
    for k in names:
        tail, dtype, init = _TRACES[k]
        shape = (T, n) + tuple(dims[d] for d in tail)
        out[k] = torch.empty(shape, dtype=dtype, device=device) if init is None or not fill else torch.full(shape, init, dtype=dtype, device=device)
    return out


def energy_table(a, w):
    """robot.py:72-77: the energy of each of the 9 actions (acceleration i, angular velocity j) -> |a_i / max a| + |w_j / max w|, float32 [9]."""
    a, w = np.asarray(a, dtype=np.float32), np.asarray(w, dtype=np.float32)
    return (np.abs(a / a.max()).reshape(3, 1) + np.abs(w / w.max()).reshape(1, 3)).reshape(-1)


def steps_run(done):
    """The number of steps the per-step loop runs on the `done` trace [T][n]: through the step that ends the last episode, or all T rows if an
    episode is still alive behind them."""
    done = np.asarray(done).astype(bool)
    return int(np.where(done.any(axis=0), done.argmax(axis=0) + 1, done.shape[0]).max(initial=0))


def tally(reward, done, info, action, discount, energy_tab):
    """THE step loop over the traces (numpy [T][n]) of n episodes: per env the discounted return (float64), the energy (float64), the length (int64),
    the last info code (uint8) and the list of its actions -- return += (discount ** t) * reward, energy += energy_tab[action] while the env is
    alive, in step order.  Rows behind `steps_run(done)` are not looked at: every env is finished there."""
    T = steps_run(done)
    n = reward.shape[1]
    alive = np.ones(n, dtype=bool)
    ret = np.zeros(n, dtype=np.float64)
    energy = np.zeros(n, dtype=np.float64)
    length = np.zeros(n, dtype=np.int64)
    last_info = np.zeros(n, dtype=np.uint8)
    etab = np.asarray(energy_tab, dtype=np.float32).astype(np.float64)
    for t in range(T):
        ret += np.where(alive, (discount ** t) * reward[t].astype(np.float64), 0.0)
        length += alive
        energy += np.where(alive, etab[np.clip(action[t], 0, len(etab) - 1)], 0.0)      # (a finished env's -1 is masked either way)
        last_info = np.where(alive, info[t], last_info)
        alive = alive & ~done[t].astype(bool)
    by_env = np.ascontiguousarray(action[:T].T)
    return dict(ret=ret, energy=energy, length=length, last_info=last_info, actions=[by_env[i, :length[i]].tolist() for i in range(n)])


def capture_lists(tr, length):
    """What the reference's robot accumulates over an episode, per env, from the numpy traces `tr` of n episodes and `tally`'s `length` [n]: a list of
    n dicts with `action_history` (L actions) and `trajectory` (N x L sub-step positions [x, y], from "traj" [T][n][N][2]) and -- when `tr` has
    "quantiles" -- the IQN policies' `actions_cvars` (L), `actions_quantiles` (L x [1][32][9]) and `actions_taus` (L x [1][32][1]), L = the env's
    length.  Plain Python numbers throughout (JSON); rows behind an env's end are not looked at."""
    iqn = "quantiles" in tr
    out = []
    for i, L in enumerate(int(l) for l in length):
        d = {"action_history": tr["action"][:L, i].tolist(), "trajectory": tr["traj"][:L, i].reshape(-1, 2).tolist()}
        if iqn:
            d["actions_cvars"] = tr["cvar"][:L, i].tolist()
            d["actions_quantiles"] = tr["quantiles"][:L, i][:, None].tolist()            # each [1][32][9], as act_eval returns
            d["actions_taus"] = tr["taus"][:L, i][:, None, :, None].tolist()             # each [1][32][1]
        out.append(d)
    return out


@torch.no_grad()
def loop_episodes(env, obs, act, max_steps, after_step=None):
    """The per-step twin of the episode launches: from the observations `obs` [n][26], up to `max_steps` times `a = act(t, obs)` (int32 [n]) and
    `obs, reward, done, info = env.step(a)` (then `after_step(t)`), stopping after the step that ends the last episode (one host look per step).
    `env` is anything with such a `step`, on any device.  Returns what the launches return: the traces reward / done / info / action of the steps
    run, a finished env's entries as the launches write them (reward 0, done 1, its terminal info code, action -1), `final_obs` and `steps_run`."""
    n, dev = obs.shape[0], obs.device
    tr = trace_buffers(max_steps, n, dev, EPISODE_TRACES)
    idle = {k: torch.tensor(v, dtype=tr[k].dtype, device=dev) for k, v in (("reward", 0.0), ("done", 1), ("action", -1))}
    alive = torch.ones(n, dtype=torch.bool, device=dev)
    steps = 0
    for t in range(max_steps):
        a = act(t, obs)
        obs, reward, done, info = env.step(a)
        if after_step is not None:
            after_step(t)
        # row t: the step's results where the env is alive, the idle entries (for info: the row above, its terminal code) where it has finished
        for k, x in (("reward", reward), ("done", done), ("info", info), ("action", a)):
            x = x.to(tr[k].dtype)
            torch.where(alive, x, idle[k] if k in idle else tr[k][t - 1] if t else x, out=tr[k][t])
        alive = alive & (done == 0)
        steps = t + 1
        if not bool(alive.any()):
            break
    out = {k: v[:steps] for k, v in tr.items()}
    out["final_obs"] = obs
    out["steps_run"] = steps
    return out


def host_traces(tr, also=()):
    """The four bookkeeping traces of an episode producer's result (and those named in `also`) as numpy arrays: `done` first, then of the others only
    the `steps_run(done)` rows that `tally` looks at (a launch writes all T rows however early its last episode ends)."""
    done = tr["done"].cpu().numpy()
    T = steps_run(done)
    return dict({k: tr[k][:T].cpu().numpy() for k in EPISODE_TRACES + tuple(also) if k != "done"}, done=done[:T])
