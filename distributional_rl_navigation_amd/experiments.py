"""Batched counterpart of the IQN part of the reference's run_experiments.py (:19-72,192-282).

The reference runs 500 randomised worlds x {adaptive IQN, IQN cvar 0.25 / 0.5 / 0.75 / 1.0} one episode at a
time on the CPU (`exp_setup_5`: fixed start (5,5) / goal (45,45), `set_boundary = True`, `robot.N = 5`,
`random_reset_state = False`, every test env seeded with 15 so that all agents see the same world sequence).
Here the worlds are generated once from the same RNG stream (bit-identical to the reference's), replicated
per policy into ONE vector env and all 500 x 5 episodes are stepped side by side on the GPU.
"""
import contextlib
import time

import numpy as np
import torch

from .episodes import EPISODE_TRACES, capture_lists, energy_table, host_traces, loop_episodes, tally
from .marinenav_env.vec_env import VecMarineNavEnv
from .planners import planner_act_batch

POLICIES = ("adaptive_IQN", "IQN_0.25", "IQN_0.5", "IQN_0.75", "IQN_1.0", "APF", "BA")   # run_experiments.py:216 (minus DQN)
ALL_POLICIES = POLICIES[:5] + ("DQN",) + POLICIES[5:]                                        # run_experiments.py:216, needs `dqn=`
_CVAR = {"IQN_0.25": 0.25, "IQN_0.5": 0.5, "IQN_0.75": 0.75, "IQN_1.0": 1.0}


@contextlib.contextmanager
def _producing(timings, device):
    """run_experiment(timings=...): the wall seconds of a trace-producing phase -- from its first launch until its traces are complete on the device --
    are added to timings["traces_s"]."""
    if timings is None:
        yield
        return
    torch.cuda.synchronize(device)
    t0 = time.perf_counter()
    yield
    torch.cuda.synchronize(device)
    timings["traces_s"] = timings.get("traces_s", 0.0) + time.perf_counter() - t0


def _configure(env):
    """exp_setup_5 (run_experiments.py:192-211)."""
    env.set_attrs(reset_start_and_goal=False, random_reset_state=False, set_boundary=True, obs_r_range=[1, 3], N=5)
    env.set_start_goal([5.0, 5.0], [45.0, 45.0])


def generate_worlds(num, n_obs, n_cores, seed=15, device="cuda:0"):
    """The world sequence every test env of the reference sees: `num` consecutive reset()s of one
    RandomState(seed) stream under exp_setup_5 settings."""
    gen = VecMarineNavEnv(1, seeds=[seed], device=device, precision="f64")
    _configure(gen)
    gen.set_attrs(num_cores=n_cores, num_obs=n_obs)
    worlds = []
    for _ in range(num):
        gen.reset()
        worlds.append(gen.get_worlds(0, 1)[0])
    gen.close()
    return worlds


CAPTURE_TRACES = ("traj",)                                   # what `capture` adds to EPISODE_TRACES for every policy ...
IQN_CAPTURE_TRACES = ("cvar", "quantiles", "taus")           # ... and for the IQN policies (act_eval's outputs)


def _episode_record(world, params, lists, seed=15):
    """One `ep_data` entry of the reference's exp_data JSON: MarineNavEnv.episode_data() (marinenav_env.py:557-622) of
    the finished episode plus, for the IQN policies, robot.actions_cvars / actions_quantiles / actions_taus
    (run_experiments.py:62-69).  `lists`: the episode's entry of `episodes.capture_lists`."""
    p = params
    ep = {"env": {}, "robot": {}}
    e = ep["env"]
    e["seed"] = seed
    e["width"], e["height"], e["r"], e["v_rel_max"], e["p"] = p.width, p.height, p.core_r, p.v_rel_max, p.p
    e["v_range"] = [p.v_range[0], p.v_range[1]]; e["obs_r_range"] = [p.obs_r_range[0], p.obs_r_range[1]]
    e["clear_r"] = p.clear_r
    e["start"] = [float(v) for v in world["start"]]; e["goal"] = [float(v) for v in world["goal"]]
    e["goal_dis"], e["timestep_penalty"], e["collision_penalty"] = p.goal_dis, p.timestep_penalty, p.collision_penalty
    e["goal_reward"], e["discount"] = p.goal_reward, p.discount
    c, o = world["cores"], world["obstacles"]
    e["cores"] = {"positions": [[float(r[0]), float(r[1])] for r in c], "clockwise": [int(r[2]) for r in c],
                  "Gamma": [float(r[3]) for r in c]}
    e["obstacles"] = {"positions": [[float(r[0]), float(r[1])] for r in o], "r": [float(r[2]) for r in o]}
    ep["robot"] = {"dt": p.dt, "N": p.N, "length": 1.0, "width": 0.5, "r": p.robot_r, "max_speed": p.max_speed,
                   "a": [p.a[0], p.a[1], p.a[2]], "w": [p.w[0], p.w[1], p.w[2]],
                   "init_theta": float(world["init_theta"]), "init_speed": float(world["init_speed"]),
                   "sonar": {"range": p.sonar_range, "angle": p.sonar_angle, "num_beams": p.num_beams}}
    ep["robot"].update(lists)
    return ep


def ep_data_from_traces(tr, length, worlds, params, seed=15):
    """The `ep_data` list of ONE policy from the numpy traces of its episodes -- `tr`: action [T][num], traj [T][num][N][2] and, for an IQN policy,
    cvar [T][num], quantiles [T][num][32][9], taus [T][num][32]; `length` [num]: `tally`'s -- whichever way they were produced (the per-step loop
    stacks what it collects per step into the same arrays the episode launches trace).  Episode i ran in worlds[i]."""
    return [_episode_record(w, params, lists, seed) for w, lists in zip(worlds, capture_lists(tr, length))]


def _records_from_traces(tr, params, names, num, launch_s=None, step_s=None, capture=None):
    """Result records of the policies `names` (policy p owns rows [p * num, (p + 1) * num)) from the numpy traces of their episodes, whichever way
    they were produced: `episodes.tally`'s numbers, sliced per policy.  `computation_times`, one entry per step of every episode, either way:
    `launch_s`, the device seconds of ONE launch that ran all the episodes, divided by the actions it chose; or `step_s`, per policy the per-step
    list of its act launch's device seconds per row served -- step t counts once for every env alive before it, i.e. with length > t.
    `capture` = (worlds, seed, iqn_tr, iqn_first): every record also gets its `ep_data` (ep_data_from_traces) from the traj trace in `tr` and, for an IQN
    policy -- a name in `iqn_first`, its first row in the cvar / quantiles / taus traces `iqn_tr` ([T][IQN rows]) --, from those."""
    tl = tally(tr["reward"], tr["done"], tr["info"], tr["action"], params.discount, energy_table(params.a[:], params.w[:]))
    length, info = tl["length"], tl["last_info"]
    dtN = params.dt * params.N
    out = {}
    for p, name in enumerate(names):
        sl = slice(p * num, (p + 1) * num)
        if step_s is None:
            times = [launch_s / max(1, int(length.sum()))] * int(length[sl].sum())
        else:
            times = [float(s_) for t, s_ in enumerate(step_s.get(name, [])) for _ in range(int((length[sl] > t).sum()))]
        out[name] = dict(success=[bool(v) for v in info[sl] == 4], out_of_area=[bool(v) for v in info[sl] == 1],
                         time=[float(dtN * l) for l in length[sl]], energy=[float(v) for v in tl["energy"][sl]],
                         reward=[float(v) for v in tl["ret"][sl]], actions=tl["actions"][sl], computation_times=times)
        if capture is not None:
            worlds, seed, iqn_tr, iqn_first = capture
            ptr = {k: tr[k][:, sl] for k in ("action", "traj")}
            if name in iqn_first:
                isl = slice(iqn_first[name], iqn_first[name] + num)
                ptr.update({k: iqn_tr[k][:, isl] for k in IQN_CAPTURE_TRACES})
            out[name]["ep_data"] = ep_data_from_traces(ptr, length[sl], worlds, params, seed)
    return out


def _noise_first(requested, names, num):
    """Under observation noise env row i of policy number p of the sweep is GLOBAL env p * num + i, whichever env holds it: the index of its first row for
    an env that holds the policies `names`, which must stand side by side in `requested`, in that order."""
    p0 = requested.index(names[0])
    if tuple(requested[p0:p0 + len(names)]) != tuple(names):
        raise ValueError(f"run_experiment(noise=...): the policies {names} share an env and must stand side by side in `policies` {requested}")
    return p0 * num


def _rollout_episodes(worlds, names, device, launch, capture=None, iqn=False, timings=None, noise=None, noise_first=0):
    """One env holding `worlds` once per policy of `names`, all of its episodes as ONE launch: `launch(env)` returns the traces (reward, done, info,
    action; with `capture` = the sweep's seed also traj and, `iqn`, cvar / quantiles / taus, which become the records' `ep_data`) or None where the
    library has no one-launch form of the policy.  Only the rows of the steps run are copied to the host.  Returns {name: record} or None."""
    env = VecMarineNavEnv(len(worlds) * len(names), device=device, precision="f64")
    _configure(env)
    env.load_worlds(worlds * len(names))
    if noise is not None:      # the launch feeds its policy the perceived rows (mn_set_obs_noise); its traces stay the clean ones
        env.set_obs_noise(noise, first_index=noise_first)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with _producing(timings, env.device):
        e0.record()
        tr = launch(env)
        e1.record()
    rec = None
    if tr is not None:
        torch.cuda.synchronize(env.device)
        also = () if capture is None else CAPTURE_TRACES + (IQN_CAPTURE_TRACES if iqn else ())
        host = host_traces(tr, also)
        cap = None if capture is None else (worlds, capture, host, {name: p * len(worlds) for p, name in enumerate(names)} if iqn else {})
        rec = _records_from_traces(host, env.params, names, len(worlds), launch_s=e0.elapsed_time(e1) * 1e-3, capture=cap)
    env.close()
    return rec


def _classical_episodes(worlds, name, device, max_steps, seed, capture=False, timings=None, noise=None, noise_first=0):
    """All of `worlds` under the classical baseline `name` ("APF" / "BA"), one episode each, as ONE launch: the policy runs inside the
    rollout kernel (VecMarineNavEnv.rollout_policy -> mn_rollout_policy).  Same result record as the launch-per-step path."""
    trace = EPISODE_TRACES + (CAPTURE_TRACES if capture else ())
    return _rollout_episodes(worlds, (name,), device, lambda env: env.rollout_policy(max_steps, name, trace=trace), capture=seed if capture else None,
                             timings=timings, noise=noise, noise_first=noise_first)[name]


@torch.no_grad()
def _iqn_episodes(worlds, names, agent, device, max_steps, capture=None, timings=None, noise=None, noise_first=0):
    """The IQN policies `names` on `worlds` as ONE mn_rollout_iqn_rows launch: policy p owns rows [p * num, (p + 1) * num), the rows of the per-step
    loop's IQN act call, so every row draws the taus it draws there.  With `capture` (the sweep's seed) the launch is mn_rollout_iqn_eval: it acts as
    the capture loop's act_eval_batch does and traces what that returns.  None where that loop's acting form has no one-launch twin (PyTorch acting,
    torch.rand taus, the exact-f32 variant)."""
    if not (agent.device.type == "cuda" and agent.use_fused_act and agent.use_library_rng):
        return None
    from .iqn.fused_act import ActRng, rollout_iqn
    if agent._act_rng is None:
        agent._act_rng = ActRng(agent.gen.initial_seed(), agent.device)
    num = len(worlds)
    cvar_rows = torch.tensor([_CVAR.get(name, 1.0) for name in names], dtype=torch.float32).repeat_interleave(num)
    adaptive_rows = torch.tensor([name == "adaptive_IQN" for name in names]).repeat_interleave(num)
    agent.qnetwork_local.eval()
    cap = capture is not None
    trace = EPISODE_TRACES + ((CAPTURE_TRACES + ("cvar",)) if cap else ())
    rec = _rollout_episodes(worlds, names, device, lambda env: rollout_iqn(agent.qnetwork_local, env, max_steps, agent._act_rng, cvar_rows=cvar_rows,
                                                                           adaptive_rows=adaptive_rows, trace=trace, want_quantiles=cap),
                            capture=capture, iqn=cap, timings=timings, noise=noise, noise_first=noise_first)
    agent.qnetwork_local.train()
    return rec


def run_experiment(agent, n_obs, n_cores, num=500, seed=15, policies=POLICIES, device="cuda:0", max_steps=1000, dqn=None,
                   capture=False, classical_rollout=True, one_launch=False, timings=None, noise=None):
    """run_experiments.py:213-282 for the IQN policies, the classical APF / BA baselines and (when `dqn`, a
    `dqn.DQNPolicy`, is given and "DQN" is in `policies`) the greedy DQN baseline.  Returns {policy: dict(success, time, energy,
    out_of_area, reward, actions)} with one entry per world.  With `capture` each policy also gets the reference's `ep_data`
    list (run_experiments.py:26-69,262-282): per episode the episode_data() dict incl. the sub-step trajectory, and for the
    IQN policies the per-action CVaR level, quantile values [1,32,9] and taus [1,32,1] of IQNAgent.act_eval -- the whole
    `exp_data` JSON the reference dumps.  `computation_times` (run_experiments.py:30,37-44,254-255: the wall-clock seconds of every
    act call, flattened over a policy's episodes) is the batched equivalent: the device time of the step's act launch(es) for that
    policy group (HIP events) divided by the rows the launch served, one entry per step of every episode -- the amortised cost of one
    action, which is what `avg_compute_t` (run_experiments.py:274) averages.
    `one_launch` (opt-in): the learned policies run whole episodes inside one kernel too -- the requested IQN policies as ONE
    mn_rollout_iqn_rows launch on one env of len(IQN policies) x num rows in the order of `policies` (per-row cvar and adaptive flag; the rows are the
    per-step loop's, so the taus are the same), DQN as one mn_rollout_dqn launch on its own env: with APF / BA the whole sweep is four launches.
    Results are bit-identical to the loop's; `computation_times` are built as for APF / BA (the launch's device time divided by the actions it
    chose).  Where the library has no one-launch form of a policy (an agent on the exact-f32 act variant or on torch.rand taus, a DQN policy with
    use_fused_act = False) that policy runs in the loop.  One difference: the agent's act-call counter ends at + the longest IQN episode, where the
    loop ends at + the longest episode of any policy in the loop.
    `capture` with `one_launch`: the same four launches also produce the `ep_data` -- every launch traces the sub-step positions of every step
    (mn_set_trajectory_trace), the IQN launch is mn_rollout_iqn_eval, which acts as act_eval does and traces the quantile values and taus of every
    action -- and both ways build `ep_data` with the same function from such traces (ep_data_from_traces), so the records are equal, `ep_data`
    included.  Trace memory on the device: max_steps x rows x (288 + 32) x 4 B for the IQN group -- about 3.2 GB for 500 worlds x 5 policies x
    1 000 steps -- and max_steps x rows x N x 16 B per launch for the trajectories, about 0.2 GB for that sweep's 2 500 IQN rows at N = 5; only the
    rows of the steps run are copied to the host.  `capture` without `one_launch` runs the loop for every policy, APF / BA included.
    `timings` (a dict, for measurements): timings["traces_s"] += the wall seconds of every trace-producing phase, launches and loop alike -- from its
    first launch until its traces are complete on the device (synchronised; the loop's per-step host copies are part of how it produces them) --, i.e.
    without the world generation, the env set-up and the host-side assembly of the records that both ways share.
    `noise` (an `obs_noise.ObsNoise`; None = perfect sensing, the code path as it was): every policy is fed what the robot perceives of its observations
    (include/marinenav_hip.h, "Observation noise") while the envs, the traces and the tallies stay those of the true state.  Row i of policy number p of
    `policies` is global env p * num + i in the noise key, whichever env holds it.  The loop wraps `act` with `env.perturb`; it runs EVERY policy (APF /
    BA too: no launch unless asked for).  With `one_launch` the same four launches run on envs with the description attached, bit-identical to that
    loop; `capture` with noise runs the loop.  Policies that share an env (the IQN group; whatever is left to the loop) must stand side by side in
    `policies`."""
    if noise is not None and noise.is_off:
        noise = None
    if noise is not None:
        one_launch = one_launch and not capture
        classical_rollout = classical_rollout and one_launch
    worlds = generate_worlds(num, n_obs, n_cores, seed, device)
    # APF / BA: the policy is a device function inside the episode rollout kernel -- one launch per policy for all worlds.  With `capture` the
    # launches run only on request (`one_launch`): otherwise the launch-per-step path below records the per-sub-step trajectory, as it always has
    requested = tuple(policies)
    rolled = {}
    if classical_rollout and (one_launch or not capture):
        rolled = {name: _classical_episodes(worlds, name, device, max_steps, seed, capture, timings, noise,
                                            _noise_first(requested, (name,), num) if noise is not None else 0)
                  for name in requested if name in ("APF", "BA")}
    if one_launch:
        iqn_names = tuple(p for p in requested if p == "adaptive_IQN" or p in _CVAR)
        if iqn_names:
            rolled.update(_iqn_episodes(worlds, iqn_names, agent, device, max_steps, seed if capture else None, timings, noise,
                                        _noise_first(requested, iqn_names, num) if noise is not None else 0) or {})
        if "DQN" in requested:
            if dqn is None:
                raise ValueError("policy 'DQN' needs run_experiment(..., dqn=DQNPolicy.load(...))")
            trace = EPISODE_TRACES + (CAPTURE_TRACES if capture else ())
            rolled.update(_rollout_episodes(worlds, ("DQN",), device, lambda env: dqn.rollout(env, max_steps, trace=trace),
                                            capture=seed if capture else None, timings=timings, noise=noise,
                                            noise_first=_noise_first(requested, ("DQN",), num) if noise is not None else 0) or {})
    policies = tuple(p for p in requested if p not in rolled)
    if not policies:
        return {name: rolled[name] for name in requested}, worlds
    n = num * len(policies)
    env = VecMarineNavEnv(n, device=device, precision="f64")
    _configure(env)
    obs = env.load_worlds(worlds * len(policies)).clone()          # policy p owns envs [p*num, (p+1)*num)
    dev = env.device
    fixed = torch.ones(n, device=dev)
    adaptive = torch.zeros(n, dtype=torch.bool, device=dev)
    classical = {}                                                 # policy name -> env rows driven by a planner
    iqn_rows = torch.zeros(n, dtype=torch.bool, device=dev)
    for p, name in enumerate(policies):
        rows = slice(p * num, (p + 1) * num)
        if name in ("APF", "BA", "DQN"):
            if name == "DQN" and dqn is None:
                raise ValueError("policy 'DQN' needs run_experiment(..., dqn=DQNPolicy.load(...))")
            classical[name] = rows
            continue
        iqn_rows[rows] = True
        if name == "adaptive_IQN":
            adaptive[rows] = True
        else:
            fixed[rows] = _CVAR[name]
    iqn_idx = torch.nonzero(iqn_rows).view(-1)
    cap = {}                                                       # capture: name -> numpy [max_steps][rows]..., row t filled by step t (allocated at step 0; untouched pages cost nothing)
    act_events = {}                                                # group -> [(start, end)] per step; groups: "IQN" (one launch for all IQN policies), planners

    def timed(group, fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        r = fn()
        e1.record()
        act_events.setdefault(group, []).append((e0, e1))
        return r

    def record(t, k, x):
        if k not in cap:
            cap[k] = np.empty((max_steps,) + x.shape, dtype=x.dtype)
        cap[k][t] = x

    def act(t, obs):
        a = torch.zeros(n, dtype=torch.int32, device=dev)
        if iqn_idx.numel():
            o = obs[iqn_idx].contiguous()

            def iqn_act():      # what the reference times (run_experiments.py:35-44): adjust_cvar + act_eval / act
                cv_ = torch.where(adaptive[iqn_idx], agent.adjust_cvar_batch(o), fixed[iqn_idx])   # agent.py:249-267 per row
                if capture:      # act_eval / act_adaptive_eval (agent.py:217-247): the action AND what it was chosen from
                    return (cv_,) + tuple(agent.act_eval_batch(o, 0.0, cv_))
                return cv_, agent.act_batch(o, 0.0, cv_), None, None
            cv, a_iqn, quant, taus = timed("IQN", iqn_act)
            a[iqn_idx] = a_iqn
            if capture:
                record(t, "cvar", cv.cpu().numpy()); record(t, "quantiles", quant.cpu().numpy()); record(t, "taus", taus.cpu().numpy()[:, :, 0])
        for name, rows in classical.items():                                 # APF.py:17-78 / BA.py:14-72
            if name == "DQN":                                                # run_experiments.py:86 (greedy predict)
                a[rows] = timed(name, lambda: dqn.act_batch(obs[rows]))
                continue
            a[rows] = timed(name, lambda: planner_act_batch(obs[rows], name, env.params.a[:], env.params.w[:]))      # one HIP launch (mn_planner_act)
        return a
    if capture:
        env.enable_trajectory()
    if noise is not None:      # obs -> perturb -> act; env.step keeps returning the clean rows
        env.set_obs_noise(noise, first_index=_noise_first(requested, policies, num))
        clean_act = act

        def act(t, obs):      # noqa: F811
            return clean_act(t, env.perturb(obs))
    if agent is not None:
        agent.qnetwork_local.eval()
    with _producing(timings, dev):
        tr = loop_episodes(env, obs, act, max_steps, after_step=(lambda t: record(t, "traj", env.get_trajectory())) if capture else None)
    if agent is not None:
        agent.qnetwork_local.train()
    torch.cuda.synchronize(dev)
    group_rows = {"IQN": max(1, int(iqn_idx.numel()))}
    step_s = {g: [e0.elapsed_time(e1) * 1e-3 / group_rows.get(g, num) for e0, e1 in evs] for g, evs in act_events.items()}
    # one entry per act call of the reference = per live episode and step: the step's amortised per-row device time
    host = host_traces(tr)
    capd = None
    if capture:      # the loop's captures as the launches' traces: [T][rows]..., T = the steps run
        T = host["done"].shape[0]
        host["traj"] = cap["traj"][:T]
        iqn_first = {name: k * num for k, name in enumerate(p_ for p_ in policies if p_ not in classical)}      # (iqn_idx is ascending: policy order)
        capd = (worlds, seed, {k: cap[k][:T] for k in IQN_CAPTURE_TRACES if k in cap}, iqn_first)
    out = _records_from_traces(host, env.params, policies, num,
                               step_s={name: step_s.get(name if name in classical else "IQN", []) for name in policies}, capture=capd)
    env.close()
    out.update(rolled)
    return {name: out[name] for name in requested}, worlds
