"""Batched counterpart of the IQN part of the reference's run_experiments.py (:19-72,192-282).

The reference runs 500 randomised worlds x {adaptive IQN, IQN cvar 0.25 / 0.5 / 0.75 / 1.0} one episode at a
time on the CPU (`exp_setup_5`: fixed start (5,5) / goal (45,45), `set_boundary = True`, `robot.N = 5`,
`random_reset_state = False`, every test env seeded with 15 so that all agents see the same world sequence).
Here the worlds are generated once from the same RNG stream (bit-identical to the reference's), replicated
per policy into ONE vector env and all 500 x 5 episodes are stepped side by side on the GPU.
"""
import torch

from .episodes import EPISODE_TRACES, energy_table, host_traces, loop_episodes, tally
from .marinenav_env.vec_env import VecMarineNavEnv
from .planners import planner_act_batch

POLICIES = ("adaptive_IQN", "IQN_0.25", "IQN_0.5", "IQN_0.75", "IQN_1.0", "APF", "BA")   # run_experiments.py:216 (minus DQN)
ALL_POLICIES = POLICIES[:5] + ("DQN",) + POLICIES[5:]                                        # run_experiments.py:216, needs `dqn=`
_CVAR = {"IQN_0.25": 0.25, "IQN_0.5": 0.5, "IQN_0.75": 0.75, "IQN_1.0": 1.0}


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


def _episode_record(world, params, name, actions, traj, cvars=None, quantiles=None, taus=None, seed=15):
    """One `ep_data` entry of the reference's exp_data JSON: MarineNavEnv.episode_data() (marinenav_env.py:557-622) of
    the finished episode plus, for the IQN policies, robot.actions_cvars / actions_quantiles / actions_taus
    (run_experiments.py:62-69)."""
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
                   "sonar": {"range": p.sonar_range, "angle": p.sonar_angle, "num_beams": p.num_beams},
                   "action_history": [int(a) for a in actions], "trajectory": [[float(q[0]), float(q[1])] for q in traj]}
    if cvars is not None:
        ep["robot"]["actions_cvars"] = [float(v) for v in cvars]
        ep["robot"]["actions_quantiles"] = [q.tolist() for q in quantiles]       # each [1][32][9], as act_eval returns
        ep["robot"]["actions_taus"] = [t.tolist() for t in taus]                 # each [1][32][1]
    return ep


def _records_from_traces(tr, params, names, num, launch_s=None, step_s=None):
    """Result records of the policies `names` (policy p owns rows [p * num, (p + 1) * num)) from the numpy traces of their episodes, whichever way
    they were produced: `episodes.tally`'s numbers, sliced per policy.  `computation_times`, one entry per step of every episode, either way:
    `launch_s`, the device seconds of ONE launch that ran all the episodes, divided by the actions it chose; or `step_s`, per policy the per-step
    list of its act launch's device seconds per row served -- step t counts once for every env alive before it, i.e. with length > t."""
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
    return out


def _rollout_episodes(worlds, names, device, launch):
    """One env holding `worlds` once per policy of `names`, all of its episodes as ONE launch: `launch(env)` returns the traces (reward, done, info,
    action) or None where the library has no one-launch form of the policy.  Returns {name: record} or None."""
    env = VecMarineNavEnv(len(worlds) * len(names), device=device, precision="f64")
    _configure(env)
    env.load_worlds(worlds * len(names))
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    tr = launch(env)
    e1.record()
    rec = None
    if tr is not None:
        torch.cuda.synchronize(env.device)
        rec = _records_from_traces(host_traces(tr), env.params, names, len(worlds), launch_s=e0.elapsed_time(e1) * 1e-3)
    env.close()
    return rec


def _classical_episodes(worlds, name, device, max_steps, seed):
    """All of `worlds` under the classical baseline `name` ("APF" / "BA"), one episode each, as ONE launch: the policy runs inside the
    rollout kernel (VecMarineNavEnv.rollout_policy -> mn_rollout_policy).  Same result record as the launch-per-step path."""
    return _rollout_episodes(worlds, (name,), device, lambda env: env.rollout_policy(max_steps, name))[name]


@torch.no_grad()
def _iqn_episodes(worlds, names, agent, device, max_steps):
    """The IQN policies `names` on `worlds` as ONE mn_rollout_iqn_rows launch: policy p owns rows [p * num, (p + 1) * num), the rows of the per-step
    loop's IQN act call, so every row draws the taus it draws there.  None where that loop's acting form has no one-launch twin (PyTorch acting,
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
    rec = _rollout_episodes(worlds, names, device, lambda env: rollout_iqn(agent.qnetwork_local, env, max_steps, agent._act_rng, cvar_rows=cvar_rows,
                                                                           adaptive_rows=adaptive_rows, trace=EPISODE_TRACES))
    agent.qnetwork_local.train()
    return rec


def run_experiment(agent, n_obs, n_cores, num=500, seed=15, policies=POLICIES, device="cuda:0", max_steps=1000, dqn=None,
                   capture=False, classical_rollout=True, one_launch=False):
    """run_experiments.py:213-282 for the IQN policies, the classical APF / BA baselines and (when `dqn`, a
    `dqn.DQNPolicy`, is given and "DQN" is in `policies`) the greedy DQN baseline.  Returns {policy: dict(success, time, energy,
    out_of_area, reward, actions)} with one entry per world.  With `capture` each policy also gets the reference's `ep_data`
    list (run_experiments.py:26-69,262-282): per episode the episode_data() dict incl. the sub-step trajectory, and for the
    IQN policies the per-action CVaR level, quantile values [1,32,9] and taus [1,32,1] of IQNAgent.act_eval -- the whole
    `exp_data` JSON the reference dumps.  `computation_times` (run_experiments.py:30,37-44,254-255: the wall-clock seconds of every
    act call, flattened over a policy's episodes) is the batched equivalent: the device time of the step's act launch(es) for that
    policy group (HIP events) divided by the rows the launch served, one entry per step of every episode -- the amortised cost of one
    action, which is what `avg_compute_t` (run_experiments.py:274) averages.
    `one_launch` (opt-in, ignored with `capture`): the learned policies run whole episodes inside one kernel too -- the requested IQN policies as ONE
    mn_rollout_iqn_rows launch on one env of len(IQN policies) x num rows in the order of `policies` (per-row cvar and adaptive flag; the rows are the
    per-step loop's, so the taus are the same), DQN as one mn_rollout_dqn launch on its own env: with APF / BA the whole sweep is four launches.
    Results are bit-identical to the loop's; `computation_times` are built as for APF / BA (the launch's device time divided by the actions it
    chose).  Where the library has no one-launch form of a policy (an agent on the exact-f32 act variant or on torch.rand taus, a DQN policy with
    use_fused_act = False) that policy runs in the loop.  One difference: the agent's act-call counter ends at + the longest IQN episode, where the
    loop ends at + the longest episode of any policy in the loop."""
    worlds = generate_worlds(num, n_obs, n_cores, seed, device)
    # APF / BA: the policy is a device function inside the episode rollout kernel -- one launch per policy for all worlds -- unless the
    # per-sub-step trajectory is wanted (`capture`), which the launch-per-step path below records
    requested = tuple(policies)
    rolled = {}
    if classical_rollout and not capture:
        rolled = {name: _classical_episodes(worlds, name, device, max_steps, seed) for name in requested if name in ("APF", "BA")}
    if one_launch and not capture:
        iqn_names = tuple(p for p in requested if p == "adaptive_IQN" or p in _CVAR)
        if iqn_names:
            rolled.update(_iqn_episodes(worlds, iqn_names, agent, device, max_steps) or {})
        if "DQN" in requested:
            if dqn is None:
                raise ValueError("policy 'DQN' needs run_experiment(..., dqn=DQNPolicy.load(...))")
            rolled.update(_rollout_episodes(worlds, ("DQN",), device,
                                            lambda env: dqn.rollout(env, max_steps, trace=EPISODE_TRACES)) or {})
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
    cap_cv, cap_q, cap_t, cap_traj = [], [], [], []
    act_events = {}                                                # group -> [(start, end)] per step; groups: "IQN" (one launch for all IQN policies), planners

    def timed(group, fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        r = fn()
        e1.record()
        act_events.setdefault(group, []).append((e0, e1))
        return r

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
                cap_cv.append(cv.cpu().numpy()); cap_q.append(quant.cpu().numpy()); cap_t.append(taus.cpu().numpy())
        for name, rows in classical.items():                                 # APF.py:17-78 / BA.py:14-72
            if name == "DQN":                                                # run_experiments.py:86 (greedy predict)
                a[rows] = timed(name, lambda: dqn.act_batch(obs[rows]))
                continue
            a[rows] = timed(name, lambda: planner_act_batch(obs[rows], name, env.params.a[:], env.params.w[:]))      # one HIP launch (mn_planner_act)
        return a
    if capture:
        env.enable_trajectory()
    if agent is not None:
        agent.qnetwork_local.eval()
    tr = loop_episodes(env, obs, act, max_steps, after_step=(lambda t: cap_traj.append(env.get_trajectory())) if capture else None)
    if agent is not None:
        agent.qnetwork_local.train()
    torch.cuda.synchronize(dev)
    group_rows = {"IQN": max(1, int(iqn_idx.numel()))}
    step_s = {g: [e0.elapsed_time(e1) * 1e-3 / group_rows.get(g, num) for e0, e1 in evs] for g, evs in act_events.items()}
    # one entry per act call of the reference = per live episode and step: the step's amortised per-row device time
    out = _records_from_traces(host_traces(tr), env.params, policies, num,
                               step_s={name: step_s.get(name if name in classical else "IQN", []) for name in policies})
    if capture:
        iqn_pos = {int(g_): k for k, g_ in enumerate(iqn_idx.cpu().numpy())}     # env row -> row of the IQN captures
        for p, name in enumerate(policies):
            eps_ = []
            for i in range(p * num, (p + 1) * num):
                acts_i = out[name]["actions"][i - p * num]
                L = len(acts_i)
                traj = [q for t_ in range(L) for q in cap_traj[t_][i]]
                if i in iqn_pos:
                    k = iqn_pos[i]
                    eps_.append(_episode_record(worlds[i - p * num], env.params, name, acts_i, traj,
                                                cvars=[cap_cv[t_][k] for t_ in range(L)],
                                                quantiles=[cap_q[t_][k:k + 1] for t_ in range(L)],
                                                taus=[cap_t[t_][k:k + 1] for t_ in range(L)], seed=seed))
                else:
                    eps_.append(_episode_record(worlds[i - p * num], env.params, name, acts_i, traj, seed=seed))
            out[name]["ep_data"] = eps_
    env.close()
    out.update(rolled)
    return {name: out[name] for name in requested}, worlds
