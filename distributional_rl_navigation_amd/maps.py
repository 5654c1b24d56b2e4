"""Maps of a world: its flow field, and what a policy does at every pose of a grid.

The reference's visualiser asks its environment two things besides replaying episodes: the current at a point
(`env_visualizer.plot_graph` evaluates `get_velocity` on a 100 x 100 grid) and the observation of a robot placed by hand.  Here both
are queries of `VecMarineNavEnv` (`velocity_at`, `observation_at`: one HIP launch for the whole grid, nothing in the env changes), and
a policy map is the observation query followed by the policy's own act call on the rows it returns.  `action_fan` and `lookahead_map` add
the other half -- what happens if the robot placed there takes an action (`step_at`, `constant_rollout_at`: the what-if step).  Nothing here plots.
"""
import numpy as np
import torch


def _host(t):
    return t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)


def flow_field(env, env_index=0, nx=100, ny=100, margin=0.0):
    """The current of world `env_index` on the grid of env_visualizer.plot_graph: xs = linspace(-margin, width + margin, nx), ys likewise over the
    height (`margin=2.5, nx=ny=110` is the visualiser's second form).  Returns (xs [nx], ys [ny], v [ny][nx][2]) as float64 arrays."""
    xs = np.linspace(-float(margin), float(env.params.width) + float(margin), int(nx))
    ys = np.linspace(-float(margin), float(env.params.height) + float(margin), int(ny))
    pts = np.stack(np.meshgrid(xs, ys, indexing="xy"), axis=-1)      # [ny][nx][2] = (x, y)
    v = _host(env.velocity_at(pts.reshape(-1, 2), env=env_index)).reshape(len(ys), len(xs), 2)
    return xs, ys, v


def pose_grid(xs, ys, thetas, speed, device="cpu"):
    """The poses of a map, [len(thetas) * len(ys) * len(xs)][4] float64 = (x, y, theta, speed): theta is the slowest index, then y, then x."""
    xs, ys, thetas = (torch.as_tensor(np.asarray(v, dtype=np.float64), device=device) for v in (xs, ys, thetas))
    t, y, x = torch.meshgrid(thetas, ys, xs, indexing="ij")
    return torch.stack((x, y, t, torch.full_like(x, float(speed))), dim=-1).reshape(-1, 4)


def policy_map(policy, env, env_index, xs, ys, thetas, speed, chunk=65536, observe=None):
    """What `policy` does at every pose (x, y, theta) of the grid, for a robot placed there with forward speed `speed` in world `env_index`
    of `env` (its velocity is speed (cos theta, sin theta) + the current, as after a reset).

    `policy`: any callable obs [m][26] float32 -> dict of tensors with m rows each (`iqn_policy`, `dqn_policy`, `planner_policy` below).  It is called
    on chunks of at most `chunk` poses, in grid order.  `observe`: states [m][4] float64 -> (obs [m][26] float32, flags [m] uint8); default
    `env.observation_at(states, env=env_index, velocity="current", return_flags=True)` -- a stand-in makes the function run without a GPU.
    Returns a dict of arrays shaped [len(thetas)][len(ys)][len(xs)] + the trailing shape of the policy's rows, plus "flags" (the bits of
    observation_at: collision, outside, goal)."""
    if observe is None:
        observe = lambda st: env.observation_at(st, env=env_index, velocity="current", return_flags=True)
    device = env.device if env is not None and hasattr(env, "device") else "cpu"
    poses = pose_grid(xs, ys, thetas, speed, device)
    shape = (len(thetas), len(ys), len(xs))
    parts, flags = {}, []
    step = max(1, int(chunk))
    for lo in range(0, poses.shape[0], step):
        st = poses[lo:lo + step]
        obs, fl = observe(st)
        out = policy(obs)
        for k, v in out.items():
            if v.shape[0] != st.shape[0]:
                raise ValueError(f"policy output {k!r} has {v.shape[0]} rows for {st.shape[0]} poses")
            parts.setdefault(k, []).append(_host(v))
        flags.append(_host(fl))
    res = {k: np.concatenate(v).reshape(shape + v[0].shape[1:]) for k, v in parts.items()}
    res["flags"] = np.concatenate(flags).reshape(shape)
    return res


def action_fan(env, env_index, state, horizon, episode_timesteps=0):
    """Where each of the nine actions leads from `state` ([4] or [6]: x, y, theta, speed[, velocity]) in world `env_index`: nine open-loop rollouts
    of `horizon` steps, rollout a holding action a (`VecMarineNavEnv.constant_rollout_at`, one launch).  Returns a dict of arrays: `trajectory`
    [9][horizon * N][2] (the sub-step positions in order, NaN behind a rollout's end), `steps` [9], `state` [9][6], `done`, `info` [9], `reward`
    [9][horizon] (per step, undiscounted; 0 behind the end)."""
    st = np.asarray(state, dtype=np.float64).reshape(1, -1).repeat(9, axis=0)
    out = env.constant_rollout_at(st, np.arange(9, dtype=np.int32), int(horizon), env=env_index, episode_timesteps=int(episode_timesteps),
                                  trace=("traj", "reward"))
    traj = _host(out["traj_trace"])      # [H][9][N][2]
    return dict(trajectory=np.ascontiguousarray(traj.transpose(1, 0, 2, 3)).reshape(9, -1, 2), steps=_host(out["steps"]), state=_host(out["state"]),
                done=_host(out["done"]), info=_host(out["info"]), reward=np.ascontiguousarray(_host(out["reward_trace"]).T))


def lookahead_map(policy, env, env_index, xs, ys, thetas, speed, gamma=None, chunk=65536, observe=None, step=None):
    """A critic against the simulator at every pose of policy_map's grid (same order, same chunks): the one-step Bellman backup of each of the nine
    actions, backup[a] = r + gamma (1 - done) max Q(s', .), where (s', r, done) is the what-if step of the placed robot under action a
    (`VecMarineNavEnv.step_at`), beside the critic's own Q(s, .).

    `policy`: a map policy whose output has `q` [m][9] (`iqn_policy`, `dqn_policy(dqn, q=True)`); one without (the planners) is refused with
    ValueError.  Per chunk it is called once on the poses' observations and then once per action on the next observations, m rows each.
    `gamma`: default `env.discount`.  `observe` as in policy_map; `step`: (states [m][4] float64, actions [m] int32) -> dict with obs [m][26]
    float32, reward [m] float64, done [m], info [m]; default `env.step_at(states, actions, env=env_index)` -- stand-ins make the function run
    without a GPU.
    Returns arrays shaped [len(thetas)][len(ys)][len(xs)] + tail: `q` [9] (as the policy gives it), `action`, `backup` [9] float64, `residual` [9]
    = backup - q, `lookahead_action` = argmax backup (int32), `reward_next` [9] float64, `done_next` [9], `info_next` [9] uint8, `flags`."""
    if observe is None:
        observe = lambda st: env.observation_at(st, env=env_index, velocity="current", return_flags=True)
    if step is None:
        step = lambda st, a: env.step_at(st, a, env=env_index)
    if gamma is None:
        gamma = env.discount
    gamma = float(gamma)
    device = env.device if env is not None and hasattr(env, "device") else "cpu"
    poses = pose_grid(xs, ys, thetas, speed, device)
    shape = (len(thetas), len(ys), len(xs))
    parts = {k: [] for k in ("q", "action", "backup", "reward_next", "done_next", "info_next", "flags")}

    def q_of(out, m):
        if "q" not in out:
            raise ValueError("lookahead_map needs a policy whose output has 'q' [m][9] (a critic); this one gives " + str(sorted(out)))
        q = out["q"]
        if tuple(q.shape) != (m, 9):
            raise ValueError(f"policy output 'q' has shape {tuple(q.shape)} for {m} poses; expected ({m}, 9)")
        return q
    width = max(1, int(chunk))
    for lo in range(0, poses.shape[0], width):
        st = poses[lo:lo + width]
        m = st.shape[0]
        obs, fl = observe(st)
        out = policy(obs)
        parts["q"].append(_host(q_of(out, m)))
        parts["action"].append(_host(out["action"]).astype(np.int32))
        parts["flags"].append(_host(fl))
        backup, rew, done, info = (np.empty((m, 9), dtype=d) for d in (np.float64, np.float64, np.uint8, np.uint8))
        for a in range(9):
            nxt = step(st, torch.full((m,), a, dtype=torch.int32, device=st.device))
            qn = _host(q_of(policy(nxt["obs"]), m)).astype(np.float64)
            rew[:, a], done[:, a], info[:, a] = _host(nxt["reward"]), _host(nxt["done"]), _host(nxt["info"])
            backup[:, a] = rew[:, a] + gamma * (1.0 - done[:, a].astype(np.float64)) * qn.max(axis=1)
        parts["backup"].append(backup); parts["reward_next"].append(rew); parts["done_next"].append(done); parts["info_next"].append(info)
    res = {k: np.concatenate(v).reshape(shape + v[0].shape[1:]) for k, v in parts.items()}
    res["residual"] = res["backup"] - res["q"].astype(np.float64)
    res["lookahead_action"] = res["backup"].argmax(axis=-1).astype(np.int32)
    return res


def iqn_policy(agent, cvar=1.0, adaptive=False, quantiles=False):
    """An IQNAgent as a map policy: action [m], the CVaR level used `cvar` [m] (`adaptive`: agent.adjust_cvar_batch per row, else the constant), `q` [m][9]
    = mean over the 32 quantile samples and, with `quantiles`, `quantiles` [m][32][9] and `taus` [m][32].  It acts through adjust_cvar_batch and
    act_eval_batch, the calls of the capture loop of experiments.run_experiment, so the taus come from the agent's act stream: one draw per chunk."""
    def policy(obs):
        n = obs.shape[0]
        cv = agent.adjust_cvar_batch(obs) if adaptive else torch.full((n,), float(cvar), dtype=torch.float32, device=obs.device)
        a, qt, taus = agent.act_eval_batch(obs, 0.0, cv)
        out = dict(action=a, cvar=cv, q=qt.mean(dim=1))
        if quantiles:
            out["quantiles"] = qt
            out["taus"] = taus.reshape(n, -1)
        return out
    return policy


def dqn_policy(dqn, q=False):
    """A dqn.policy.DQNPolicy as a map policy: action [m] and, with `q`, its Q-values `q` [m][9] (what lookahead_map needs)."""
    if q:
        return lambda obs: dict(action=dqn.act_batch(obs), q=dqn.q_values(obs))
    return lambda obs: dict(action=dqn.act_batch(obs))


def planner_policy(kind, params):
    """The classical baselines ("APF" | "BA", planners.planner_act_batch: one HIP launch) as a map policy: action [m].  `params`: the env's
    parameters (`env.params`: the robot's acceleration / angular-velocity tables a, w)."""
    from .planners import planner_act_batch
    if kind not in ("APF", "BA"):
        raise ValueError(f"planner_policy: kind must be 'APF' or 'BA', got {kind!r}")
    a, w = [float(v) for v in params.a], [float(v) for v in params.w]
    return lambda obs: dict(action=planner_act_batch(obs, kind, a, w))


# ---- minimum-time-to-goal fields (VecMarineNavEnv.time_field, C-ABI mn_time_field) -------------------------------------------------------------------
# offset of stencil direction k, as include/marinenav_hip.h lists them
TIME_FIELD_DX = (1, 0, -1, 0, 1, -1, -1, 1, 2, 1, -1, -2, -2, -1, 1, 2)
TIME_FIELD_DY = (0, 1, 0, -1, 1, 1, -1, -1, 1, 2, 2, 1, -1, -2, -2, -1)
TIME_FIELD_NO_DIR = 255


def time_field(env, env_index, nx=128, ny=128, speed=None, clearance=0.0, goal=None, max_sweeps=None):
    """The minimum-time-to-goal field of world `env_index` on an nx x ny grid (`VecMarineNavEnv.time_field`: one launch).  Returns a dict of device
    tensors: `T` [ny][nx] float64 (seconds; +inf where the goal cannot be reached), `dir` [ny][nx] uint8 (the stencil direction of the first move,
    TIME_FIELD_DX / _DY; 255: none), `free` [ny][nx] bool (T finite: the cell is free and the goal reachable from it), `xs` [nx], `ys` [ny] (the
    cell centres), and `status`, `sweeps` (ints), `hx`, `hy` (floats: the cell size).  A status of _capi.TIME_FIELD_NOT_CONVERGED means max_sweeps
    (default 4 (nx + ny)) was too small: call again with more."""
    T, d, status, sweeps = env.time_field(int(env_index), nx, ny, speed=speed, clearance=clearance, max_sweeps=max_sweeps,
                                          goals=None if goal is None else torch.as_tensor(goal, dtype=torch.float64).reshape(1, 2))
    return field_dict(T[0], d[0], float(env.params.width), float(env.params.height), int(status[0]), int(sweeps[0]))


def field_dict(T, d, width, height, status=0, sweeps=0):
    """The dict of `time_field` from a field's tensors T, dir [ny][nx] (on any device) and the map's size."""
    ny, nx = T.shape
    hx, hy = float(width) / nx, float(height) / ny
    xs = (torch.arange(nx, dtype=torch.float64, device=T.device) + 0.5) * hx
    ys = (torch.arange(ny, dtype=torch.float64, device=T.device) + 0.5) * hy
    return dict(T=T, dir=d, free=torch.isfinite(T), xs=xs, ys=ys, status=status, sweeps=sweeps, hx=hx, hy=hy, width=float(width), height=float(height))


def _cells_of(field, xy):
    """(cell index [Q] int64, inside [Q] bool) of the points xy [Q][2]: cell (i, j) = (floor(x / hx), floor(y / hy)); a point on the map's far edge
    belongs to the last cell, a point outside the map (or NaN) to none (index 0, inside False)."""
    T = field["T"]
    ny, nx = T.shape
    if not torch.is_tensor(xy):
        xy = np.asarray(xy, dtype=np.float64)      # (a list would pass through float32)
    p = torch.as_tensor(xy).to(device=T.device, dtype=torch.float64).reshape(-1, 2)
    x, y = p[:, 0], p[:, 1]
    inside = (x >= 0.0) & (x <= nx * field["hx"]) & (y >= 0.0) & (y <= ny * field["hy"])
    i = torch.floor(torch.where(inside, x, torch.zeros_like(x)) / field["hx"]).long().clamp_(0, nx - 1)
    j = torch.floor(torch.where(inside, y, torch.zeros_like(y)) / field["hy"]).long().clamp_(0, ny - 1)
    return torch.where(inside, j * nx + i, torch.zeros_like(i)), inside


def time_at(field, xy):
    """T of the cell that contains each point of xy [Q][2]: float64 [Q] on the field's device, an exact lookup (no interpolation); NaN for a point
    outside the map."""
    c, inside = _cells_of(field, xy)
    t = field["T"].reshape(-1)[c]
    return torch.where(inside, t, torch.full_like(t, float("nan")))


def time_path(field, xy0):
    """The route the field gives from each start of xy0 [Q][2]: the centres of the cells that following `dir` visits, from the start's own cell to a
    source.  A bounded loop of torch gathers on the field's device, at most nx ny hops.  Returns (path [Q][L][2] float64, NaN behind each route's
    end; lengths [Q] int64, the points of each route): a start outside the map, in a blocked cell or in one the goal cannot be reached from has
    length 0, a start in a source cell length 1.  L is the longest route of the call."""
    T, d = field["T"], field["dir"]
    ny, nx = T.shape
    flat_t, flat_d = T.reshape(-1), d.reshape(-1).long()
    dx = torch.tensor(TIME_FIELD_DX + (0,), dtype=torch.int64, device=T.device)
    dy = torch.tensor(TIME_FIELD_DY + (0,), dtype=torch.int64, device=T.device)
    cur, inside = _cells_of(field, xy0)
    alive = inside & torch.isfinite(flat_t[cur])
    lengths = torch.zeros_like(cur)
    pts = []
    for _ in range(nx * ny):
        if not bool(alive.any()):
            break
        centre = torch.stack((field["xs"][cur % nx], field["ys"][cur // nx]), dim=-1)
        pts.append(torch.where(alive[:, None], centre, torch.full_like(centre, float("nan"))))
        lengths = lengths + alive.long()
        k = flat_d[cur]
        alive = alive & (k != TIME_FIELD_NO_DIR)
        k = torch.where(alive, k, torch.full_like(k, 16))
        cur = cur + dy[k] * nx + dx[k]
    path = torch.stack(pts, dim=1) if pts else torch.zeros(cur.shape[0], 0, 2, dtype=torch.float64, device=T.device)
    return path, lengths


def reference_times(env, envs=None, nx=128, ny=128, speed=None, clearance=0.0, max_sweeps=None):
    """The yardstick of an episode: T at each env's own start, on its own world's field (one launch for all of `envs`; default: every env).  float64
    [len(envs)] on the device; +inf where the start's cell is blocked on this grid or the goal cannot be reached from it.  A field that did not
    converge in max_sweeps raises RuntimeError."""
    from . import _capi
    idx = np.arange(env.n_envs, dtype=np.int32) if envs is None else np.asarray(_host(envs), dtype=np.int32).reshape(-1)
    worlds = env.get_worlds()
    starts = torch.as_tensor(np.array([worlds[int(e)]["start"] for e in idx], dtype=np.float64).reshape(-1, 2), device=env.device)
    T, _, status, _ = env.time_field(idx, nx, ny, speed=speed, clearance=clearance, max_sweeps=max_sweeps, want_dir=False, want_sweeps=False)
    if bool((status == _capi.TIME_FIELD_NOT_CONVERGED).any()):
        raise RuntimeError("reference_times: a field did not converge; raise max_sweeps")
    hx, hy = float(env.params.width) / int(nx), float(env.params.height) / int(ny)
    c, inside = _cells_of(dict(T=T[0], hx=hx, hy=hy), starts)      # (a field per start: time_at's lookup, row f in field f)
    t = T.reshape(len(idx), -1)[torch.arange(len(idx), device=T.device), c]
    return torch.where(inside, t, torch.full_like(t, float("nan")))


# ---- the field pilot (VecMarineNavEnv.pilot_act / rollout_pilot, C-ABI mn_pilot_act / mn_rollout_pilot) -------------------------------------------------
def time_interp(field, xy):
    """Tint of include/marinenav_hip.h ("Field pilot") at the points xy [Q][2], operation for operation: the bilinear value of T between the four
    cell centres around the point where all four are finite, else T of the containing cell (`_cells_of`); +inf outside the map and for a NaN.
    float64 [Q] on the field's device -- the words the pilot's kernels and tests/pilot_host.hip form."""
    T = field["T"]
    ny, nx = T.shape
    hx, hy = float(field["hx"]), float(field["hy"])
    width, height = float(field.get("width", nx * hx)), float(field.get("height", ny * hy))
    if not torch.is_tensor(xy):
        xy = np.asarray(xy, dtype=np.float64)
    p = torch.as_tensor(xy).to(device=T.device, dtype=torch.float64).reshape(-1, 2)
    x, y = p[:, 0], p[:, 1]
    inside = (x >= 0.0) & (x <= width) & (y >= 0.0) & (y <= height)
    xs, ys = torch.where(inside, x, torch.zeros_like(x)), torch.where(inside, y, torch.zeros_like(y))
    flat = T.reshape(-1)
    # (divisors as tensors on the field's device: a device tensor divided by a Python number is multiplied by its reciprocal, which is another word)
    hx, hy = torch.full((), hx, dtype=torch.float64, device=T.device), torch.full((), hy, dtype=torch.float64, device=T.device)
    i = torch.floor(xs / hx).long().clamp_(0, nx - 1)
    j = torch.floor(ys / hy).long().clamp_(0, ny - 1)
    v = flat[j * nx + i]
    if nx > 1 and ny > 1:
        u, w = xs / hx - 0.5, ys / hy - 0.5
        i0 = torch.floor(u).long().clamp_(0, nx - 2)
        j0 = torch.floor(w).long().clamp_(0, ny - 2)
        fx = (u - i0.to(torch.float64)).clamp_(0.0, 1.0)
        fy = (w - j0.to(torch.float64)).clamp_(0.0, 1.0)
        T00, T10, T01, T11 = flat[j0 * nx + i0], flat[j0 * nx + i0 + 1], flat[(j0 + 1) * nx + i0], flat[(j0 + 1) * nx + i0 + 1]
        ok = torch.isfinite(T00) & torch.isfinite(T10) & torch.isfinite(T01) & torch.isfinite(T11)
        z = torch.zeros_like(T00)
        a00, a10, a01, a11 = (torch.where(ok, t, z) for t in (T00, T10, T01, T11))
        bil = (a00 * (1.0 - fx) + a10 * fx) * (1.0 - fy) + (a01 * (1.0 - fx) + a11 * fx) * fy
        v = torch.where(ok, bil, v)
    inf = torch.full_like(v, float("inf"))
    return torch.where(inside & ~torch.isnan(v), v, inf)


def pilot_map(env, env_index, xs, ys, thetas, speed, field, horizon=2):
    """The field pilot's action and nine scores at every pose of policy_map's grid (same order), for a robot placed there with forward speed `speed`
    in world `env_index`; `field`: the dict of `time_field` for that world (or its T).  One launch (`VecMarineNavEnv.pilot_act`).  Returns arrays
    shaped [len(thetas)][len(ys)][len(xs)] + tail: `action` (int32; -1: poisoned), `scores` [9] float64, `steps` [9], `infos` [9], `flags`."""
    poses = pose_grid(xs, ys, thetas, speed, env.device)
    shape = (len(thetas), len(ys), len(xs))
    out = env.pilot_act(poses, field["T"] if isinstance(field, dict) else field, env=int(env_index), horizon=horizon,
                        want=("action", "scores", "steps", "infos", "flags"))
    return {k: _host(v).reshape(shape + tuple(v.shape[1:])) for k, v in out.items()}


def pilot_times(env, envs=None, nx=128, ny=128, horizon=2, clearance=0.0, n_steps=None, speed=None, max_sweeps=None):
    """The field pilot as a yardstick: solve the fields of the worlds `envs` (default: every env) and run their current episodes under the pilot --
    two launches (`time_field`, `rollout_pilot`).  An env outside `envs` is given no field and ends at once.  `n_steps`: default the parameters'
    max_episode_steps.  Returns a dict of device tensors over `envs`: `success` [E] bool (the episode reached the goal), `steps` [E] int64 (the
    steps it ran), `time` [E] float64 = steps * step_time, `T_start` [E] float64 (reference_times' lookup on the same fields) and `ratio` = time /
    T_start (NaN without success)."""
    from . import _capi
    n = env.n_envs
    idx = np.arange(n, dtype=np.int32) if envs is None else np.asarray(_host(envs), dtype=np.int32).reshape(-1)
    T, _, status, _ = env.time_field(idx, nx, ny, speed=speed, clearance=clearance, max_sweeps=max_sweeps, want_dir=False, want_sweeps=False)
    field_of_env = np.full(n, -1, dtype=np.int32)
    field_of_env[idx] = np.arange(len(idx), dtype=np.int32)
    steps_max = int(env.params.max_episode_steps) if n_steps is None else int(n_steps)
    tr = env.rollout_pilot(steps_max, T, field_of_env=field_of_env, horizon=horizon, trace=("done", "info"))
    if bool((status == _capi.TIME_FIELD_NOT_CONVERGED).any()):
        raise RuntimeError("pilot_times: a field did not converge; raise max_sweeps")
    sel = torch.as_tensor(idx.astype(np.int64), device=env.device)
    done, info = tr["done"][:, sel].bool(), tr["info"][:, sel]
    ended = done.any(dim=0)
    first = torch.where(ended, done.to(torch.uint8).argmax(dim=0), torch.full_like(sel, steps_max - 1))
    steps = torch.where(ended, first + 1, torch.full_like(sel, steps_max))
    success = ended & (info.gather(0, first[None, :])[0] == 4)      # MN_INFO_REACH_GOAL
    worlds = env.get_worlds()
    starts = torch.as_tensor(np.array([worlds[int(e)]["start"] for e in idx], dtype=np.float64).reshape(-1, 2), device=env.device)
    hx, hy = float(env.params.width) / int(nx), float(env.params.height) / int(ny)
    c, inside = _cells_of(dict(T=T[0], hx=hx, hy=hy), starts)
    t0 = T.reshape(len(idx), -1)[torch.arange(len(idx), device=T.device), c]
    t0 = torch.where(inside, t0, torch.full_like(t0, float("nan")))
    time = steps.to(torch.float64) * (float(env.params.N) * float(env.params.dt))
    ratio = torch.where(success, time / t0, torch.full_like(time, float("nan")))
    return dict(success=success, steps=steps, time=time, T_start=t0, ratio=ratio)
