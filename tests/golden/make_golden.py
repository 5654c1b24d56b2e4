#!/usr/bin/env python3
"""Generate the golden vectors under tests/golden/ by IMPORTING the Python reference.

Runs only in the build container (needs /root/reference).  Nothing here is used at
test/bench time: the tests read the emitted .npz/.json data files only.

The reference needs two shims to import under numpy 2.x without gym installed
(SURVEY.md Appendix B): a stub ``gym`` module and ``np.infty``.

Outputs (all small, committed):
  g1_reset.npz          world generation: seeds x world sizes x 3 consecutive resets
  g2_trace_*.npz        1000-step traces with caller-side reset on done
  g3_single_step.npz    2048 independent (world, state, action) -> step outputs
  g4_sonar_edge.npz     hand-built sonar/observation edge cases
  g5_velocity.npz       current-field samples (inside core, far field, 0/1-core worlds)
  g6_pretrained_replay.npz   stored action sequences of the reference's own evaluation
                        files + the reference's stored returns/success/time/energy
  eval_config_seed3.json     data file shipped by the reference (30 evaluation worlds)
  g7_iqn.npz            IQN forward / loss / grads with injected taus, adjust_cvar, linear_eps
  g8_boundary_trace.npz set_boundary = True, robot.N = 5 trace (run_experiments.py settings)
  g9_planners.npz       APF / BA baseline actions for 2304 observations
  pretrained_IQN_seed3/ checkpoint data files shipped by the reference (weights only)
  g12_replay.npz        the reference ReplayBuffer: 1500 adds into maxlen 1000, contents, one sample()
  g15_replay_nstep.npz  the reference ReplayBuffer with n_step = 3: 40 adds into maxlen 25, contents
  g13_learn_loop.npz    bookkeeping of the reference IQNAgent.learn loop over 400 timesteps on the reference env
  g14_iqn_episodes.npz  run_experiments.py's evaluation_IQN loop on the reference env + pretrained agent, injected taus:
                        per-step action / CVaR / quantiles / taus, per-episode outcome and trajectory
  g16_reset_params.npz  g1's recipe under the parameter sets of tests/params_sets.py (seeds 0-11 x 3 resets each): the 500-try limits
                        of the start / goal, core and obstacle loops, 60 x 36 and 36 x 60 maps, pose / start / goal from the parameters
  g17_step_params.npz   g3's recipe under other robot / sonar / reward / map parameters (5 sets x 256 steps) + stability flags
  g18_sonar_params_edge.npz  g4's layout at sonar.range 80 and 15: the snapped outermost beam, the range limit, several obstacles on one
                        beam; `obs_ld` = the same formulas in np.longdouble
  g19_planner_branches.npz   APF / BA actions on float32-exact rows, class by class (returns 0-11, still / crawl / slow / fast, returns
                        behind the robot, span edges, vertical / near-vertical / sloped walls near and far, two-return tangents, APF's d0,
                        extremes and near-cancellation, hand-written exact rows) under five (a, w) tables, with `stable` = the action
                        survives 8 copies of the row perturbed by 1e-9 relative
  g20_ladder_edges.npz  the case table of tests/ladder_edges.py (stationary robots on the termination ladder's thresholds, ties, coinciding rungs)
                        through MarineNavEnv.step; written without time stamps, so it regenerates byte for byte
  (g10 / g11: make_golden_dqn.py)
"""
import contextlib
import io
import json
import os
import shutil
import sys
import types
import warnings

import numpy as np

REF = "/root/reference"
OUT = os.path.dirname(os.path.abspath(__file__))

warnings.filterwarnings("ignore", category=PendingDeprecationWarning)
if not hasattr(np, "infty"):
    np.infty = np.inf


def _install_gym_stub():
    gym = types.ModuleType("gym")

    class Env:
        def close(self):
            pass

    class Discrete:
        def __init__(self, n):
            self.n = n

    class Box:
        def __init__(self, low, high, dtype=None):
            self.low, self.high, self.dtype = low, high, dtype

    spaces = types.ModuleType("gym.spaces")
    spaces.Discrete, spaces.Box = Discrete, Box
    envs = types.ModuleType("gym.envs")
    reg = types.ModuleType("gym.envs.registration")
    reg.register = lambda **kw: None
    envs.registration = reg
    gym.Env, gym.spaces, gym.envs = Env, spaces, envs
    sys.modules.update({"gym": gym, "gym.spaces": spaces, "gym.envs": envs,
                        "gym.envs.registration": reg})


_install_gym_stub()
sys.path.insert(0, REF)
from marinenav_env.envs.marinenav_env import MarineNavEnv, Core, Obstacle  # noqa: E402

INFO_CODE = {"normal": 0, "out of boundary": 1, "too long episode": 2, "collision": 3, "reach goal": 4}
MAXC, MAXO = 8, 10


def quiet(fn, *a, **kw):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **kw)


def world_arrays(env):
    c = np.zeros((MAXC, 4))
    o = np.zeros((MAXO, 3))
    for i, k in enumerate(env.cores):
        c[i] = [k.x, k.y, float(k.clockwise), k.Gamma]
    for i, k in enumerate(env.obstacles):
        o[i] = [k.x, k.y, k.r]
    return c, o, len(env.cores), len(env.obstacles)


def robot_state(env):
    r = env.robot
    return np.array([r.x, r.y, r.theta, r.speed, r.velocity[0], r.velocity[1]])


def peek_next_double(env):
    st = env.rd.get_state()
    v = env.rd.random_sample()
    env.rd.set_state(st)
    return v


WORLD_SIZES = [(4, 6, 30.0), (6, 8, 35.0), (8, 10, 40.0), (8, 5, 25.0)]


def g1_reset():
    rec = {k: [] for k in ("seed", "size", "start", "goal", "cores", "obs", "ncores", "nobs",
                           "theta0", "speed0", "obs0", "state0", "next_double")}
    for seed in (0, 1, 2, 3, 348):
        for (nc, no, md) in WORLD_SIZES:
            env = MarineNavEnv(seed=seed)
            env.num_cores, env.num_obs, env.min_start_goal_dis = nc, no, md
            for _ in range(3):
                ob = env.reset()
                c, o, n1, n2 = world_arrays(env)
                rec["seed"].append(seed)
                rec["size"].append([nc, no, md])
                rec["start"].append(env.start.copy())
                rec["goal"].append(env.goal.copy())
                rec["cores"].append(c)
                rec["obs"].append(o)
                rec["ncores"].append(n1)
                rec["nobs"].append(n2)
                rec["theta0"].append(env.robot.init_theta)
                rec["speed0"].append(env.robot.init_speed)
                rec["obs0"].append(ob)
                rec["state0"].append(robot_state(env))
                rec["next_double"].append(peek_next_double(env))
    np.savez_compressed(os.path.join(OUT, "g1_reset.npz"), **{k: np.array(v) for k, v in rec.items()})


def g1b_eval_worlds():
    """create_eval_configs semantics (train_IQN_model.py:123-148): seed 348, fixed start/goal."""
    env = MarineNavEnv(seed=348)
    env.obs_r_range = [1, 3]
    env.reset_start_and_goal = False
    env.start = np.array([5.0, 5.0])
    env.goal = np.array([45.0, 45.0])
    # the regenerated worlds are compared with eval_config_seed3.json by the tests
    shutil.copyfile(os.path.join(REF, "pretrained_models/IQN/seed_3/eval_config.json"),
                    os.path.join(OUT, "eval_config_seed3.json"))


def trace(seed, schedule, name, n_steps=1000, world=None):
    env = MarineNavEnv(seed=seed, schedule=schedule)
    if world is not None:
        env.num_cores, env.num_obs, env.min_start_goal_dis = world
    ar = np.random.RandomState(seed + 1000)
    actions = ar.randint(9, size=n_steps)
    obs0 = quiet(env.reset)
    rec = {k: [] for k in ("obs", "reward", "done", "info", "state", "ep_t", "tot_t", "reset_obs")}
    worlds = [world_arrays(env) + (env.start.copy(), env.goal.copy())]
    for t in range(n_steps):
        ob, r, d, info = env.step(int(actions[t]))
        rec["obs"].append(ob)
        rec["reward"].append(r)
        rec["done"].append(d)
        rec["info"].append(INFO_CODE[info["state"]])
        rec["state"].append(robot_state(env))
        rec["ep_t"].append(env.episode_timesteps)
        rec["tot_t"].append(env.total_timesteps)
        if d:
            ro = quiet(env.reset)
            rec["reset_obs"].append(ro)
            worlds.append(world_arrays(env) + (env.start.copy(), env.goal.copy()))
        else:
            rec["reset_obs"].append(np.zeros(26))
    out = {k: np.array(v) for k, v in rec.items()}
    out["actions"] = actions
    out["obs0"] = obs0
    out["seed"] = seed
    out["world_cores"] = np.array([w[0] for w in worlds])
    out["world_obs"] = np.array([w[1] for w in worlds])
    out["world_n"] = np.array([[w[2], w[3]] for w in worlds])
    out["world_start"] = np.array([w[4] for w in worlds])
    out["world_goal"] = np.array([w[5] for w in worlds])
    out["size"] = np.array([env.num_cores, env.num_obs, env.min_start_goal_dis])
    if schedule is not None:
        out["sched_timesteps"] = np.array(schedule["timesteps"])
        out["sched_num_cores"] = np.array(schedule["num_cores"])
        out["sched_num_obstacles"] = np.array(schedule["num_obstacles"])
        out["sched_min_dis"] = np.array(schedule["min_start_goal_dis"])
    np.savez_compressed(os.path.join(OUT, name), **out)


def g2_traces():
    trace(0, None, "g2_trace_seed0_default.npz")
    trace(1, None, "g2_trace_seed1_stage0.npz", world=(4, 6, 30.0))
    trace(2, None, "g2_trace_seed2_stage2.npz", world=(8, 10, 40.0))
    # a compressed curriculum so the schedule lookup changes inside the trace
    # (episodes of a random policy usually time out at step 1001, so resets land near 1001, 2002, 3003)
    sched = dict(timesteps=[0, 900, 2100], num_cores=[4, 6, 8], num_obstacles=[6, 8, 10],
                 min_start_goal_dis=[30.0, 35.0, 40.0])
    trace(5, sched, "g2_trace_seed5_schedule.npz", n_steps=3100)


def g8_boundary_trace():
    """run_experiments.py:192-211 style settings: set_boundary = True, robot.N = 5, fixed start/goal near
    the map edge so that 'out of boundary' terminations occur; caller-side reset on done."""
    env = MarineNavEnv(seed=21)
    env.set_boundary = True
    env.robot.N = 5
    env.reset_start_and_goal = False
    env.start = np.array([3.0, 4.0])
    env.goal = np.array([46.0, 45.0])
    env.num_cores, env.num_obs = 8, 8
    ar = np.random.RandomState(77)
    n_steps = 1500
    actions = ar.randint(9, size=n_steps)
    obs0 = env.reset()
    rec = {k: [] for k in ("obs", "reward", "done", "info", "state", "ep_t", "reset_obs")}
    for t in range(n_steps):
        ob, r, d, info = env.step(int(actions[t]))
        rec["obs"].append(ob); rec["reward"].append(r); rec["done"].append(d)
        rec["info"].append(INFO_CODE[info["state"]]); rec["state"].append(robot_state(env)); rec["ep_t"].append(env.episode_timesteps)
        rec["reset_obs"].append(env.reset() if d else np.zeros(26))
    out = {k: np.array(v) for k, v in rec.items()}
    out.update(actions=actions, obs0=obs0, seed=21, start=env.start, goal=env.goal)
    np.savez_compressed(os.path.join(OUT, "g8_boundary_trace.npz"), **out)


def g9_planners():
    """Classical baselines (APF.py:17-78, BA.py:14-155) on the 2048 observations of g3 plus synthetic
    corner cases: expected action indices."""
    import APF, BA
    z = np.load(os.path.join(OUT, "g3_single_step.npz"))
    obs = z["obs"].copy()
    rng = np.random.RandomState(99)
    extra = obs[rng.randint(len(obs), size=256)].copy()
    extra[:64, :2] *= 1e-4                      # near-zero velocity branches
    extra[64:128, 4:] = 0.0                     # no sonar returns
    for i in range(128, 192):                   # exactly one / two returns
        pts = extra[i, 4:].reshape(11, 2); keep = rng.choice(11, size=1 + (i % 2), replace=False)
        m = np.zeros(11, bool); m[keep] = True
        pts[~m] = 0.0
        pts[m] = rng.uniform(-8, 8, size=(m.sum(), 2))
    for i in range(192, 256):                   # vertical wall: same x for all returns
        pts = extra[i, 4:].reshape(11, 2); pts[:, 0] = rng.uniform(1, 8); pts[:, 1] = rng.uniform(-6, 6, size=11)
    obs = np.concatenate([obs, extra])
    env = MarineNavEnv(seed=0)
    apf = APF.APF_agent(env.robot.a, env.robot.w)
    ba = BA.BA_agent(env.robot.a, env.robot.w)
    a_apf = np.array([apf.act(o) for o in obs]); a_ba = np.array([ba.act(o) for o in obs])
    np.savez_compressed(os.path.join(OUT, "g9_planners.npz"), obs=obs, apf=a_apf, ba=a_ba, a=env.robot.a, w=env.robot.w)


# ---- g19: the planners branch by branch -------------------------------------------------------------------------------------------------
# (a, w) tables next to the robot's default: S1 of tests/params_sets.py; all-positive unsorted entries; no positive `a` (the mandated-
# acceleration rules meet an all-inf table); duplicated entries (exact ties of argmin / argmax that do not depend on the observation)
G19_TABLES = (("S1", (-0.6, 0.0, 0.5), (-0.7, 0.1, 0.4)),
              ("positive_unsorted", (0.3, 0.1, 0.2), (0.2, -0.5, 0.1)),
              ("no_positive_a", (-0.5, 0.0, -0.2), (0.4, -0.1, -0.6)),
              ("duplicates", (0.4, 0.4, -0.4), (0.5, 0.5, -0.5)))
# the hand-written rows: (velocity, goal, {beam slot: return}, why).  Every deciding quantity is exact in IEEE arithmetic on both sides
# (the comments use the default tables a = (-0.4, 0, 0.4), w = (-pi/6, 0, pi/6))
G19_EXACT = (
    ((1.0, 0.0), (-5.0, 0.0), {}, "speed == min_vel is not slow: APF a_proj = -0.5 keeps a[0]; BA: goal straight behind, diff = pi wraps to -pi"),
    ((1.0, 0.0), (6.0, 0.0), {5: (3.0, 0.0)}, "BA wall_follow at speed == min_vel: a = argmin |a|; a single return on the x axis: d = sqrt(10), dir = (-1, 3)"),
    ((0.0, 0.0), (3.0, 4.0), {}, "v = (0, 0): V_dir = (1, 0) in APF and in BA's move_to_goal; |goal| = 5 exactly"),
    ((0.0, 0.0), (0.0, 5.0), {8: (0.0, 3.0)}, "v = (0, 0) in wall_follow: dot = 0 does not flip dir = (-1, 0); diff = pi - 0 wraps to -pi; d = 1; mandated acceleration"),
    ((-1.0, 0.0), (-4.0, 0.0), {}, "goal straight ahead of v = (-1, +0): pi - pi = 0"),
    ((-1.0, 0.0), (-4.0, -0.0), {}, "goal (-4, -0) ahead of v = (-1, +0): -pi - pi = -2 pi wraps to 0 in one shift"),
    ((-1.0, -0.0), (-4.0, 0.0), {}, "goal (-4, +0) ahead of v = (-1, -0): pi + pi = 2 pi wraps to 0"),
    ((-1.0, 0.0), (4.0, 0.0), {}, "goal straight behind v = (-1, +0): 0 - pi = -pi is in range and stays"),
    ((-1.0, -0.0), (4.0, 0.0), {}, "goal straight behind v = (-1, -0): 0 + pi = pi is NOT in range (>=) and becomes -pi"),
    ((-2.0, 0.0), (4.0, 3.0), {}, "fast v = (-2, +0), goal off the axis, |goal| = 5"),
    ((-2.0, -0.0), (4.0, -3.0), {}, "fast v = (-2, -0), goal off the axis on the other side"),
    ((-1.0, 0.0), (0.0, 5.0), {9: (0.0, 3.0)}, "near wall (d = 1), dir = (-1, 0) along v: diff = pi - pi = 0 is not > 0: argmin(w)"),
    ((1.0, 0.0), (0.0, 5.0), {9: (0.0, 3.0)}, "the same wall against v: dir flips to (1, -0), diff = -0 - 0 is not > 0"),
    ((2.0, 0.0), (-2.0, 0.0), {}, "APF a_proj = -0.2 exactly: |a[0] - a_proj| == |a[1] - a_proj| (0.2 both), first index wins"),
    ((2.0, 0.0), (2.0, 0.0), {}, "APF a_proj = 0.2 exactly: a[1] and a[2] tie, first index wins"),
    ((0.5, 0.0), (2.0, 0.0), {}, "slow: the same a_proj = 0.2 with a <= 0 masked: a[2]"),
    ((0.5, 0.0), (-2.0, 0.0), {}, "slow, a_proj = -0.2: APF still mandates a[2]"),
    ((0.0, 0.0009765625), (0.0, 5.0), {}, "|v| = 2^-10 < 1e-3: standing still for both planners, V_angle = 0"),
    ((0.0, 0.001953125), (0.0, 5.0), {}, "|v| = 2^-9 > 1e-3: moving, V_angle = pi / 2"),
    ((0.0, 0.0009765625), (5.0, 0.0), {5: (3.0, 0.0)}, "|v| = 2^-10 in wall_follow: atan2(v) is used as it is (pi / 2), no stand-in"),
    ((1.0, 0.0), (8.0, 1.0), {2: (4.0, -1.0), 7: (4.0, 2.0)}, "two returns with equal x: dir = (0, 0), d = 0 / 0 is not < follow_dist, diff = 0 - 0"),
    ((0.0, 2.0), (8.0, 1.0), {2: (4.0, -1.0), 7: (4.0, 2.0)}, "the same (0, 0) tangent with v = (0, 2): diff = 0 - pi / 2"),
    ((0.0, 0.0), (8.0, 1.0), {2: (4.0, -1.0), 7: (4.0, 2.0)}, "the (0, 0) tangent standing still: diff = 0 - 0, mandated acceleration"),
    ((-1.0, 0.0), (8.0, 1.0), {2: (4.0, -1.0), 7: (4.0, 2.0)}, "the (0, 0) tangent with v = (-1, +0): dot = 0 does not flip, diff = 0 - pi = -pi stays"),
    ((-1.0, -0.0), (8.0, 1.0), {2: (4.0, -1.0), 7: (4.0, 2.0)}, "the (0, 0) tangent with v = (-1, -0): diff = 0 + pi = pi becomes -pi"),
    ((0.0, -2.0), (8.0, 1.0), {0: (4.0, -1.0), 1: (4.0, 2.0)}, "the (0, 0) tangent with v = (0, -2): diff = pi / 2; neighbouring beams"),
    ((0.5, 0.5), (8.0, 1.0), {2: (4.0, 2.0), 7: (4.0, -1.0)}, "the (0, 0) tangent, slow diagonal v: diff = -pi / 4, a_pos = the smallest positive a"),
    ((-0.5, 0.5), (8.0, 1.0), {2: (4.0, 2.0), 7: (4.0, -1.0)}, "the (0, 0) tangent, slow v at 135 degrees: diff = -3 pi / 4"),
    ((3.0, -3.0), (8.0, 1.0), {2: (4.0, 2.0), 7: (4.0, -1.0)}, "the (0, 0) tangent, fast v at -45 degrees: diff = pi / 4"),
    ((-3.0, -3.0), (8.0, 1.0), {2: (4.0, 2.0), 7: (4.0, -1.0)}, "the (0, 0) tangent, fast v at -135 degrees: diff = 3 pi / 4"),
    ((-1.0, 0.0), (7.0, 0.0), {3: (2.0, 1.0), 4: (5.0, -1.0)}, "two returns, v against dir = (3, 0): (-3, -0), atan2 = -pi, diff = -2 pi wraps to 0; d = 1"),
    ((1.0, 0.0), (7.0, 0.0), {3: (5.0, 1.0), 4: (2.0, -1.0)}, "two returns in falling x, v against dir = (-3, 0): (3, -0), atan2 = -0"),
    ((1.0, 0.0), (7.0, 0.0), {0: (2.0, 1.0), 10: (5.0, -1.0)}, "two returns with a gap of nine beams, v along dir = (3, 0): diff = 0"),
    ((0.0, 1.0), (6.0, 0.25), {1: (3.0, -2.0), 4: (3.0, 0.5), 9: (3.0, 2.0)}, "vertical wall x = 3 (det = 0 exactly), v along (0, 1): diff = 0, d = 3 < 5: argmin(w)"),
    ((0.0, -1.0), (6.0, 0.25), {1: (3.0, -2.0), 4: (3.0, 0.5), 9: (3.0, 2.0)}, "the same wall, v against: dir = (-0, -1), atan2 = -pi / 2 = atan2(v): diff = 0"),
    ((0.0, 2.0), (16.0, 0.5), {1: (8.0, -2.0), 4: (8.0, 0.5), 9: (8.0, 2.0)}, "vertical wall x = 8: d = 8 is not near: argmin |w - 0|"),
    ((1.0, 0.0), (0.0, 5.0), {5: (10.0, 0.0)}, "a return at d0 = 10 exactly: 1/d - 1/d0 = 0, no repulsion at all; F = (0, 250)"),
    ((1.0, 0.0), (-5.0, 0.0), {0: (-3.0, 0.0)}, "a return straight behind at (-3, +0): bearing pi, max + margin wraps"),
    ((1.0, 0.0), (-5.0, 0.0), {0: (-3.0, -0.0)}, "a return straight behind at (-3, -0): bearing -pi, min - margin wraps"),
    ((1.0, 0.0), (5.0, 0.0), {0: (-3.0, -0.0), 10: (-3.0, 0.0)}, "returns at bearing -pi and pi: both ends wrap, the goal ahead"),
)


def g19_planner_branches(n_copies=8, delta=1e-9):
    """APF.py / BA.py held against float32-exact rows, class by class and under five (a, w) tables: `act` = the reference's action
    for every (table, kind, row), `stable` = the row and `n_copies` copies of it -- every nonzero entry scaled by 1 + U(-delta, delta),
    zeros (misses) kept -- all get that action.  A host libm and the device's differ by a few float64 ulp in atan2, sqrt and the
    sums; a 1e-9 perturbation of the inputs runs through the same cancellations and dominates them by seven orders, so a row that
    survives it is one on which every faithful float64 evaluation must agree.  Classes are set by construction below."""
    import APF, BA
    deg = np.pi / 180.0
    margin = 10.0 * deg
    BEAM = np.linspace(-60.0, 60.0, 11) * deg
    KINDS = ("still", "crawl", "slow", "fast")
    rows, cls, names = [], [], []

    def add(name, vel, goal, pts):
        if name not in names:
            names.append(name)
        r = np.zeros(26)
        r[0:2], r[2:4], r[4:] = vel, goal, np.asarray(pts, dtype=np.float64).reshape(22)
        rows.append(r); cls.append(names.index(name))

    def polar(r, th):
        return np.array([r * np.cos(th), r * np.sin(th)])

    def vel(rng, kind, th=None):
        th = rng.uniform(-np.pi, np.pi) if th is None else th
        if kind == "still":
            return np.zeros(2)
        mag = {"crawl": 10.0 ** rng.uniform(-4.3, -2.5), "slow": rng.uniform(0.01, 0.99), "fast": rng.uniform(1.01, 3.0)}[kind]
        return polar(mag, th)

    def goal(rng, th=None):
        return polar(10.0 ** rng.uniform(-0.5, 1.5), rng.uniform(-np.pi, np.pi) if th is None else th)

    def place(rng, xy):      # the returns, in the order given, into random beam slots (gaps between them)
        xy = np.asarray(xy, dtype=np.float64).reshape(-1, 2)
        P = np.zeros((11, 2))
        P[np.sort(rng.choice(11, len(xy), replace=False))] = xy
        return P

    def beams(rng, k, rmin=0.3, rmax=20.0):      # k returns near their beams' bearings
        P = np.zeros((11, 2))
        for i in np.sort(rng.choice(11, k, replace=False)):
            P[i] = polar(rng.uniform(rmin, rmax), BEAM[i] + rng.uniform(-3.0, 3.0) * deg)
        return P

    def toward(rng, P, spread=8.0):      # a goal whose bearing lies near one of the returns' (inside the obstacle span), or anywhere if there is none
        v = P[(P != 0).any(axis=1)]
        if len(v) == 0:
            return goal(rng)
        p = v[rng.randint(len(v))]
        return goal(rng, np.arctan2(p[1], p[0]) + rng.uniform(-spread, spread) * deg)

    def centroid_goal(rng, P):      # a goal behind the wall, on the ray through the returns' centroid
        v = P[(P != 0).any(axis=1)]
        return v.mean(axis=0) * rng.uniform(1.2, 3.0)

    real = np.load(os.path.join(OUT, "g3_single_step.npz"))["obs"]
    for o in real:
        add("real", o[0:2], o[2:4], o[4:])

    rng = np.random.RandomState(1901)
    for k, count in ((0, 100), (1, 220), (2, 220), (3, 220)) + tuple((k, 50) for k in range(4, 12)):
        for i in range(count):
            P = beams(rng, k)
            add(f"returns_{k}", vel(rng, KINDS[i % 4]), toward(rng, P) if i % 8 < 6 else goal(rng), P)

    rng = np.random.RandomState(1902)
    for kind in KINDS:
        for i in range(120):
            P = beams(rng, rng.randint(0, 12))
            add(kind, vel(rng, kind), toward(rng, P) if i % 2 else goal(rng), P)

    rng = np.random.RandomState(1903)      # returns beyond +-120 degrees: left, right, both sides; goals inside and outside the span
    for i in range(240):
        k = rng.randint(1, 6)
        sign = (np.ones(k), -np.ones(k), rng.choice([-1.0, 1.0], size=k))[i % 3]
        P = place(rng, [polar(rng.uniform(0.5, 15.0), s * rng.uniform(120.0, 180.0) * deg) for s in sign])
        add("behind", vel(rng, KINDS[1 + i % 3]), toward(rng, P, 15.0) if i % 2 else goal(rng), P)

    rng = np.random.RandomState(1904)      # the goal's bearing against [min - margin, max + margin] and the +-60 degree clamps
    for i in range(320):
        mode, k = i % 8, rng.randint(1, 5)
        th = rng.uniform(-40.0, 40.0, size=k) * deg
        if mode == 4: th[0] = rng.uniform(50.5, 60.0) * deg            # hi clamps to pi
        if mode == 5: th[0] = -rng.uniform(50.5, 60.0) * deg           # lo clamps to -pi
        if mode == 6: th[0] = 50.0 * deg + rng.choice([-1.0, 1.0]) * 10.0 ** rng.uniform(-5.0, -2.0)      # hi on either side of the clamp
        if mode == 7: th[0] = -50.0 * deg - rng.choice([-1.0, 1.0]) * 10.0 ** rng.uniform(-5.0, -2.0)
        P = place(rng, [polar(rng.uniform(0.5, 15.0), t) for t in th]).astype(np.float32).astype(np.float64)
        ang = np.arctan2(P[:, 1], P[:, 0])[(P != 0).any(axis=1)]
        eps = 10.0 ** rng.uniform(-6.0, -1.5)
        gth = (ang.max() + margin - eps, ang.max() + margin + eps, ang.min() - margin + eps, ang.min() - margin - eps,
               rng.uniform(ang.max() + margin + 0.01, np.pi - 0.01), -rng.uniform(-(ang.min() - margin) + 0.01, np.pi - 0.01),
               rng.uniform(65.0, 175.0) * deg, -rng.uniform(65.0, 175.0) * deg)[mode]
        add("span", vel(rng, KINDS[1 + (i // 8) % 3]), goal(rng, gth), P)

    # walls of three and more returns; each with the fitted wall nearer and farther than follow_dist = 5 and the velocity along and against the tangent
    WALL_KINDS = ("slow", "fast", "fast", "crawl", "still", "fast", "slow", "fast")

    def wall_d(rng, i):
        return rng.uniform(0.5, 4.95) if i % 2 == 0 else (rng.uniform(5.05, 6.0) if i % 4 == 1 else rng.uniform(6.0, 15.0))

    def wall_vel(rng, i, tangent):
        along = (i // 2) % 2 == 0
        return vel(rng, WALL_KINDS[(i // 4) % 8], np.arctan2(tangent[1], tangent[0]) + (0.0 if along else np.pi) + rng.uniform(-60.0, 60.0) * deg)

    rng = np.random.RandomState(1905)
    for i in range(192):      # equal x
        k, x = rng.randint(3, 12), np.float64(np.float32(wall_d(rng, i)))
        P = place(rng, [(x, y) for y in rng.uniform(-6.0, 6.0, size=k)])
        add("wall_vertical", wall_vel(rng, i, (0.0, 1.0)), centroid_goal(rng, P), P)
    for i in range(288):      # x spread 10^U(-4, 0): s1 / s0 on both sides of 1e-3
        k, x, spread = rng.randint(3, 12), wall_d(rng, i), 10.0 ** rng.uniform(-4.0, 0.0)
        P = place(rng, [(x + spread * rng.uniform(-1.0, 1.0), y) for y in rng.uniform(-6.0, 6.0, size=k)])
        add("wall_near_vertical", wall_vel(rng, i, (0.0, 1.0)), centroid_goal(rng, P), P)
    for i in range(256):      # general: normal direction phi, foot of the perpendicular at distance d, returns along the tangent with a little noise
        k, d = rng.randint(3, 12), wall_d(rng, i)
        phi = rng.choice([-1.0, 1.0]) * rng.uniform(8.0, 100.0) * deg
        tangent = np.array([-np.sin(phi), np.cos(phi)])
        P = place(rng, [polar(d, phi) + t * tangent + rng.normal(0.0, 0.02, size=2) for t in rng.uniform(-6.0, 6.0, size=k)])
        add("wall_sloped", wall_vel(rng, i, tangent), centroid_goal(rng, P), P)

    rng = np.random.RandomState(1906)
    for i in range(80):      # two returns with equal x: the tangent is (0, 0)
        x = np.float64(np.float32(rng.uniform(0.5, 15.0)))
        P = place(rng, [(x, y) for y in rng.uniform(-6.0, 6.0, size=2)])
        add("two_same_x", vel(rng, KINDS[i % 4]), centroid_goal(rng, P), P)
    for i in range(120):      # two returns, velocity against (x1 - x0, 0): the flipped tangent is (-(x1 - x0), -0)
        x0, x1 = rng.uniform(0.5, 15.0, size=2)
        P = place(rng, [(x0, rng.uniform(-6.0, 6.0)), (x1, rng.uniform(-6.0, 6.0))])
        v = vel(rng, KINDS[1 + i % 3], (np.pi if x1 > x0 else 0.0) + rng.uniform(-80.0, 80.0) * deg)
        if i % 5 == 0:
            v[1] = 0.0
        add("two_flip", v, centroid_goal(rng, P), P)

    rng = np.random.RandomState(1907)      # APF: the sign of 1/d - 1/d0 (d0 = 10), the extremes of d and d_goal
    for name, rlo, rhi, glo, ghi in (("apf_inside_d0", 0.5, 9.5, None, None), ("apf_beyond_d0", 10.5, 20.0, None, None), ("apf_around_d0", 9.0, 11.0, None, None),
                                     ("apf_return_0.1", 0.1, 0.1, None, None), ("apf_goal_0.01", 0.3, 20.0, 0.01, 0.01), ("apf_goal_30", 0.3, 20.0, 30.0, 30.0)):
        for i in range(100):
            P = beams(rng, rng.randint(1, 7), rlo, rhi)
            g = toward(rng, P, 40.0) if i % 2 else goal(rng)
            if glo is not None:
                g = g / np.linalg.norm(g) * glo
            add(name, vel(rng, KINDS[i % 4]), g, P)
    for i in range(200):      # one return nearly on the way to the goal at the distance where repulsion is (1 + eps) x attraction
        dg, gth, eps = rng.uniform(1.0, 20.0), rng.uniform(-60.0, 60.0) * deg, rng.choice([-1.0, 1.0]) * 10.0 ** rng.uniform(-5.0, -1.0)
        lo, hi = 0.05, 10.0
        for _ in range(200):      # bisection: the repulsion falls monotonically with d on (0, d0)
            d = 0.5 * (lo + hi)
            inv = 1.0 / d - 0.1
            if 500.0 * inv * dg * dg / (d * d) + 500.0 * inv * inv * dg > 50.0 * dg * (1.0 + eps): lo = d
            else: hi = d
        P = place(rng, [polar(d, gth + rng.uniform(-0.02, 0.02))])
        add("apf_cancel", vel(rng, KINDS[i % 4]), polar(dg, gth), P)

    assert len(G19_EXACT) <= 64
    for v, g, pts, _why in G19_EXACT:
        P = np.zeros((11, 2))
        for slot, p in pts.items():
            P[slot] = p
        add("exact", v, g, P)

    obs = np.array(rows).astype(np.float32)      # what the kernel is handed; the reference gets the float64 value of the same numbers
    cls = np.array(cls, dtype=np.int16)
    n = len(obs)
    pts = obs[:, 4:].reshape(n, 11, 2)
    n_ret = ((pts[:, :, 0] != 0) | (pts[:, :, 1] != 0)).sum(axis=1)
    for k in range(12):      # (rounding made no return a miss)
        assert (n_ret[cls == names.index(f"returns_{k}")] == k).all()
    obs64 = obs.astype(np.float64)
    rng = np.random.RandomState(1999)
    copies = [obs64] + [obs64 * (1.0 + rng.uniform(-delta, delta, size=obs64.shape)) for _ in range(n_copies)]
    env = MarineNavEnv(seed=0)
    tables = [("default", env.robot.a, env.robot.w)] + list(G19_TABLES)
    T = len(tables)
    act = np.zeros((T, 2, n), dtype=np.int8)
    stable = np.zeros((T, 2, n), dtype=bool)
    with np.errstate(all="ignore"), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for ti, (_name, a, w) in enumerate(tables):
            agents = (APF.APF_agent(np.array(a, dtype=np.float64), np.array(w, dtype=np.float64)),
                      BA.BA_agent(np.array(a, dtype=np.float64), np.array(w, dtype=np.float64)))
            for ki, agent in enumerate(agents):
                got = np.array([[agent.act(o) for o in c] for c in copies])
                act[ti, ki] = got[0]
                stable[ti, ki] = (got == got[0]).all(axis=0)
    exact = cls == names.index("exact")
    unstable_counts = (~stable[:, :, ~exact]).sum(axis=2)
    class_stable_min = np.array([[[stable[ti, ki, cls == c].sum() for c in range(len(names))] for ki in range(2)] for ti in range(T)])
    print(f"  g19: {n} rows, {len(names)} classes; unstable per (table, kind) {unstable_counts.tolist()}; exact rows unstable "
          f"{(~stable[:, :, exact]).sum(axis=2).tolist()}; fewest stable rows of a class {class_stable_min[:, :, :-1].min()}")
    for c, name in enumerate(names):
        if (~stable[:, :, cls == c]).any():
            print(f"       {name}: {(cls == c).sum()} rows, unstable per (table, kind) {(~stable[:, :, cls == c]).sum(axis=2).tolist()}")
    assert (unstable_counts <= 0.01 * (~exact).sum()).all(), unstable_counts
    not_exact = [c for c in range(len(names)) if names[c] != "exact"]
    assert (class_stable_min[:, :, not_exact] >= 20).all(), class_stable_min
    path = os.path.join(OUT, "g19_planner_branches.npz")
    np.savez_compressed(path, obs=obs, cls=cls, cls_names=np.array(names), tables=np.array([[t[1], t[2]] for t in tables], dtype=np.float64),
                        table_names=np.array([t[0] for t in tables]), act=act, stable=stable, unstable_counts=unstable_counts,
                        exact_reasons=np.array([e[3] for e in G19_EXACT]), n_copies=n_copies, delta=delta)
    assert os.path.getsize(path) <= 400_000, os.path.getsize(path)


def g3_single_step(n_worlds=64, per_world=32):
    rng = np.random.RandomState(777)
    rec = {k: [] for k in ("cores", "obs_tab", "n", "start", "goal", "state_in", "action", "ep_t",
                           "obs", "reward", "done", "info", "state_out")}
    for wi in range(n_worlds):
        nc, no, md = WORLD_SIZES[wi % 4]
        if wi % 16 == 15:
            nc = 0            # no vortices
        if wi % 16 == 14:
            nc = 1            # scalar-idx KDTree path (marinenav_env.py:428-429)
        env = MarineNavEnv(seed=10_000 + wi)
        env.num_cores, env.num_obs, env.min_start_goal_dis = nc, no, md
        env.reset()
        c, o, n1, n2 = world_arrays(env)
        for j in range(per_world):
            # random state anywhere in the map; a third of them near an obstacle or the goal so
            # that collision / goal / sonar branches are exercised
            mode = j % 3
            if mode == 1 and n2 > 0:
                k = env.obstacles[rng.randint(n2)]
                ang = rng.uniform(0, 2 * np.pi)
                dist = k.r + rng.uniform(0.3, 6.0)
                x, y = k.x + dist * np.cos(ang), k.y + dist * np.sin(ang)
            elif mode == 2:
                ang = rng.uniform(0, 2 * np.pi)
                dist = rng.uniform(0.5, 6.0)
                x, y = env.goal[0] + dist * np.cos(ang), env.goal[1] + dist * np.sin(ang)
            else:
                x, y = rng.uniform(0, 50, size=2)
            theta = rng.uniform(0, 2 * np.pi)
            speed = rng.uniform(0, 2.0)
            a = int(rng.randint(9))
            ep_t = int(rng.choice([0, 5, 999, 1000]))
            env.robot.x, env.robot.y, env.robot.theta, env.robot.speed = float(x), float(y), float(theta), float(speed)
            env.robot.velocity = np.zeros(2)
            env.episode_timesteps = ep_t
            sin = np.array([x, y, theta, speed])
            ob, r, d, info = env.step(a)
            rec["cores"].append(c); rec["obs_tab"].append(o); rec["n"].append([n1, n2])
            rec["start"].append(env.start.copy()); rec["goal"].append(env.goal.copy())
            rec["state_in"].append(sin); rec["action"].append(a); rec["ep_t"].append(ep_t)
            rec["obs"].append(ob); rec["reward"].append(r); rec["done"].append(d)
            rec["info"].append(INFO_CODE[info["state"]]); rec["state_out"].append(robot_state(env))
    np.savez_compressed(os.path.join(OUT, "g3_single_step.npz"), **{k: np.array(v) for k, v in rec.items()})


def g4_sonar_edge():
    """Observation-only cases: world + robot pose -> get_observation()."""
    cases = []

    def add(name, obstacles, x, y, theta, goal=(45.0, 45.0), vel=(0.3, -0.2)):
        env = MarineNavEnv(seed=0)
        env.cores.clear()
        env.obstacles.clear()
        for (ox, oy, r) in obstacles:
            env.obstacles.append(Obstacle(ox, oy, r))
        env.goal = np.array(goal)
        env.robot.x, env.robot.y, env.robot.theta, env.robot.speed = x, y, theta, 1.0
        env.robot.velocity = np.array(vel)
        ob = env.get_observation()
        o = np.zeros((MAXO, 3))
        for i, ob_ in enumerate(obstacles):
            o[i] = ob_
        cases.append(dict(name=name, obs_tab=o, n_obs=len(obstacles), pose=[x, y, theta],
                          goal=list(goal), vel=list(vel), obs=ob))

    phi = (2 * np.pi / 3) / 10
    # beam i exactly vertical / within and outside the 1e-3 snap window
    for i in (0, 5, 10):
        rel = -np.pi / 3 + i * phi
        for vert in (np.pi / 2, 3 * np.pi / 2):
            for eps in (0.0, 5e-4, -9.9e-4, 1.5e-3, -1.01e-3):
                th = vert - rel + eps
                while th < 0:
                    th += 2 * np.pi
                while th >= 2 * np.pi:
                    th -= 2 * np.pi
                sign = 1.0 if vert < np.pi else -1.0
                add(f"vert_b{i}_{vert:.2f}_{eps}", [(20.0, 20.0 + sign * 6.0, 2.0), (21.5, 20.0 + sign * 4.0, 1.0)],
                    20.0, 20.0, th)
    # robot inside a circle (nearer wall behind -> no hit; nearer wall ahead -> hit)
    add("inside_behind", [(20.5, 20.0, 3.0)], 20.0, 20.0, np.pi)       # nearer wall is at -x side? heading -x
    add("inside_ahead", [(20.5, 20.0, 3.0)], 20.0, 20.0, 0.0)
    add("inside_center_off", [(20.0, 21.0, 2.5)], 20.0, 20.0, np.pi / 2 - 0.2)
    # break-quirk: list order matters (near obstacle listed after a far one and vice versa)
    near, far, mid = (24.0, 20.0, 1.0), (28.0, 20.0, 2.0), (26.0, 20.3, 0.8)
    for order_name, order in (("nfm", [near, far, mid]), ("fnm", [far, near, mid]), ("fmn", [far, mid, near]),
                              ("mfn", [mid, far, near]), ("nmf", [near, mid, far]), ("mnf", [mid, near, far])):
        add("break_" + order_name, order, 20.0, 20.0, 0.0)
        add("break2_" + order_name, order, 20.0, 20.0, 0.15)
    # tangent / range boundary
    add("tangent", [(25.0, 21.0, 1.0)], 20.0, 20.0, 0.0)
    add("tangent_eps_in", [(25.0, 20.999999, 1.0)], 20.0, 20.0, 0.0)
    add("tangent_eps_out", [(25.0, 21.000001, 1.0)], 20.0, 20.0, 0.0)
    add("range_in", [(31.0, 20.0, 1.0000001)], 20.0, 20.0, 0.0)
    add("range_out", [(31.0, 20.0, 0.9999999)], 20.0, 20.0, 0.0)
    add("behind", [(15.0, 20.0, 1.0)], 20.0, 20.0, 0.0)
    add("no_obstacles", [], 20.0, 20.0, 1.0)
    add("ten_obstacles", [(22.0 + 1.7 * i, 20.0 + (-1) ** i * (1.0 + 0.3 * i), 0.9) for i in range(10)], 20.0, 20.0, 0.05)
    # wide theta sweep through a fixed obstacle field
    field = [(25.0, 25.0, 2.0), (18.0, 27.0, 1.5), (24.0, 16.0, 2.5), (14.0, 17.0, 1.2), (20.0, 29.5, 1.1)]
    for k in range(64):
        add(f"sweep_{k}", field, 20.0, 21.0, 2 * np.pi * k / 64.0)
    np.savez_compressed(
        os.path.join(OUT, "g4_sonar_edge.npz"),
        names=np.array([c["name"] for c in cases]),
        obs_tab=np.array([c["obs_tab"] for c in cases]),
        n_obs=np.array([c["n_obs"] for c in cases]),
        pose=np.array([c["pose"] for c in cases]),
        goal=np.array([c["goal"] for c in cases]),
        vel=np.array([c["vel"] for c in cases]),
        obs=np.array([c["obs"] for c in cases]),
    )


def g5_velocity():
    rng = np.random.RandomState(55)
    recs = {k: [] for k in ("cores", "n", "xy", "v")}
    for wi, nc in enumerate((8, 8, 4, 6, 1, 0, 2, 3)):
        env = MarineNavEnv(seed=500 + wi)
        env.num_cores, env.num_obs = nc, 0
        env.reset()
        c, _, n1, _ = world_arrays(env)
        pts = [rng.uniform(0, 50, size=2) for _ in range(40)]
        for k in env.cores:      # inside the core (d <= r) and just outside
            for rad in (0.05, 0.3, 0.4999, 0.5, 0.5001, 0.8):
                ang = rng.uniform(0, 2 * np.pi)
                pts.append(np.array([k.x + rad * np.cos(ang), k.y + rad * np.sin(ang)]))
        for p in pts:
            v = env.get_velocity(float(p[0]), float(p[1]))
            recs["cores"].append(c); recs["n"].append(n1); recs["xy"].append(p); recs["v"].append(v)
    np.savez_compressed(os.path.join(OUT, "g5_velocity.npz"), **{k: np.array(v) for k, v in recs.items()})


def g6_pretrained_replay():
    d = os.path.join(REF, "pretrained_models/IQN/seed_3")
    with open(os.path.join(d, "eval_config.json")) as f:
        cfg = json.load(f)
    out = {}
    for pol in ("greedy", "adaptive"):
        z = np.load(os.path.join(d, f"{pol}_evaluations.npz"), allow_pickle=True)
        evals = [0, 150, 299]
        envs = [0, 7, 13, 19, 24, 29]
        acts, lens, rews, succ, times, ener, ids = [], [], [], [], [], [], []
        for e in evals:
            for k in envs:
                a = np.asarray(z["actions"][e][k], dtype=np.int32)
                pad = np.full(1000, -1, dtype=np.int32)
                pad[: len(a)] = a
                acts.append(pad); lens.append(len(a))
                rews.append(float(z["rewards"][e][k])); succ.append(bool(z["successes"][e][k]))
                times.append(float(z["times"][e][k])); ener.append(float(z["energies"][e][k]))
                ids.append([e, k])
        out[f"{pol}_actions"] = np.array(acts); out[f"{pol}_len"] = np.array(lens)
        out[f"{pol}_reward"] = np.array(rews); out[f"{pol}_success"] = np.array(succ)
        out[f"{pol}_time"] = np.array(times); out[f"{pol}_energy"] = np.array(ener)
        out[f"{pol}_ids"] = np.array(ids)
        out[f"{pol}_timesteps_head"] = np.asarray(z["timesteps"][:3])
    np.savez_compressed(os.path.join(OUT, "g6_pretrained_replay.npz"), **out)
    # checkpoint data files (weights + constructor json) shipped by the reference
    pd = os.path.join(OUT, "pretrained_IQN_seed3")
    os.makedirs(pd, exist_ok=True)
    for fn in ("network_params.pth", "constructor_params.json"):
        shutil.copyfile(os.path.join(d, fn), os.path.join(pd, fn))
        os.chmod(os.path.join(pd, fn), 0o644)
    os.chmod(os.path.join(OUT, "eval_config_seed3.json"), 0o644)


def g7_iqn():
    import torch
    th = types.ModuleType("thirdparty"); th.__path__ = [os.path.join(REF, "thirdparty")]
    iq = types.ModuleType("thirdparty.IQN"); iq.__path__ = [os.path.join(REF, "thirdparty/IQN")]
    sys.modules["thirdparty"] = th; sys.modules["thirdparty.IQN"] = iq
    from thirdparty.IQN.agent import IQNAgent, calculate_huber_loss
    from thirdparty.IQN.model import ObsEncoder

    out = {}
    net = ObsEncoder(26, 9, seed=7)
    for k, v in net.state_dict().items():
        out["sd_" + k] = v.numpy().copy()
    # seeded-init parity: two nets with the same seed are identical
    rng = np.random.RandomState(9)
    obs = rng.normal(0, 5, size=(16, 26)).astype(np.float32)
    obs[:, 4:][rng.uniform(size=(16, 22)) < 0.5] = 0.0
    taus32 = rng.uniform(size=(16, 32)).astype(np.float32)
    taus8a = rng.uniform(size=(16, 8)).astype(np.float32)
    taus8b = rng.uniform(size=(16, 8)).astype(np.float32)

    inject = []
    real_rand = torch.rand

    def fake_rand(*shape, **kw):
        t = inject.pop(0)
        assert tuple(t.shape) == tuple(shape), (t.shape, shape)
        return torch.from_numpy(t.copy())

    torch.rand = fake_rand
    try:
        for cvar in (1.0, 0.5):
            inject.append(taus32)
            with torch.no_grad():
                q, t = net.forward(torch.from_numpy(obs), 32, cvar)
            out[f"fwd_quantiles_cvar{cvar}"] = q.numpy(); out[f"fwd_taus_cvar{cvar}"] = t.numpy()
            out[f"qvals_cvar{cvar}"] = q.mean(dim=1).numpy()
        # one train() step through the reference agent (B=16) with injected taus
        agent = IQNAgent(26, 9, BATCH_SIZE=16, seed=7)
        nxt = rng.normal(0, 5, size=(16, 26)).astype(np.float32)
        act = rng.randint(9, size=(16, 1)).astype(np.int64)
        rew = rng.normal(0, 3, size=(16, 1)).astype(np.float32)
        don = (rng.uniform(size=(16, 1)) < 0.25).astype(np.float32)
        # perturb the target net so the TD error is not trivially symmetric
        with torch.no_grad():
            for p in agent.qnetwork_target.parameters():
                p.add_(0.01 * torch.from_numpy(rng.normal(size=tuple(p.shape)).astype(np.float32)))
        for k, v in agent.qnetwork_target.state_dict().items():
            out["tgt_" + k] = v.numpy().copy()
        before = {k: v.numpy().copy() for k, v in agent.qnetwork_local.state_dict().items()}
        inject.extend([taus8a, taus8b])   # target forward draws first, then local (agent.py:279,285)
        exp = tuple(torch.from_numpy(x) for x in (obs, act, rew, nxt, don))
        loss = agent.train(exp)
        out["train_loss"] = np.array(loss)
        for (k, p) in agent.qnetwork_local.named_parameters():
            out["grad_" + k] = p.grad.numpy().copy()     # clipped in place by clip_grad_norm_
        for k, v in agent.qnetwork_local.state_dict().items():
            out["after_" + k] = v.numpy().copy()
            assert np.array_equal(before[k], out["sd_" + k])
    finally:
        torch.rand = real_rand
    out.update(obs=obs, taus32=taus32, taus8_target=taus8a, taus8_local=taus8b, next_obs=nxt,
               actions=act, rewards=rew, dones=don)
    # huber
    td = torch.from_numpy(rng.normal(0, 2, size=(4, 8, 8)).astype(np.float32))
    out["huber_in"] = td.numpy(); out["huber_out"] = calculate_huber_loss(td, 1.0).numpy()
    # adjust_cvar / linear_eps / energy cost tables
    ag = IQNAgent(26, 9, seed=0)
    states = rng.normal(0, 4, size=(32, 26))
    states[:8, 4:] = 0.0
    states[8:16, 4:] *= 0.0002
    out["cvar_states"] = states
    out["cvar_values"] = np.array([ag.adjust_cvar(s) for s in states])
    eps = []
    for t in (0, 1, 1000, 299_999, 300_000, 300_001, 3_000_000):
        ag.current_timestep = t
        eps.append(ag.linear_eps(3_000_000))
    out["eps_t"] = np.array([0, 1, 1000, 299_999, 300_000, 300_001, 3_000_000]); out["eps_v"] = np.array(eps)
    env = MarineNavEnv(seed=0)
    out["energy_cost"] = np.array([env.robot.compute_action_energy_cost(a) for a in range(9)])
    out["action_table"] = np.array(env.robot.actions)
    # pretrained net on the fixed obs with injected taus
    pre = ObsEncoder.load(os.path.join(REF, "pretrained_models/IQN/seed_3"))
    torch.rand = fake_rand
    try:
        inject.append(taus32)
        with torch.no_grad():
            q, _ = pre.forward(torch.from_numpy(obs), 32, 1.0)
        out["pretrained_quantiles"] = q.numpy()
    finally:
        torch.rand = real_rand
    np.savez_compressed(os.path.join(OUT, "g7_iqn.npz"), **out)


def _import_iqn():
    th = types.ModuleType("thirdparty"); th.__path__ = [os.path.join(REF, "thirdparty")]
    iq = types.ModuleType("thirdparty.IQN"); iq.__path__ = [os.path.join(REF, "thirdparty/IQN")]
    sys.modules["thirdparty"] = th; sys.modules["thirdparty.IQN"] = iq
    from thirdparty.IQN.agent import IQNAgent
    from thirdparty.IQN.replay_buffer import ReplayBuffer
    return IQNAgent, ReplayBuffer


def g12_replay():
    """The reference's ReplayBuffer (thirdparty/IQN/replay_buffer.py:6-59): 1500 adds into maxlen 1000, the deque
    contents afterwards (oldest -> newest), and what sample() returns (shapes, dtypes, which rows)."""
    _, ReplayBuffer = _import_iqn()
    rng = np.random.RandomState(12)
    n, cap, B = 1500, 1000, 32
    states = rng.normal(0, 5, size=(n, 26))
    nexts = rng.normal(0, 5, size=(n, 26))
    actions = rng.randint(9, size=n)
    rewards = rng.normal(0, 3, size=n)
    dones = rng.uniform(size=n) < 0.2
    buf = ReplayBuffer(cap, B, "cpu", seed=5, gamma=0.99)
    sizes = []
    for i in range(n):
        buf.add(states[i], int(actions[i]), float(rewards[i]), nexts[i], bool(dones[i]))
        sizes.append(len(buf))
    mem = list(buf.memory)
    out = dict(in_states=states, in_next=nexts, in_actions=actions, in_rewards=rewards, in_dones=dones,
               capacity=np.array(cap), batch=np.array(B), sizes=np.array(sizes),
               mem_states=np.stack([e.state for e in mem]), mem_next=np.stack([e.next_state for e in mem]),
               mem_actions=np.array([e.action for e in mem]), mem_rewards=np.array([e.reward for e in mem]),
               mem_dones=np.array([e.done for e in mem]))
    s, a, r, ns, d = buf.sample()
    out.update(sample_states=s.numpy(), sample_actions=a.numpy(), sample_rewards=r.numpy(), sample_next=ns.numpy(),
               sample_dones=d.numpy())
    for k in ("sample_states", "sample_actions", "sample_rewards", "sample_next", "sample_dones"):
        out[k + "_dtype"] = np.array(str(out[k].dtype))
    np.savez_compressed(os.path.join(OUT, "g12_replay.npz"), **out)


def g15_replay_nstep():
    """The reference's ReplayBuffer with n_step = 3 (replay_buffer.py:26-41): 40 adds into maxlen 25 -- the sliding window does not
    restart at `done` -- and the deque afterwards."""
    _, ReplayBuffer = _import_iqn()
    rng = np.random.RandomState(15)
    n_in, cap, n_step, gamma = 40, 25, 3, 0.97
    S = rng.normal(size=(n_in, 26)); NS = rng.normal(size=(n_in, 26))
    A = rng.randint(9, size=n_in); R = rng.normal(size=n_in); D = rng.uniform(size=n_in) < 0.2
    buf = ReplayBuffer(cap, 8, "cpu", seed=5, gamma=gamma, n_step=n_step)
    sizes = []
    for i in range(n_in):
        buf.add(S[i], int(A[i]), float(R[i]), NS[i], bool(D[i]))
        sizes.append(len(buf))
    mem = list(buf.memory)
    np.savez_compressed(os.path.join(OUT, "g15_replay_nstep.npz"), capacity=cap, n_step=n_step, gamma=gamma,
                        in_states=S, in_actions=A, in_rewards=R, in_next=NS, in_dones=D, sizes=np.array(sizes),
                        mem_states=np.stack([e.state for e in mem]), mem_actions=np.array([e.action for e in mem]),
                        mem_rewards=np.array([e.reward for e in mem]), mem_next=np.stack([e.next_state for e in mem]),
                        mem_dones=np.array([e.done for e in mem]))


def g13_learn_loop():
    """The reference's IQNAgent.learn (thirdparty/IQN/agent.py:94-173) run on the reference env for 400 timesteps:
    the trajectory-independent bookkeeping of the loop -- counters, at which learning steps train() / soft_update() /
    evaluation() fire, what the evaluation npz records -- for the drop-in loop to reproduce."""
    import tempfile
    import torch
    IQNAgent, _ = _import_iqn()
    cfg = dict(total_timesteps=400, learning_starts=100, eval_freq=150, target_update_interval=64, UPDATE_EVERY=4,
               BATCH_SIZE=32, BUFFER_SIZE=1000, seed=3, env_seed=11)
    torch.manual_seed(0)
    agent = IQNAgent(26, 9, BATCH_SIZE=cfg["BATCH_SIZE"], BUFFER_SIZE=cfg["BUFFER_SIZE"], UPDATE_EVERY=cfg["UPDATE_EVERY"],
                     learning_starts=cfg["learning_starts"], target_update_interval=cfg["target_update_interval"],
                     seed=cfg["seed"])
    train_env = MarineNavEnv(seed=cfg["env_seed"])
    eval_env = MarineNavEnv(seed=348)
    eval_env.reset_start_and_goal = False
    eval_env.start = np.array([5.0, 5.0]); eval_env.goal = np.array([45.0, 45.0])
    eval_config = {}
    for i, (nc, no) in enumerate(((4, 6), (8, 10))):
        eval_env.num_cores, eval_env.num_obs = nc, no
        quiet(eval_env.reset)
        eval_config[f"env_{i}"] = eval_env.episode_data()
    log = dict(train_at=[], train_mem=[], sync_at=[], eval_at=[], eval_ts=[], resets=0)
    real_train, real_sync, real_eval, real_reset = agent.train, agent.soft_update, agent.evaluation, train_env.reset

    def train(exp):
        log["train_at"].append(agent.learning_timestep); log["train_mem"].append(len(agent.memory))
        return real_train(exp)

    def sync(a, b):
        log["sync_at"].append(agent.learning_timestep)
        return real_sync(a, b)

    def evaluation(env, eval_config, greedy=True, eval_log_path=None):
        log["eval_at"].append((agent.learning_timestep, int(greedy))); log["eval_ts"].append(agent.current_timestep)
        return real_eval(env, eval_config=eval_config, greedy=greedy, eval_log_path=eval_log_path)

    def reset():
        log["resets"] += 1
        return real_reset()

    agent.train, agent.soft_update, agent.evaluation, train_env.reset = train, sync, evaluation, reset
    # third numpy-2 shim: agent.py:390 hands np.savez ragged python lists (per-episode action sequences), which numpy < 1.24
    # turned into object arrays silently and numpy 2 refuses
    real_savez = np.savez

    def savez(file, **kw):
        fixed = {}
        for k, v in kw.items():
            try:
                fixed[k] = np.asanyarray(v)
            except ValueError:
                fixed[k] = np.array(v, dtype=object)
        return real_savez(file, **fixed)

    np.savez = savez
    with tempfile.TemporaryDirectory() as tmp:
        quiet(agent.learn, total_timesteps=cfg["total_timesteps"], train_env=train_env, eval_env=eval_env,
              eval_config=eval_config, eval_freq=cfg["eval_freq"], eval_log_path=tmp, verbose=False)
        files = sorted(os.listdir(tmp))
        zg = np.load(os.path.join(tmp, "greedy_evaluations.npz"), allow_pickle=True)
        za = np.load(os.path.join(tmp, "adaptive_evaluations.npz"), allow_pickle=True)
        out = dict(npz_keys=np.array(sorted(zg.files)), greedy_timesteps=zg["timesteps"], adaptive_timesteps=za["timesteps"],
                   greedy_rewards_shape=np.array(zg["rewards"].shape), greedy_successes_shape=np.array(zg["successes"].shape))
    np.savez = real_savez
    out.update(files=np.array(files), current_timestep=np.array(agent.current_timestep),
               learning_timestep=np.array(agent.learning_timestep), train_at=np.array(log["train_at"]),
               train_mem=np.array(log["train_mem"]), sync_at=np.array(log["sync_at"]), eval_at=np.array(log["eval_at"]),
               eval_ts=np.array(log["eval_ts"]), memory_len=np.array(len(agent.memory)),
               env_total_timesteps=np.array(train_env.total_timesteps), train_resets=np.array(log["resets"]),
               eval_config=np.array(json.dumps(eval_config)), cfg=np.array(json.dumps(cfg)))
    np.savez_compressed(os.path.join(OUT, "g13_learn_loop.npz"), **out)


def g14_iqn_episodes():
    """run_experiments.py's evaluation_IQN loop (:19-72) restated around the reference's own env and agent
    (act_eval / act_adaptive_eval, pretrained seed_3 checkpoint) under exp_setup_5 (:192-211), with the taus of every
    act call injected from a seeded stream: per step the action, CVaR level, quantiles [1,32,9], taus [1,32,1]; per
    episode the outcome and episode_data()."""
    import torch
    IQNAgent, _ = _import_iqn()
    agent = IQNAgent(26, 9, seed=2)
    agent.load_model(os.path.join(REF, "pretrained_models/IQN/seed_3"), "cpu")
    real_rand = torch.rand
    out = {}
    for name, adaptive, cvar in (("adaptive", True, None), ("cvar0.5", False, 0.5), ("cvar1.0", False, 1.0)):
        env = MarineNavEnv(seed=15)
        env.reset_start_and_goal = False; env.random_reset_state = False; env.set_boundary = True
        env.obs_r_range = [1, 3]; env.start = np.array([5.0, 5.0]); env.goal = np.array([45.0, 45.0])
        env.robot.N = 5; env.num_cores, env.num_obs = 6, 8
        rng = np.random.RandomState(77)
        obs = env.reset()
        if name == "adaptive":
            c, o, n1, n2 = world_arrays(env)
            out.update(world_cores=c[:n1], world_obs=o[:n2], obs0=obs)
        rec = dict(actions=[], cvars=[], quantiles=[], taus=[], taus_in=[], obs=[])
        length, done, ret, energy = 0, False, 0.0, 0.0
        while not done and length < 1000:
            t_in = rng.uniform(size=(1, 32)).astype(np.float32)
            torch.rand = lambda *shape, **kw: torch.from_numpy(t_in.copy())
            try:
                if adaptive:
                    (action, quantiles, taus), cv = agent.act_adaptive_eval(obs)
                else:
                    action, quantiles, taus = agent.act_eval(obs, cvar=cvar)
                    cv = cvar
            finally:
                torch.rand = real_rand
            rec["obs"].append(obs); rec["taus_in"].append(t_in[0]); rec["actions"].append(int(action)); rec["cvars"].append(cv)
            rec["quantiles"].append(quantiles); rec["taus"].append(taus)
            obs, reward, done, info = env.step(int(action))
            ret += env.discount ** length * reward
            length += 1
            energy += env.robot.compute_action_energy_cost(int(action))
        ep = env.episode_data()
        for k, v in rec.items():
            out[f"{name}_{k}"] = np.array(v)
        out[f"{name}_success"] = np.array(info["state"] == "reach goal"); out[f"{name}_out_of_area"] = np.array(info["state"] == "out of boundary")
        out[f"{name}_time"] = np.array(env.robot.dt * env.robot.N * length); out[f"{name}_energy"] = np.array(energy)
        out[f"{name}_return"] = np.array(ret)
        out[f"{name}_trajectory"] = np.array(ep["robot"]["trajectory"])
        out[f"{name}_ep_keys"] = np.array(json.dumps({"env": sorted(ep["env"].keys()), "robot": sorted(ep["robot"].keys())}))
    np.savez_compressed(os.path.join(OUT, "g14_iqn_episodes.npz"), **out)


# ---- g16 / g17 / g18: the env parameters away from their defaults ---------------------------------------------------------
sys.path.insert(0, os.path.dirname(OUT))
import params_sets as PS  # noqa: E402      (tests/params_sets.py: the sets, by mn_params field name)

_ENV_ATTR = {"core_r": "r"}                                     # mn_params field -> MarineNavEnv attribute where the names differ
_ROBOT_ATTR = {"dt": "dt", "N": "N", "max_speed": "max_speed", "robot_r": "r"}
_SONAR_ATTR = {"sonar_range": "range", "sonar_angle": "angle"}
_BOOLS = ("reset_start_and_goal", "random_reset_state", "set_boundary")


def apply_set(env, spec):
    """The attribute writes a set stands for (what reset_with_eval_config does from a file, marinenav_env.py:467-555), followed by
    the recomputations it calls (:532-533, :541-542)."""
    for k, v in spec.items():
        if k in ("a", "w"):
            setattr(env.robot, k, np.array(v, dtype=float))
        elif k in _ROBOT_ATTR:
            setattr(env.robot, _ROBOT_ATTR[k], v)
        elif k in _SONAR_ATTR:
            setattr(env.robot.sonar, _SONAR_ATTR[k], v)
        elif k in ("start", "goal"):
            setattr(env, k, np.array(v, dtype=float))
        elif k in ("v_range", "obs_r_range"):
            setattr(env, k, list(v))
        elif k in _BOOLS:
            setattr(env, k, bool(v))
        else:
            setattr(env, _ENV_ATTR.get(k, k), v)
    env.robot.compute_k()
    env.robot.compute_actions()
    env.robot.sonar.compute_phi()
    env.robot.sonar.compute_beam_angles()


class _CountingRandomState:
    """Forwards to the env's RandomState and counts the calls, so that the tries each of reset()'s three rejection loops used can be
    told apart: the first binomial() is drawn after 2 uniform() calls per start / goal try and one for the first core centre."""

    def __init__(self, rd):
        self.rd, self.n_uniform, self.n_binomial, self.uniform_at_first_binomial = rd, 0, 0, None

    def uniform(self, *a, **kw):
        self.n_uniform += 1
        return self.rd.uniform(*a, **kw)

    def binomial(self, *a, **kw):
        if self.uniform_at_first_binomial is None:
            self.uniform_at_first_binomial = self.n_uniform
        self.n_binomial += 1
        return self.rd.binomial(*a, **kw)

    def __getattr__(self, k):
        return getattr(self.rd, k)


def g16_reset_params():
    """g1's recipe under the parameter sets PS.RESET_SETS: world generation where the 500-try limits are reached, on maps that are
    not square, and with the pose / start / goal taken from the parameters.  `tries` = candidates drawn by the start / goal, core
    and obstacle loops."""
    keys = ("set", "seed", "start", "goal", "cores", "obs", "ncores", "nobs", "theta0", "speed0", "obs0", "state0", "next_double", "tries")
    rec = {k: [] for k in keys}
    for si, (name, spec) in enumerate(PS.RESET_SETS):
        for seed in PS.RESET_SEEDS:
            env = MarineNavEnv(seed=seed)
            apply_set(env, spec)
            for _ in range(PS.RESET_REPEATS):
                cnt = _CountingRandomState(env.rd)
                env.rd = cnt
                ob = env.reset()
                env.rd = cnt.rd
                sg = 0 if cnt.uniform_at_first_binomial is None else (cnt.uniform_at_first_binomial - 1) // 2
                pose = 2 if env.random_reset_state else 0
                ob_tries = (cnt.n_uniform - 2 * sg - 2 * cnt.n_binomial - pose) // 2
                assert cnt.n_binomial > 0 and 2 * (sg + cnt.n_binomial + ob_tries) + pose == cnt.n_uniform
                c, o, n1, n2 = world_arrays(env)
                rec["set"].append(si); rec["seed"].append(seed)
                rec["start"].append(env.start.copy()); rec["goal"].append(env.goal.copy())
                rec["cores"].append(c); rec["obs"].append(o); rec["ncores"].append(n1); rec["nobs"].append(n2)
                rec["theta0"].append(env.robot.init_theta); rec["speed0"].append(env.robot.init_speed)
                rec["obs0"].append(ob); rec["state0"].append(robot_state(env)); rec["next_double"].append(peek_next_double(env))
                rec["tries"].append([sg, cnt.n_binomial, ob_tries])
    out = {k: np.array(v) for k, v in rec.items()}
    out["set_names"] = np.array([n for n, _ in PS.RESET_SETS])
    # what the sets are there for
    tries, st = out["tries"], out["set"]
    sel = lambda name: st == [n for n, _ in PS.RESET_SETS].index(name)
    assert (tries[sel("R1")][:, 0] == 500).all()
    r2 = tries[sel("R2")][:, 0]
    assert (r2 == 500).sum() >= 10 and ((r2 < 500) & (r2 > 64)).sum() >= 1, r2
    for name in ("R3", "R6"):
        assert ((out["ncores"][sel(name)] < 8) & (tries[sel(name)][:, 1] == 500)).sum() >= 10, name
    r4 = sel("R4")
    assert (out["ncores"][r4] < 8).sum() >= 1 and ((out["ncores"][r4] == 8) & (tries[r4][:, 1] > 64)).sum() >= 1
    assert ((out["nobs"][sel("R5")] < 10) & (tries[sel("R5")][:, 2] == 500)).sum() >= 10
    for name in ("R7a", "R7b"):
        assert (out["ncores"][sel(name)] == 8).all() and (out["nobs"][sel(name)] == 10).all()
    # check_core tests `y + r > width` (sic, :349).  R7a (60 x 36): cores reach over the top edge, which a test against the height
    # would refuse; R7b (36 x 60): no core above y = 36 - r although the map goes on to 60
    assert (out["cores"][sel("R7a")][:, :, 1] + 0.5 > 36.0).any()
    assert (out["cores"][sel("R7b")][:, :, 1] + 0.5 <= 36.0).all() and (out["obs"][sel("R7b")][:, :, 1] > 36.0).any()
    assert (out["start"][sel("R8")] == np.array([7.0, 9.0])).all() and (out["theta0"][sel("R8")] == 2.5).all()
    for name, _ in PS.RESET_SETS:
        m = sel(name)
        print(f"  g16 {name}: start/goal tries {np.bincount(np.minimum(tries[m][:, 0] // 64, 8))}, "
              f"short of cores {(out['ncores'][m] < PS.RESET_SETS[int(st[m][0])][1].get('num_cores', 8)).sum()}/36, "
              f"short of obstacles {(out['nobs'][m] < PS.RESET_SETS[int(st[m][0])][1].get('num_obs', 5)).sum()}/36, "
              f"core tries max {tries[m][:, 1].max()}, obstacle tries max {tries[m][:, 2].max()}")
    np.savez_compressed(os.path.join(OUT, "g16_reset_params.npz"), **out)


def _eval_step(env, sin, a, ep_t):
    env.robot.x, env.robot.y, env.robot.theta, env.robot.speed = (float(v) for v in sin)
    env.robot.velocity = np.zeros(2)
    env.episode_timesteps = ep_t
    ob, r, d, info = env.step(a)
    return ob, r, d, INFO_CODE[info["state"]], robot_state(env)


def _hit(ob):
    p = np.asarray(ob)[4:].reshape(11, 2)
    return ~((p[:, 0] == 0) & (p[:, 1] == 0))


def g17_step_params(n_worlds=8, per_world=32):
    """g3's recipe under the parameter sets PS.STEP_SETS, plus stability flags: a beam's hit / miss, or the info code, is `stable`
    if it is the same with sonar.range, every obstacle radius, goal_dis and robot.r each moved by +-1e-4."""
    keys = ("set", "cores", "obs_tab", "n", "start", "goal", "state_in", "action", "ep_t", "obs", "reward", "done", "info", "state_out",
            "beam_stable", "info_stable")
    rec = {k: [] for k in keys}
    eps = 1e-4
    for si, (name, spec) in enumerate(PS.STEP_SETS):
        rng = np.random.RandomState(1700 + si)
        W, H = spec.get("width", 50.0), spec.get("height", 50.0)
        first = len(rec["set"])
        for wi in range(n_worlds):
            nc, no, md = [(8, 10, 30.0), (6, 8, 30.0), (8, 10, 25.0), (4, 10, 30.0)][wi % 4]
            env = MarineNavEnv(seed=17_000 + 100 * si + wi)
            apply_set(env, spec)
            env.num_cores, env.num_obs, env.min_start_goal_dis = nc, no, md
            env.reset()
            c, o, n1, n2 = world_arrays(env)
            for j in range(per_world):
                # a third near an obstacle, a third near the goal; of the rest S4 puts half within 0.5 m of a map edge (either side
                # of it) and S5 three in four within 1.5 m of a core centre (a quarter of all)
                mode = j % 3
                if mode == 1 and n2 > 0:
                    k = env.obstacles[rng.randint(n2)]
                    ang = rng.uniform(0, 2 * np.pi)
                    dist = k.r + rng.uniform(0.3, 4.0)
                    x, y = k.x + dist * np.cos(ang), k.y + dist * np.sin(ang)
                elif mode == 2:
                    ang = rng.uniform(0, 2 * np.pi)
                    dist = rng.uniform(0.5, 2.5 * env.goal_dis)
                    x, y = env.goal[0] + dist * np.cos(ang), env.goal[1] + dist * np.sin(ang)
                elif name == "S4" and (j // 3) % 2 == 0:
                    x, y = rng.uniform(0, W), rng.uniform(0, H)
                    edge = rng.randint(4)
                    off = rng.uniform(-0.5, 0.5)
                    if edge < 2:
                        x = (0.0, W)[edge] + off
                    else:
                        y = (0.0, H)[edge - 2] + off
                elif name == "S5" and (j // 3) % 4 != 3 and n1 > 0:
                    k = env.cores[rng.randint(n1)]
                    ang = rng.uniform(0, 2 * np.pi)
                    dist = rng.uniform(0.0, 1.5)
                    x, y = k.x + dist * np.cos(ang), k.y + dist * np.sin(ang)
                else:
                    x, y = rng.uniform(0, W), rng.uniform(0, H)
                theta = rng.uniform(0, 2 * np.pi)
                speed = rng.uniform(0, env.robot.max_speed)
                a = int(rng.randint(9))
                ep_t = int(rng.choice([0, 5, 999, 1000], p=[0.3, 0.3, 0.25, 0.15]))
                sin = np.array([x, y, theta, speed])
                ob, r, d, info, sout = _eval_step(env, sin, a, ep_t)
                # stability: the same sample with each threshold moved by +-1e-4
                hits, infos = [_hit(ob)], [info]
                keep = (env.robot.sonar.range, env.goal_dis, env.robot.r, [k.r for k in env.obstacles])
                for sg in (+eps, -eps):
                    for what in ("range", "radius", "goal_dis", "robot_r"):
                        if what == "range":
                            env.robot.sonar.range = keep[0] + sg
                        elif what == "radius":
                            for k, rr in zip(env.obstacles, keep[3]):
                                k.r = rr + sg
                        elif what == "goal_dis":
                            env.goal_dis = keep[1] + sg
                        else:
                            env.robot.r = keep[2] + sg
                        ob2, _, _, info2, _ = _eval_step(env, sin, a, ep_t)
                        hits.append(_hit(ob2)); infos.append(info2)
                        env.robot.sonar.range, env.goal_dis, env.robot.r = keep[:3]
                        for k, rr in zip(env.obstacles, keep[3]):
                            k.r = rr
                hits = np.array(hits)
                rec["set"].append(si); rec["cores"].append(c); rec["obs_tab"].append(o); rec["n"].append([n1, n2])
                rec["start"].append(env.start.copy()); rec["goal"].append(env.goal.copy())
                rec["state_in"].append(sin); rec["action"].append(a); rec["ep_t"].append(ep_t)
                rec["obs"].append(ob); rec["reward"].append(r); rec["done"].append(d); rec["info"].append(info); rec["state_out"].append(sout)
                rec["beam_stable"].append((hits == hits[0]).all(axis=0)); rec["info_stable"].append(all(i == info for i in infos))
        # what the set is there for: every outcome it can produce, both kinds of beams, few knife-edge items
        info = np.array(rec["info"][first:]); hit = np.array([_hit(ob) for ob in rec["obs"][first:]])
        bst = np.array(rec["beam_stable"][first:]); ist = np.array(rec["info_stable"][first:])
        codes = [0, 2, 3, 4] + ([1] if spec.get("set_boundary") else [])
        counts = {k: int((info == k).sum()) for k in codes}
        print(f"  g17 {name}: info counts {counts}, beam hits {hit.mean():.3f}, unstable beams {(~bst).sum()}/{bst.size}, unstable infos {(~ist).sum()}/{ist.size}")
        assert min(counts.values()) >= 10 and set(np.unique(info)) <= set(codes), counts
        assert 0.10 <= hit.mean() <= 0.90, hit.mean()
        assert (~bst).mean() <= 0.01 and (~ist).mean() <= 0.01
    out = {k: np.array(v) for k, v in rec.items()}
    out["set_names"] = np.array([n for n, _ in PS.STEP_SETS])
    np.savez_compressed(os.path.join(OUT, "g17_step_params.npz"), **out)


def _observation_longdouble(env):
    """get_observation() with robot.py:125-198's slope-form intersection and marinenav_env.py:281-326's frame change evaluated in
    np.longdouble (64-bit mantissa).  The beam angle and the snap decision (:132-136) are the reference's float64 ones: they select
    the formula.  Returns (obs [26] longdouble, hit [11])."""
    ld = np.longdouble
    rb = env.robot
    X, Y, th, rng_ = ld(rb.x), ld(rb.y), ld(rb.theta), ld(rb.sonar.range)
    pts, hit = [], []
    for rel_a in rb.sonar.beam_angles:
        angle = rb.theta + rel_a
        vert = np.abs(angle - np.pi / 2) < 1e-03 or np.abs(angle - 3 * np.pi / 2) < 1e-03
        al = ld(rb.theta) + ld(rel_a)
        ca, sa = np.cos(al), np.sin(al)
        best, have, dist = None, False, ld(np.inf)
        for ob in env.obstacles:
            ox, oy, orad = ld(ob.x), ld(ob.y), ld(ob.r)
            if vert:
                M = orad * orad - (X - ox) * (X - ox)
                if M < 0:
                    continue
                x1 = x2 = X
                y1, y2 = oy - np.sqrt(M), oy + np.sqrt(M)
            else:
                K = np.tan(al)
                a = 1 + K * K
                b = 2 * K * (Y - K * X - oy) - 2 * ox
                c = ox * ox + (Y - K * X - oy) * (Y - K * X - oy) - orad * orad
                delta = b * b - 4 * a * c
                if delta < 0:
                    continue
                x1 = (-b - np.sqrt(delta)) / (2 * a)
                x2 = (-b + np.sqrt(delta)) / (2 * a)
                y1 = Y + K * (x1 - X)
                y2 = Y + K * (x2 - X)
            n1, n2 = np.sqrt((x1 - X) ** 2 + (y1 - Y) ** 2), np.sqrt((x2 - X) ** 2 + (y2 - Y) ** 2)
            vx, vy, nv = (x1 - X, y1 - Y, n1) if n1 < n2 else (x2 - X, y2 - Y, n2)
            if nv > rng_:
                continue
            if vx * ca + vy * sa < 0:
                continue
            if have and nv >= dist:
                break
            dist, best, have = nv, (vx + X, vy + Y), True
        pts.append(best); hit.append(have)
    c, s = np.cos(th), np.sin(th)
    rot = lambda px, py: (c * (px - X) + s * (py - Y), -s * (px - X) + c * (py - Y))
    vel = (c * ld(rb.velocity[0]) + s * ld(rb.velocity[1]), -s * ld(rb.velocity[0]) + c * ld(rb.velocity[1]))
    out = [vel[0], vel[1], *rot(ld(env.goal[0]), ld(env.goal[1]))]
    for p, h in zip(pts, hit):
        out.extend(rot(*p) if h else (ld(0), ld(0)))
    return np.array(out, dtype=ld), np.array(hit)


def g18_sonar_params_edge():
    """Observation-only cases in g4's layout at sonar.range = 80 (on a 120 x 120 map) and 15: the outermost beam inside and outside
    the 1e-3 rad snap window with an obstacle next to it on the side away from the fan, the range limit, an obstacle behind, several
    obstacles on one beam; at range 80 also with sonar.angle = 0.9 pi and an obstacle on an outermost beam.  The robot stands still (speed 0, no current), so a step without acceleration or turn leaves it where it
    is.  `obs_ld`: the same formulas in np.longdouble."""
    cases = []

    def add(name, rng_, obstacles, x, y, theta, goal=(60.0, 60.0), angle=PS.EDGE_ANGLES[0]):
        env = MarineNavEnv(seed=0)
        apply_set(env, dict(sonar_range=rng_, sonar_angle=angle, width=PS.EDGE_MAP, height=PS.EDGE_MAP))
        env.cores.clear()
        env.obstacles.clear()
        for (ox, oy, r) in obstacles:
            env.obstacles.append(Obstacle(ox, oy, r))
        env.goal = np.array(goal)
        env.robot.x, env.robot.y, env.robot.theta, env.robot.speed = x, y, theta, 0.0
        env.robot.velocity = np.zeros(2)
        ob = env.get_observation()
        ob_ld, hit_ld = _observation_longdouble(env)
        assert np.array_equal(hit_ld, _hit(ob)), name
        o = np.zeros((MAXO, 3))
        for i, ob_ in enumerate(obstacles):
            o[i] = ob_
        cases.append(dict(name=name, range=rng_, angle=angle, obs_tab=o, n_obs=len(obstacles), pose=[x, y, theta], goal=list(goal),
                          vel=[0.0, 0.0], obs=ob, obs_ld=ob_ld.astype(np.float64)))
        return _hit(ob)

    rel = [-(2 * np.pi / 3) / 2 + i * ((2 * np.pi / 3) / 10) for i in range(11)]
    seen = set()
    for rng_ in (80.0, 15.0):
        for bi in (0, 10):
            for vert, sgn in ((np.pi / 2, 1.0), (3 * np.pi / 2, -1.0)):
                # the side of the cast beam that faces away from the fan: clockwise of beam 0, counter-clockwise of beam 10
                side = (1.0 if bi == 0 else -1.0) * sgn
                x, y = 60.0, 60.0 - sgn * 50.0
                for eps in (0.0009, -0.0009, 0.0011, -0.0011):
                    th = vert - rel[bi] + eps
                    assert 0.0 <= th < 2 * np.pi
                    h = add(f"edge_r{rng_:.0f}_b{bi}_{'up' if sgn > 0 else 'down'}_{eps}", rng_, [(x + side * 0.999, y + sgn * 0.85 * rng_, 1.0)], x, y, th)
                    seen.add((abs(eps) < 1e-3, bool(h[bi])))
        # the range limit: the near intersection of the centre beam 1e-6 inside / outside the range
        add(f"range_in_r{rng_:.0f}", rng_, [(20.0 + rng_ + 1.0 - 1e-6, 60.0, 1.0)], 20.0, 60.0, 0.0)
        add(f"range_out_r{rng_:.0f}", rng_, [(20.0 + rng_ + 1.0 + 1e-6, 60.0, 1.0)], 20.0, 60.0, 0.0)
        add(f"behind_r{rng_:.0f}", rng_, [(20.0 - 0.5 * rng_, 60.0, 1.0)], 20.0, 60.0, 0.0)
        near, far, mid = (20.0 + 0.3 * rng_, 60.0, 1.0), (20.0 + 0.8 * rng_, 60.0, 2.0), (20.0 + 0.55 * rng_, 60.2, 0.8)
        for order_name, order in (("nf", [near, far]), ("fn", [far, near]), ("mfn", [mid, far, near]), ("fmn", [far, mid, near]),
                                  ("nfm", [near, far, mid])):
            add(f"break_{order_name}_r{rng_:.0f}", rng_, order, 20.0, 60.0, 0.0)
            add(f"break2_{order_name}_r{rng_:.0f}", rng_, order, 20.0, 60.0, 0.02)
    assert seen == {(True, True), (False, True), (False, False)}, seen      # a snapped beam always hits; an unsnapped one does both
    # a wide fan (0.9 pi) at range 80: an obstacle ON an outermost beam (and on its neighbour) at 0.9 x range, where the work-list's
    # wedge test depends on sin(sonar_angle / 2) by more than an obstacle's radius
    wide = PS.EDGE_ANGLES[1]
    rel_w = [-wide / 2 + i * (wide / 10) for i in range(11)]
    for bi in (0, 1, 9, 10):
        for th in (0.3, 2.0, 4.4):
            ang = th + rel_w[bi]
            assert min(abs(ang - np.pi / 2), abs(ang - 3 * np.pi / 2)) > 0.01
            ux, uy = np.cos(ang), np.sin(ang)
            x, y = 60.0 - 36.0 * ux, 60.0 - 36.0 * uy
            h = add(f"wide_r80_b{bi}_{th}", 80.0, [(x + 72.0 * ux, y + 72.0 * uy, 1.0)], x, y, th, angle=wide)
            assert h[bi] and h.sum() == 1
    obs = np.array([c["obs"] for c in cases]); obs_ld = np.array([c["obs_ld"] for c in cases])
    print(f"  g18: {len(cases)} cases, max |obs - obs_ld| {np.abs(obs - obs_ld).max():.3e}")
    np.savez_compressed(
        os.path.join(OUT, "g18_sonar_params_edge.npz"),
        names=np.array([c["name"] for c in cases]), range=np.array([c["range"] for c in cases]), angle=np.array([c["angle"] for c in cases]),
        obs_tab=np.array([c["obs_tab"] for c in cases]), n_obs=np.array([c["n_obs"] for c in cases]),
        pose=np.array([c["pose"] for c in cases]), goal=np.array([c["goal"] for c in cases]),
        vel=np.array([c["vel"] for c in cases]), obs=obs, obs_ld=obs_ld)


# ---- g20: the termination ladder on its thresholds, ties and coinciding rungs ---------------------------------------------------
def _savez_fixed(path, arrays):
    """np.savez_compressed without the clock: every member stamped 1980-01-01, members in the order given, so the same arrays give the same bytes."""
    import zipfile
    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_DEFLATED, compresslevel=9) as z:
        for k, v in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(v), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue(), compresslevel=9)


def g20_ladder_edges():
    """tests/ladder_edges.py's case table through MarineNavEnv.step: obstacle list + KD-tree, goal, pose, episode_timesteps and the set's parameters
    written into a fresh env, one step.  `ref_ok`: the reference can express the case (its ladder holds 1000 for the episode limit; the other rows stay
    zero).  On a TIE case the nearest obstacle is whatever scipy's KD-tree answers: kept apart (`tie_ref_nearest`, `tie_ref_info`), for the record only."""
    import scipy.spatial
    import ladder_edges as LE
    cases = LE.table()
    inp, ok = LE.arrays(), LE.expressible()
    n = len(cases)
    ref = dict(ref_obs=np.zeros((n, 26)), ref_reward=np.zeros(n), ref_done=np.zeros(n, bool), ref_info=np.zeros(n, np.uint8), ref_state=np.zeros((n, 6)),
               ref_ep_t=np.zeros(n, np.int64), ref_tot_t=np.zeros(n, np.int64), tie_ref_nearest=np.full(n, -1, np.int32), tie_ref_info=np.zeros(n, np.uint8))
    for i, c in enumerate(cases):
        if not ok[i]:
            continue
        env = MarineNavEnv(seed=0)
        apply_set(env, LE.pset_spec(c.pset))
        env.cores.clear()
        env.obstacles.clear()
        for (ox, oy, r) in c.obstacles:
            env.obstacles.append(Obstacle(ox, oy, r))
        if c.obstacles:
            env.obs_centers = scipy.spatial.KDTree(np.array([[o[0], o[1]] for o in c.obstacles]))
        env.goal = np.array(c.goal)
        env.total_timesteps = c.tot_t
        ob, r, d, info, sout = _eval_step(env, c.pose, c.action, c.ep_t)
        if c.tie:
            ref["tie_ref_nearest"][i] = env.obs_centers.query(np.array([env.robot.x, env.robot.y]))[1]
            ref["tie_ref_info"][i] = info
        ref["ref_obs"][i], ref["ref_reward"][i], ref["ref_done"][i], ref["ref_info"][i], ref["ref_state"][i] = ob, r, d, info, sout
        ref["ref_ep_t"][i], ref["ref_tot_t"][i] = env.episode_timesteps, env.total_timesteps
    exp = LE.expected()
    tie = inp["tie"]
    agree = ok & ~tie & (ref["ref_info"] == exp["info"])
    print(f"  g20: {n} cases, {int(ok.sum())} the reference can express; info equal to exact arithmetic on {int(agree.sum())} of {int((ok & ~tie).sum())} "
          f"untied ones; KD-tree = first in generation order on {int((ref['tie_ref_info'][tie] == exp['info'][tie]).sum())} of {int(tie.sum())} ties")
    out = dict(inp)
    out["ref_ok"] = ok
    out["set_names"] = np.array(LE.PSET_NAMES)
    out.update(ref)
    _savez_fixed(os.path.join(OUT, "g20_ladder_edges.npz"), out)


if __name__ == "__main__":
    which = sys.argv[1:] or ["g1", "g2", "g3", "g4", "g5", "g6", "g7", "g8", "g9", "g12", "g13", "g14", "g15", "g16", "g17", "g18", "g19", "g20"]
    if "g20" in which:
        g20_ladder_edges()
    if "g16" in which:
        g16_reset_params()
    if "g17" in which:
        g17_step_params()
    if "g18" in which:
        g18_sonar_params_edge()
    if "g12" in which:
        g12_replay()
    if "g15" in which:
        g15_replay_nstep()
    if "g13" in which:
        g13_learn_loop()
    if "g14" in which:
        g14_iqn_episodes()
    if "g1" in which:
        g1_reset(); g1b_eval_worlds()
    if "g2" in which:
        g2_traces()
    if "g3" in which:
        g3_single_step()
    if "g4" in which:
        g4_sonar_edge()
    if "g5" in which:
        g5_velocity()
    if "g6" in which:
        g6_pretrained_replay()
    if "g7" in which:
        g7_iqn()
    if "g8" in which:
        g8_boundary_trace()
    if "g9" in which:
        g9_planners()
    if "g19" in which:
        g19_planner_branches()
    for f in sorted(os.listdir(OUT)):
        p = os.path.join(OUT, f)
        if os.path.isfile(p):
            print(f"{os.path.getsize(p):>9d}  {f}")
