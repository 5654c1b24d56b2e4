"""The parameter sets behind the fixtures g16_reset_params / g17_step_params / g18_sonar_params_edge, shared by their generator
(tests/golden/make_golden.py) and by the tests that replay them (tests/test_params_golden.py through the CPU twin,
tests/test_params_gpu.py on the device).  A set is a dict of `mn_params` fields (include/marinenav_hip.h); the fixtures hold
only a set's INDEX, so a set may never be edited without regenerating them.  `start` / `goal` are not `mn_params` fields: they
go through mn_set_start_goal (the reference's `env.start = ...` with `reset_start_and_goal = False`)."""
import ctypes as C

import numpy as np

PI = np.pi

# g16: world generation.  Every set runs seeds 0-11, three consecutive resets each.
RESET_SETS = [
    ("R1", dict(num_cores=8, num_obs=10, min_start_goal_dis=70.0)),      # start / goal: all 500 tries, the running-best pair is kept
    ("R2", dict(num_cores=8, num_obs=10, min_start_goal_dis=60.0)),      # ... all but one: that one stops in a later pass
    ("R3", dict(v_rel_max=0.1, p=0.1, num_cores=8, num_obs=6, min_start_goal_dis=30.0)),      # the core loop gives up short of 8
    ("R4", dict(v_rel_max=0.3, p=0.3, num_cores=8, num_obs=6, min_start_goal_dis=30.0)),      # ... mostly completes late in the 500
    ("R5", dict(obs_r_range=(4.0, 7.0), num_cores=4, num_obs=10, min_start_goal_dis=30.0)),   # the obstacle loop gives up short of 10
    ("R6", dict(core_r=4.0, clear_r=14.0, num_cores=8, num_obs=6)),
    ("R7a", dict(width=60.0, height=36.0, num_cores=8, num_obs=10, min_start_goal_dis=30.0)),
    ("R7b", dict(width=36.0, height=60.0, num_cores=8, num_obs=10, min_start_goal_dis=30.0)),
    ("R8", dict(random_reset_state=0, init_theta=2.5, init_speed=1.2, reset_start_and_goal=0, start=(7.0, 9.0), goal=(41.0, 33.0),
                v_range=(2.0, 4.0), core_r=1.5)),
]
RESET_SEEDS = tuple(range(12))
RESET_REPEATS = 3

# g17: single steps.  Per set 8 worlds x 32 (state, action, ep_t) triples.
STEP_SETS = [
    ("S1", dict(dt=0.05, N=5, max_speed=3.0, a=(-0.6, 0.0, 0.5), w=(-0.7, 0.1, 0.4), robot_r=1.3)),
    ("S2", dict(sonar_range=15.0, sonar_angle=0.9 * PI)),      # work-list wedge filter on, wide wedge
    ("S3", dict(sonar_range=6.0, sonar_angle=PI)),             # filter off
    ("S4", dict(goal_dis=4.0, timestep_penalty=-0.3, collision_penalty=-7.0, goal_reward=33.0, set_boundary=1, width=60.0, height=36.0)),
    ("S5", dict(core_r=1.5)),
]

# g18: per case sonar_range, sonar_angle and the map (the other parameters stay at their defaults)
EDGE_MAP = 120.0
EDGE_ANGLES = (2 * PI / 3, 0.9 * PI)
EDGE_GROUPS = [(80.0, EDGE_ANGLES[0]), (15.0, EDGE_ANGLES[0]), (80.0, EDGE_ANGLES[1])]      # (sonar_range, sonar_angle) of a handle
EDGE_IDS = ["range80", "range15", "range80_wide"]


def edge_group(z, group):
    """(fixture rows, mn_params fields) of one (sonar_range, sonar_angle) group of g18."""
    rows = np.nonzero((z["range"] == group[0]) & (z["angle"] == group[1]))[0]
    return rows, dict(sonar_range=group[0], sonar_angle=group[1], width=EDGE_MAP, height=EDGE_MAP)

ARRAY_FIELDS = ("v_range", "obs_r_range", "a", "w")


def apply(p, spec):
    """Write a set into an MnParams structure (distributional_rl_navigation_amd._capi)."""
    for k, v in spec.items():
        if k in ("start", "goal"):
            continue
        if k in ARRAY_FIELDS:
            arr = getattr(p, k)
            for i, x in enumerate(v):
                arr[i] = float(x)
        else:
            setattr(p, k, type(getattr(p, k))(v))
    return p


def driver_set(d, spec):
    """The same through tests/test_cpu_twin.py's Driver (either library): mn_set_params, then mn_set_start_goal."""
    apply(d.p, spec)
    assert d.L.mn_set_params(d.h, C.byref(d.p)) == 0, d.L.mn_last_error(d.h)
    if "start" in spec:
        s = (C.c_double * 2)(*spec["start"]); g = (C.c_double * 2)(*spec["goal"])
        assert d.L.mn_set_start_goal(d.h, -1, s, g) == 0


def vec_env_set(env, spec):
    """The same through VecMarineNavEnv: one mn_set_params with every field of the set."""
    apply(env.params, spec)
    env._check(env.L.mn_set_params(env.h, C.byref(env.params)))
    if "start" in spec:
        env.set_start_goal(spec["start"], spec["goal"])


def beam_rel(spec):
    """robot.py:14-21 in its own expression order."""
    angle = spec.get("sonar_angle", 2 * PI / 3)
    phi = angle / 10
    return np.array([-angle / 2 + i * phi for i in range(11)])


def slope_tol(theta, spec, base=1e-9):
    """[n, 22] tolerance of the beam entries against the reference's slope-form intersection (robot.py:164-179), whose own rounding
    error grows like K^2, K = tan(beam angle): base + 1e-12 K^2 (tests/test_env_gpu.py::test_g3_single_step_golden)."""
    K = np.tan(np.asarray(theta)[:, None] + beam_rel(spec)[None, :])
    return np.repeat(base + 1e-12 * K * K, 2, axis=1)


def miss(obs):
    """[n, 11] bool: the beam is reported as a miss, the point exactly (0, 0) (marinenav_env.py:315-316)."""
    p = np.asarray(obs)[:, 4:].reshape(len(obs), 11, 2)
    return (p[:, :, 0] == 0) & (p[:, :, 1] == 0)


# ---- assertions shared by the CPU-twin and the device tests ---------------------------------------------------------------------
def check_reset(z, rows, w, peek, obs0, state, obs_atol=1e-10):
    """Fixture rows `rows` (one per env) of g16 against what a library generated: `w` the padded tables (Driver.worlds() layout),
    `peek` the next double of every stream, `obs0` the first observations, `state` [n, 6].  Tables, counts, start / goal, pose and
    stream position bit for bit; the first observation to `obs_atol`, the velocity in `state` to 1e-9."""
    assert np.array_equal(w["ncores"], z["ncores"][rows]) and np.array_equal(w["nobs"], z["nobs"][rows])
    assert np.array_equal(w["cores"], z["cores"][rows]) and np.array_equal(w["obstacles"], z["obs"][rows])
    assert np.array_equal(w["start"], z["start"][rows]) and np.array_equal(w["goal"], z["goal"][rows])
    assert np.array_equal(w["theta0"], z["theta0"][rows]) and np.array_equal(w["speed0"], z["speed0"][rows])
    assert np.array_equal(peek, z["next_double"][rows])
    assert np.array_equal(state[:, :4], z["state0"][rows][:, :4])
    np.testing.assert_allclose(state[:, 4:], z["state0"][rows][:, 4:], rtol=0, atol=1e-9)
    np.testing.assert_allclose(obs0, z["obs0"][rows], rtol=0, atol=obs_atol)


def check_step_f64(z, rows, spec, obs, rew, done, info, state):
    """g3's float64 assertions on rows `rows` of g17: done / info and every beam's hit / miss equal, head of the observation, reward
    and state within 1e-9, beams within 1e-9 + 1e-12 K^2."""
    assert np.array_equal(np.asarray(done).astype(bool), z["done"][rows]) and np.array_equal(info, z["info"][rows])
    ref = z["obs"][rows]
    assert np.array_equal(miss(obs), miss(ref))
    np.testing.assert_allclose(obs[:, :4], ref[:, :4], rtol=0, atol=1e-9)
    err, tol = np.abs(obs[:, 4:] - ref[:, 4:]), slope_tol(z["state_out"][rows][:, 2], spec)
    assert (err <= tol).all(), (float(err.max()), np.argwhere(err > tol)[:5])
    np.testing.assert_allclose(state, z["state_out"][rows], rtol=0, atol=1e-9)
    np.testing.assert_allclose(rew, z["reward"][rows], rtol=0, atol=1e-9)


def check_edge(z, rows, obs, what):
    """g18: flags exact, every element within 1e-9 + 2 |obs - obs_ld| of the reference (obs_ld = the reference's formulas in long
    double: twice its distance from them is what the float64 slope form itself is good for at this range).  Returns the largest
    tolerance used and the largest error."""
    ref, tol = z["obs"][rows], 1e-9 + 2 * np.abs(z["obs"][rows] - z["obs_ld"][rows])
    assert np.array_equal(miss(obs), miss(ref)), (what, [str(z["names"][rows][i]) for i in np.nonzero((miss(obs) != miss(ref)).any(axis=1))[0]])
    err = np.abs(obs - ref)
    bad = np.nonzero((err > tol).any(axis=1))[0]
    assert len(bad) == 0, (what, [str(z["names"][rows][i]) for i in bad], float(err.max()))
    return float(tol.max()), float(err.max())
