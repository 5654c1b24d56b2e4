"""The reset and step kernels AWAY from the default env parameters, against fixtures generated from the Python reference
(tests/golden/make_golden.py g16 / g17 / g18; tests/test_params_golden.py replays the same files through the CPU oracle):

  * g16: world generation where the three rejection loops of the reset kernel reach their 500 tries (the clamp of the last pass, the
    running-best start / goal pair, worlds with fewer objects than asked for and the stream position after one), on maps that are
    not square (check_core's `y + r > width`, every span), with pose / start / goal taken from the parameters -- through mn_reset and
    through the reset kernel that runs under the act kernel;
  * g17: single steps under other robot, sonar, reward and map parameters, i.e. every constant `derive()` (csrc/mn_capi.hip) makes
    from them, for every lanes-per-env mapping, in float64 and in mixed precision;
  * g18: the sonar work-list at sonar.range 80 and 15 -- the outermost beam snapped to the vertical just outside the fan;
  * a later mn_set_params rebuilds the derived constants; the episode kernels step with them exactly as mn_step does."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import params_sets as PS      # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
G = os.path.join(os.path.dirname(__file__), "golden")
RESET_IDS = [n for n, _ in PS.RESET_SETS]
STEP_IDS = [n for n, _ in PS.STEP_SETS]


@pytest.fixture(scope="module")
def torch():
    import torch as t
    if not t.cuda.is_available():
        pytest.skip("no GPU")
    return t


@pytest.fixture(scope="module")
def g16():
    return np.load(os.path.join(G, "g16_reset_params.npz"))


@pytest.fixture(scope="module")
def g17():
    return np.load(os.path.join(G, "g17_step_params.npz"))


@pytest.fixture(scope="module")
def g18():
    return np.load(os.path.join(G, "g18_sonar_params_edge.npz"))


def make_env(n, precision, spec=None, **kw):
    """A handle CREATED with the set's parameters (mn_create runs derive() on them)."""
    from distributional_rl_navigation_amd import _capi
    from distributional_rl_navigation_amd.marinenav_env.vec_env import VecMarineNavEnv
    env = VecMarineNavEnv(n, device=DEV, precision=precision, obs64=precision == "f64", params=PS.apply(_capi.default_params(), spec or {}), **kw)
    if spec and "start" in spec:
        env.set_start_goal(spec["start"], spec["goal"])
    return env


def padded_worlds(env):
    """get_worlds() in the padded layout of the fixtures (tests/test_cpu_twin.py Driver.worlds)."""
    ws = env.get_worlds()
    n = len(ws)
    out = dict(cores=np.zeros((n, 8, 4)), obstacles=np.zeros((n, 10, 3)), ncores=np.array([w["n_cores"] for w in ws]),
               nobs=np.array([w["n_obs"] for w in ws]), start=np.array([w["start"] for w in ws]), goal=np.array([w["goal"] for w in ws]),
               theta0=np.array([w["init_theta"] for w in ws]), speed0=np.array([w["init_speed"] for w in ws]))
    for i, w in enumerate(ws):
        out["cores"][i, :w["n_cores"]] = w["cores"]
        out["obstacles"][i, :w["n_obs"]] = w["obstacles"]
    return out


@pytest.mark.parametrize("under_act", [False, True], ids=["mn_reset", "under_act"])
@pytest.mark.parametrize("precision", ["f64", "mixed"])
@pytest.mark.parametrize("si", range(len(PS.RESET_SETS)), ids=RESET_IDS)
def test_g16_reset_under_other_parameters(torch, g16, si, precision, under_act):
    """12 seeds x 3 consecutive resets per set: world tables, counts, start / goal, pose and the stream position bit for bit; first
    observation <= 1e-10 from the float64 copies of an f64 handle, <= 1e-5 (the project's float32 bound) from the float32 rows of a
    mixed one.  `under_act`: every one of the three resets is made by mn_reset_done_async's kernel (the RNG block read in place),
    after two steps that end every episode (max_episode_steps = 1; a step draws nothing from the stream)."""
    spec = dict(PS.RESET_SETS[si][1])
    if under_act:
        spec["max_episode_steps"] = 1
    env = make_env(len(PS.RESET_SEEDS), precision, spec, seeds=PS.RESET_SEEDS)
    env.set_reset_under_act_max(2 ** 31 - 1)
    base = np.nonzero(g16["set"] == si)[0]
    zero = torch.zeros(env.n_envs, dtype=torch.int32, device=DEV)
    for k in range(PS.RESET_REPEATS):
        if under_act:
            env.step(zero); env.step(zero)
            assert int(env.done.sum()) == env.n_envs
            obs = env.reset_done(under_next_act=True)
            assert env.late_rows is not None
            env.join_reset()
        else:
            obs = env.reset()
        torch.cuda.synchronize()
        obs0 = env.get_obs64() if precision == "f64" else obs.cpu().numpy().astype(np.float64)
        PS.check_reset(g16, base[k::PS.RESET_REPEATS], padded_worlds(env), env.peek_next_double(), obs0, env.get_state()[0],
                       obs_atol=1e-10 if precision == "f64" else 1e-5)
    assert env.reset_launches == ([0, PS.RESET_REPEATS] if under_act else [0, 0])
    env.close()


def load_g17(env, z, rows):
    worlds = [dict(cores=z["cores"][i][:z["n"][i][0]], obstacles=z["obs_tab"][i][:z["n"][i][1]], start=z["start"][i], goal=z["goal"][i],
                   init_theta=0.0, init_speed=0.0) for i in rows]
    env.load_worlds(worlds)
    s = np.zeros((len(rows), 6))
    s[:, :4] = z["state_in"][rows]
    env.set_state(s, z["ep_t"][rows])


@pytest.mark.parametrize("lanes", [1, 2, 4, 8])
@pytest.mark.parametrize("si", range(len(PS.STEP_SETS)), ids=STEP_IDS)
def test_g17_single_steps_f64(torch, g17, si, lanes):
    """g3's float64 assertions (done / info / hit or miss equal, floats <= 1e-9, beams <= 1e-9 + 1e-12 K^2), no sample excluded."""
    spec = PS.STEP_SETS[si][1]
    rows = np.nonzero(g17["set"] == si)[0]
    env = make_env(len(rows), "f64", spec, step_lanes=lanes)
    load_g17(env, g17, rows)
    env.step(torch.from_numpy(g17["action"][rows].astype(np.int32)).to(DEV))
    PS.check_step_f64(g17, rows, spec, env.get_obs64(), env.get_reward64(), env.done.cpu().numpy(), env.info.cpu().numpy(), env.get_state()[0])
    env.close()


@pytest.mark.parametrize("lanes", [1, 2, 4, 8])
@pytest.mark.parametrize("si", range(len(PS.STEP_SETS)), ids=STEP_IDS)
def test_g17_single_steps_mixed(torch, g17, si, lanes):
    """Mixed precision: every float32 output (observation, reward) and the pose within 1e-5 ABSOLUTE of the reference; info code and
    hit / miss equal on every item the fixture calls stable (unchanged when sonar.range, the radii, goal_dis and robot.r move by
    1e-4); unstable items that differ are counted and printed, and only their values are left out of the comparison."""
    spec = PS.STEP_SETS[si][1]
    rows = np.nonzero(g17["set"] == si)[0]
    env = make_env(len(rows), "mixed", spec, step_lanes=lanes)
    load_g17(env, g17, rows)
    env.step(torch.from_numpy(g17["action"][rows].astype(np.int32)).to(DEV))
    obs = env.obs.cpu().numpy().astype(np.float64); rew = env.reward.cpu().numpy().astype(np.float64)
    info = env.info.cpu().numpy(); done = env.done.cpu().numpy().astype(bool)
    st = env.get_state()[0]
    env.close()
    ref = g17["obs"][rows]
    info_diff = info != g17["info"][rows]
    flip = PS.miss(obs) != PS.miss(ref)
    print(f"[g17 mixed {STEP_IDS[si]} lanes={lanes}] differing unstable items: info {int((info_diff & ~g17['info_stable'][rows]).sum())} of "
          f"{int((~g17['info_stable'][rows]).sum())}, beams {int((flip & ~g17['beam_stable'][rows]).sum())} of {int((~g17['beam_stable'][rows]).sum())}")
    assert not (info_diff & g17["info_stable"][rows]).any() and not (flip & g17["beam_stable"][rows]).any()
    assert np.array_equal(done, info != 0)
    err = np.abs(obs - ref)
    err[:, 4:][np.repeat(flip, 2, axis=1)] = 0.0
    print(f"[g17 mixed {STEP_IDS[si]} lanes={lanes}] worst observation error {err.max():.3e}, reward {np.abs(rew - g17['reward'][rows])[~info_diff].max():.3e}, "
          f"pose {np.abs(st[:, :4] - g17['state_out'][rows][:, :4]).max():.3e}")
    assert (err <= 1e-5).all(), (int((err > 1e-5).sum()), float(err.max()))
    assert (np.abs(rew - g17["reward"][rows])[~info_diff] <= 1e-5).all()
    np.testing.assert_allclose(st[:, :4], g17["state_out"][rows][:, :4], rtol=0, atol=1e-5)


def g18_worlds(z, rows):
    return [dict(cores=np.zeros((0, 4)), obstacles=z["obs_tab"][i][:int(z["n_obs"][i])], start=z["pose"][i][:2], goal=z["goal"][i],
                 init_theta=float(z["pose"][i][2]), init_speed=0.0) for i in rows]


@pytest.mark.parametrize("group", PS.EDGE_GROUPS, ids=PS.EDGE_IDS)
def test_g18_sonar_edges_through_the_step_kernel(torch, g18, group):
    """The hand-built cases at sonar.range 80 (120 x 120 map) and 15: first observation of the loaded pose, then the observation the
    STEP kernel makes after an action without acceleration or turn -- the robot stands still (speed 0, no current), so it is cast from
    the same pose -- for every lanes-per-env mapping.  The third group has sonar.angle = 0.9 pi at range 80 and an obstacle on an outermost
    beam at 0.9 x range, where the work-list's wedge test depends on sin(sonar_angle / 2) by more than the obstacle's radius.  Hit / miss
    exact; values within 1e-9 + 2 |obs - obs_ld| (largest per group: 2.0e-6 at range 80 and 3.8e-6 at range 15, both at a beam 1.1e-3 rad
    off the vertical, where the reference's slope K = tan(angle) is ~900; 1.03e-9 for the wide fan)."""
    rows, spec = PS.edge_group(g18, group)
    for lanes in (1, 2, 4, 8):
        env = make_env(len(rows), "f64", spec, step_lanes=lanes)
        env.load_worlds(g18_worlds(g18, rows))
        tol, e0 = PS.check_edge(g18, rows, env.get_obs64(), f"first observation, lanes {lanes}")
        env.step(torch.full((len(rows),), 4, dtype=torch.int32, device=DEV))
        assert np.array_equal(env.get_state()[0][:, :3], g18["pose"][rows])
        _, e1 = PS.check_edge(g18, rows, env.get_obs64(), f"after a step, lanes {lanes}")
        print(f"[g18 step {PS.EDGE_IDS[PS.EDGE_GROUPS.index(group)]} lanes {lanes}] largest tolerance {tol:.3e}, largest error {max(e0, e1):.3e}")
        env.close()


@pytest.mark.parametrize("group", PS.EDGE_GROUPS, ids=PS.EDGE_IDS)
def test_g18_sonar_edges_through_the_query_kernel(torch, g18, group):
    """The same cases through `observation_at` (mn_query_observation), one query per case.  Tolerance as above."""
    rows, spec = PS.edge_group(g18, group)
    env = make_env(len(rows), "f64", spec)
    env.load_worlds(g18_worlds(g18, rows))
    st = np.zeros((len(rows), 6))
    st[:, :3] = g18["pose"][rows]
    obs = env.observation_at(st, env=np.arange(len(rows)), velocity="given", dtype=torch.float64).cpu().numpy()
    tol, e = PS.check_edge(g18, rows, obs, "observation_at")
    print(f"[g18 query {PS.EDGE_IDS[PS.EDGE_GROUPS.index(group)]}] largest tolerance {tol:.3e}, largest error {e:.3e}")
    env.close()


STEP_FIELDS = sorted({k for _, s in PS.STEP_SETS for k in s})
ATTR_NAME = {"core_r": "r"}      # VecMarineNavEnv.set_attrs speaks the reference's attribute names


def attrs_of(spec):
    """set_attrs arguments that bring a handle from ANY of the step sets to `spec`: every field a step set touches, at the set's value
    or at its default."""
    from distributional_rl_navigation_amd import _capi
    p = PS.apply(_capi.default_params(), spec)
    out = {}
    for k in STEP_FIELDS:
        v = getattr(p, k)
        out[ATTR_NAME.get(k, k)] = list(v) if k in PS.ARRAY_FIELDS else v
    return out


def _steps(torch, env, z, rows, actions):
    load_g17(env, z, rows)
    out = []
    for a in actions:
        o, r, d, i = env.step(a)
        out.append((o.clone(), r.clone(), d.clone(), i.clone(), env.get_state()[0], env.get_obs64() if env.precision == "f64" else None))
    return out


@pytest.mark.parametrize("precision", ["f64", "mixed"])
def test_set_params_rebuilds_the_derived_tables(torch, g17, precision):
    """A handle created with the defaults and stepped once, then set_attrs to S1, to S2 and so on, against handles CREATED with those
    parameters: observations, rewards, done / info and state of 5 steps from the same 67 loaded states, bit for bit."""
    n = 67
    g = torch.Generator(device=DEV); g.manual_seed(11)
    actions = [torch.randint(0, 9, (n,), device=DEV, dtype=torch.int32, generator=g) for _ in range(5)]
    live = make_env(n, precision, seed=4)
    live.reset()
    live.step(actions[0])
    for si, (name, spec) in enumerate(PS.STEP_SETS):
        rows = np.nonzero(g17["set"] == si)[0][:n]
        live.set_attrs(**attrs_of(spec))
        made = make_env(n, precision, spec, seed=4)
        a, b = _steps(torch, live, g17, rows, actions), _steps(torch, made, g17, rows, actions)
        for t, (x, y) in enumerate(zip(a, b)):
            assert all(torch.equal(p, q) for p, q in zip(x[:4], y[:4])), (name, t)
            assert np.array_equal(x[4], y[4]), (name, t)
            assert precision != "f64" or np.array_equal(x[5], y[5]), (name, t)
        made.close()
    live.close()


@pytest.mark.parametrize("precision", ["f64", "mixed"])
@pytest.mark.parametrize("si", [0, 1], ids=STEP_IDS[:2])
def test_episode_kernels_step_like_mn_step_under_other_parameters(torch, si, precision):
    """S1 and S2, n = 67: mn_rollout with given actions for T = 8 = 8 x (step, reset_done), and rollout_policy("APF") = its launch-per-
    step loop (planner_act_batch, step), bit for bit."""
    from distributional_rl_navigation_amd.planners import planner_act_batch
    spec = dict(PS.STEP_SETS[si][1], num_cores=8, num_obs=10, min_start_goal_dis=30.0)
    n, T = 67, 8
    g = torch.Generator(device=DEV); g.manual_seed(5)
    acts = torch.randint(0, 9, (T, n), device=DEV, dtype=torch.int32, generator=g)
    a_env, b_env = make_env(n, precision, spec, seed=9), make_env(n, precision, spec, seed=9)
    assert torch.equal(a_env.reset(), b_env.reset())
    out = a_env.rollout(T, actions=acts, trace=("obs", "reward", "done", "info"))
    for t in range(T):
        o, r, d, i = b_env.step(acts[t])
        assert torch.equal(out["obs"][t], o) and torch.equal(out["reward"][t], r) and torch.equal(out["done"][t], d) and torch.equal(out["info"][t], i), t
        b_env.reset_done()
    assert torch.equal(out["final_obs"], b_env.obs)
    assert all(np.array_equal(x, y) for x, y in zip(a_env.get_state(), b_env.get_state()))
    assert np.array_equal(a_env.peek_next_double(), b_env.peek_next_double())
    if precision == "f64":
        assert np.array_equal(a_env.get_obs64(), b_env.get_obs64())
    # the policy launch, from where the two handles now stand (same worlds, same poses)
    a_tab, w_tab = a_env.params.a[:], a_env.params.w[:]
    tr = a_env.rollout_policy(T, "APF", trace=("obs", "reward", "done", "info", "action"))
    alive = torch.ones(n, dtype=torch.bool, device=DEV)
    obs = b_env.obs.clone()
    for t in range(T):
        act = planner_act_batch(obs, "APF", a_tab, w_tab)
        nobs, rew, done, info = b_env.step(act)
        for k, v in (("action", act), ("reward", rew), ("done", done), ("info", info), ("obs", nobs)):
            assert torch.equal(tr[k][t][alive], v[alive]), (k, t)
        alive = alive & ~done.bool()
        obs = nobs.clone()
    a_env.close(); b_env.close()
