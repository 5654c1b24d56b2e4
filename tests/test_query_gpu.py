"""The query entry points on the device (mn_query_velocity / mn_query_observation, VecMarineNavEnv.velocity_at / observation_at, maps): the HIP arithmetic
against the reference-made fixtures with nothing in between (G4: get_observation at hand-built sonar edge poses, G5: get_velocity samples), against the
step and reset kernels, a numpy twin of the flag bits, shapes and indexing, and the promise that a query writes nothing into the handle.
Float bounds: 1e-9 is the project's float64 bound against the reference; 2e-9 where two sides are each held to 1e-9 of it; 1e-5 for float32 rows."""
import ctypes as C
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

G = os.path.join(os.path.dirname(__file__), "golden")


@pytest.fixture(scope="module")
def torch():
    import torch as t
    if not t.cuda.is_available():
        pytest.skip("no GPU")
    return t


def make_env(n, precision="f64", **kw):
    from distributional_rl_navigation_amd.marinenav_env.vec_env import VecMarineNavEnv
    kw.setdefault("obs64", precision == "f64")
    return VecMarineNavEnv(n, precision=precision, **kw)


def _eval_worlds():
    from distributional_rl_navigation_amd.marinenav_env.vec_env import VecMarineNavEnv
    with open(os.path.join(G, "eval_config_seed3.json")) as f:
        cfg = json.load(f)
    return [VecMarineNavEnv.world_from_eval_config(cfg[f"env_{k}"]) for k in range(len(cfg))]


def _idx(torch, env, values):
    return torch.as_tensor(np.asarray(values, dtype=np.int32), device=env.device)


# ---- G5: get_velocity ---------------------------------------------------------------------------------------------------------------
def test_g5_velocity_on_device(torch):
    z = np.load(os.path.join(G, "g5_velocity.npz"))
    worlds, env_of = [], []
    for i in range(len(z["n"])):      # the samples of one world are consecutive and carry that world's cores
        c = z["cores"][i][:int(z["n"][i])]
        if not worlds or worlds[-1]["cores"].shape != c.shape or not np.array_equal(worlds[-1]["cores"], c):
            worlds.append(dict(cores=c, obstacles=np.zeros((0, 3)), start=[5.0, 5.0], goal=[45.0, 45.0], init_theta=0.0, init_speed=0.0))
        env_of.append(len(worlds) - 1)
    assert len(worlds) == 8 and {len(w["cores"]) for w in worlds} >= {0, 1, 8}
    env = make_env(len(worlds), "f64")
    env.load_worlds(worlds)
    v = env.velocity_at(z["xy"], env=_idx(torch, env, env_of)).cpu().numpy()      # every sample, one call
    err = np.abs(v - z["v"])
    print(f"[g5 on device] {len(err)} samples, worst |v - ref| = {err.max():.3e}")
    assert (err <= 1e-9).all(), err.max()
    env.close()


# ---- G4: get_observation ------------------------------------------------------------------------------------------------------------
def _g4(torch, precision):
    z = np.load(os.path.join(G, "g4_sonar_edge.npz"))
    n = len(z["names"])
    env = make_env(n, precision)
    env.load_worlds([dict(cores=np.zeros((0, 4)), obstacles=z["obs_tab"][i][:int(z["n_obs"][i])], start=z["pose"][i][:2], goal=z["goal"][i],
                          init_theta=float(z["pose"][i][2]), init_speed=1.0) for i in range(n)])
    st = np.concatenate([z["pose"], np.ones((n, 1)), z["vel"]], axis=1)
    idx = _idx(torch, env, np.arange(n))
    o64 = env.observation_at(st, env=idx, velocity="given", dtype=torch.float64).cpu().numpy()
    o32 = env.observation_at(st, env=idx, velocity="given", dtype=torch.float32).cpu().numpy()
    env.close()
    return z, o64, o32


def test_g4_sonar_edge_cases_every_case(torch):
    z, o64, o32 = _g4(torch, "f64")
    err = np.abs(o64 - z["obs"]).max(axis=1)
    worst = int(err.argmax())
    print(f"[g4 on device] {len(err)} cases, worst {err.max():.3e} ({z['names'][worst]})")
    bad = [(str(z["names"][i]), float(err[i])) for i in np.nonzero(~(err <= 1e-9))[0]]
    assert not bad, bad      # every case: tangent, range boundary, the `break` quirk, vertical and near-vertical beams
    assert o32.dtype == np.float32 and np.array_equal(o32, o64.astype(np.float32))
    zm, m64, m32 = _g4(torch, "mixed")      # both precisions read the float64 master tables
    assert np.array_equal(m64, o64) and np.array_equal(m32, o32)


# ---- against the step and reset kernels ---------------------------------------------------------------------------------------------
def test_observation_at_follows_the_step_kernel(torch):
    n = 64
    env = make_env(n, "f64", seed=100)
    env.set_attrs(num_cores=8, num_obs=10, min_start_goal_dis=40.0)
    env.reset()
    idx = _idx(torch, env, np.arange(n))
    checked = 0
    for t in range(1, 41):
        env.step(env.random_actions(5, t - 1))
        env.reset_done()      # finished envs restart: every row is a live pose
        if t in (1, 7, 40):
            st = env.get_state()[0]
            want = env.get_obs64()
            got = env.observation_at(st, env=idx, velocity="given", dtype=torch.float64).cpu().numpy()
            err = np.abs(got - want)
            print(f"[query vs step kernel] step {t}: worst {err.max():.3e}")
            assert (err <= 2e-9).all(), (t, err.max())
            checked += 1
    assert checked == 3
    env.close()


def test_placed_robot_matches_first_observation(torch):
    worlds = _eval_worlds()
    assert len(worlds) == 30
    env = make_env(30, "f64")
    first32 = env.load_worlds(worlds).clone().cpu().numpy()
    first64 = env.get_obs64()
    st = np.array([[w["start"][0], w["start"][1], w["init_theta"], w["init_speed"]] for w in worlds])
    idx = _idx(torch, env, np.arange(30))
    o32 = env.observation_at(st, env=idx, velocity="current").cpu().numpy()
    o64 = env.observation_at(st, env=idx, dtype=torch.float64).cpu().numpy()      # [Q, 4] implies "current"
    print(f"[placed robot] f32 worst {np.abs(o32.astype(np.float64) - first32).max():.3e}, f64 worst {np.abs(o64 - first64).max():.3e}")
    assert (np.abs(o32.astype(np.float64) - first32.astype(np.float64)) <= 1e-5).all()
    assert (np.abs(o64 - first64) <= 2e-9).all()
    env.close()


# ---- flags --------------------------------------------------------------------------------------------------------------------------
def _flags_twin(w, p, x, y):
    f = 0
    o = w["obstacles"]
    if len(o):      # marinenav_env.py:329-336: only the obstacle with the nearest centre, first of equals
        dx, dy = o[:, 0] - x, o[:, 1] - y
        d = np.sqrt(dx * dx + dy * dy)
        k = int(np.argmin(d))
        if d[k] <= o[k, 2] + p.robot_r:
            f |= 1
    if (x < 0.0 or x > p.width) or (y < 0.0 or y > p.height):
        f |= 2
    gx, gy = x - w["goal"][0], y - w["goal"][1]
    if np.sqrt(gx * gx + gy * gy) <= p.goal_dis:
        f |= 4
    return f


def test_flags_against_numpy_twin(torch):
    env = make_env(2, "mixed")
    small, big = (20.0, 20.0, 1.0), (26.0, 20.0, 4.0)
    env.load_worlds([dict(cores=np.zeros((0, 4)), obstacles=np.array([small, big, (40.0, 10.0, 2.0)]), start=[5.0, 5.0], goal=[45.0, 45.0], init_theta=0.0, init_speed=0.0),
                     dict(cores=np.zeros((0, 4)), obstacles=np.zeros((0, 3)), start=[5.0, 5.0], goal=[30.0, 30.0], init_theta=0.0, init_speed=0.0)])
    worlds = env.get_worlds()
    poses = [
        (0, 20.2, 20.0, 1), (0, 21.8, 20.0, None), (0, 21.9, 20.0, 0),      # inside the small obstacle; at / beyond r + robot_r
        (0, 22.5, 20.0, 0),      # the quirk: inside the big obstacle's disc, but the small one's centre is nearer and out of reach
        (0, 24.0, 20.0, 1),      # ... and once the big one's centre is the nearest it counts
        (0, 0.0, 10.0, 0), (0, -1e-9, 10.0, 2), (0, 50.0, 10.0, 0), (0, 50.000001, 10.0, 2),
        (0, 10.0, 0.0, 0), (0, 10.0, -1e-9, 2), (0, 10.0, 50.0, 0), (0, 10.0, 50.000001, 2), (0, -3.0, 60.0, 2),
        (0, 45.0, 43.0, 4), (0, 45.0, 42.999, 0), (0, 44.0, 44.0, 4), (0, 46.5, 46.5, 0),
        (1, 20.2, 20.0, 0), (1, 30.0, 31.0, 4), (1, 30.0, 28.0, 4), (1, 51.0, 30.0, 2), (1, 30.0, 27.9, 0),      # a world without obstacles
    ]
    st = np.array([[x, y, 0.3, 1.0] for _, x, y, _ in poses])
    _, fl = env.observation_at(st, env=_idx(torch, env, [e for e, *_ in poses]), return_flags=True)
    fl = fl.cpu().numpy()
    for (e, x, y, want), got in zip(poses, fl):
        twin = _flags_twin(worlds[e], env.params, x, y)
        assert got == twin, (e, x, y, got, twin)
        if want is not None:
            assert got == want, (e, x, y, got, want)
    env.close()


# ---- shapes and indexing ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def world200(torch):
    """200 generated worlds, 1000 queries aimed at them (env 0 and env n - 1 among them), and every query answered by a call of its own."""
    n, q = 200, 1000
    env = make_env(n, "f64", seed=11)
    env.set_attrs(num_cores=8, num_obs=10, min_start_goal_dis=40.0)
    env.reset()
    rng = np.random.RandomState(4)
    st = np.stack([rng.uniform(0, 50, q), rng.uniform(0, 50, q), rng.uniform(0, 2 * np.pi, q), rng.uniform(0, 2, q)], axis=1)
    idx = rng.randint(n, size=q).astype(np.int32)
    idx[:4] = [0, n - 1, n - 1, 0]
    std = torch.from_numpy(st).to(env.device)
    one_obs, one_fl, one_v = [], [], []
    for k in range(q):
        o, f = env.observation_at(std[k:k + 1], env=int(idx[k]), dtype=torch.float64, return_flags=True)
        one_obs.append(o); one_fl.append(f)
        one_v.append(env.velocity_at(std[k:k + 1, :2], env=int(idx[k])))
    ref = dict(obs=torch.cat(one_obs), flags=torch.cat(one_fl), v=torch.cat(one_v))
    yield env, std, idx, ref
    env.close()


@pytest.mark.parametrize("q", [1, 63, 64, 65, 1000])
def test_batches_equal_single_queries(torch, world200, q):
    env, std, idx, ref = world200
    di = _idx(torch, env, idx[:q])
    o, f = env.observation_at(std[:q], env=di, dtype=torch.float64, return_flags=True)
    assert torch.equal(o, ref["obs"][:q]) and torch.equal(f, ref["flags"][:q])
    assert not torch.isnan(o).any()
    o32 = env.observation_at(std[:q], env=di)
    assert torch.equal(o32, ref["obs"][:q].to(torch.float32))
    assert torch.equal(env.velocity_at(std[:q, :2], env=di), ref["v"][:q])


@pytest.mark.parametrize("e", [0, 199])
def test_one_world_for_all_equals_an_index_per_query(torch, world200, e):
    env, std, idx, ref = world200
    di = _idx(torch, env, np.full(300, e))
    for vel in ("current", "given"):
        a, fa = env.observation_at(std[:300] if vel == "current" else torch.cat([std[:300], std[:300, :2]], dim=1), env=e, velocity=vel, dtype=torch.float64, return_flags=True)
        b, fb = env.observation_at(std[:300] if vel == "current" else torch.cat([std[:300], std[:300, :2]], dim=1), env=di, velocity=vel, dtype=torch.float64, return_flags=True)
        assert torch.equal(a, b) and torch.equal(fa, fb)
    assert torch.equal(env.velocity_at(std[:300, :2], env=e), env.velocity_at(std[:300, :2], env=di))


def test_bad_env_index_inside_a_batch(torch, world200):
    env, std, idx, ref = world200
    q = 130
    bad = idx[:q].copy()
    bad[7], bad[64], bad[129] = -1, 200, 1 << 30
    o, f = env.observation_at(std[:q], env=_idx(torch, env, bad), dtype=torch.float64, return_flags=True)
    o32 = env.observation_at(std[:q], env=_idx(torch, env, bad))
    v = env.velocity_at(std[:q, :2], env=_idx(torch, env, bad))
    ok = np.ones(q, bool); ok[[7, 64, 129]] = False
    okd = torch.from_numpy(ok).to(env.device)
    assert torch.isnan(o[~okd]).all() and torch.isnan(o32[~okd]).all() and torch.isnan(v[~okd]).all()
    assert (f[~okd] == 0x80).all()
    assert torch.equal(o[okd], ref["obs"][:q][okd]) and torch.equal(f[okd], ref["flags"][:q][okd]) and torch.equal(v[okd], ref["v"][:q][okd])
    # the call was MN_OK (no exception) and the handle steps on
    st0 = env.get_state()
    env.step(env.random_actions(1, 0))
    torch.cuda.synchronize()
    assert np.isfinite(env.obs.cpu().numpy()).all()
    env.set_state(*st0)


def test_host_visible_bad_arguments(torch, world200):
    from distributional_rl_navigation_amd import _capi
    env, std, idx, ref = world200
    L, h, s = env.L, env.h, env._stream()
    p = lambda t: C.c_void_p(t.data_ptr())
    xy = std[:8, :2].contiguous()
    st = torch.cat([std[:8], std[:8, :2]], dim=1).contiguous()
    v = torch.empty(8, 2, dtype=torch.float64, device=env.device)
    obs = torch.empty(8, 26, dtype=torch.float32, device=env.device)

    def refused(rc, handle=h):
        assert rc == -1      # MN_ERR_INVALID
        assert len(L.mn_last_error(handle)) > 0

    refused(L.mn_query_velocity(None, None, 0, p(xy), 8, p(v), s), None)
    refused(L.mn_query_velocity(h, None, 0, p(xy), -1, p(v), s))
    refused(L.mn_query_velocity(h, None, 200, p(xy), 8, p(v), s))
    refused(L.mn_query_velocity(h, None, -1, p(xy), 8, p(v), s))
    refused(L.mn_query_velocity(h, None, 0, p(xy), 8, None, s))
    refused(L.mn_query_observation(None, None, 0, p(st), 0, 8, p(obs), None, None, s), None)
    refused(L.mn_query_observation(h, None, 0, p(st), 0, -5, p(obs), None, None, s))
    refused(L.mn_query_observation(h, None, 200, p(st), 0, 8, p(obs), None, None, s))
    refused(L.mn_query_observation(h, None, 0, p(st), 7, 8, p(obs), None, None, s))
    refused(L.mn_query_observation(h, None, 0, p(st), 0, 8, None, None, None, s))
    # Q = 0: MN_OK, nothing launched, nothing needed
    assert L.mn_query_velocity(h, None, 0, None, 0, None, s) == 0
    assert L.mn_query_observation(h, None, 0, None, 1, 0, None, None, None, s) == 0
    assert env.velocity_at(np.zeros((0, 2))).shape == (0, 2) and env.observation_at(np.zeros((0, 4))).shape == (0, 26)
    with pytest.raises(ValueError):
        env.observation_at(np.zeros((3, 4)), velocity="given")
    with pytest.raises(ValueError):
        env.observation_at(np.zeros((3, 4)), env=np.zeros(2, np.int32))
    with pytest.raises(_capi.MarineNavHipError):
        env.velocity_at(np.zeros((3, 2)), env=200)


def test_four_million_queries_take_the_stride_loop(torch, world200):
    """Above 2048 workgroups a lane answers several queries: 2^22 of them against the same queries asked in pieces small enough for one query per lane."""
    env, std, idx, ref = world200
    q, piece = 1 << 22, 1 << 19
    g = torch.Generator(device=env.device); g.manual_seed(3)
    st = torch.rand(q, 4, dtype=torch.float64, device=env.device, generator=g) * torch.tensor([50.0, 50.0, 6.28, 2.0], dtype=torch.float64, device=env.device)
    di = torch.randint(0, 200, (q,), dtype=torch.int32, device=env.device, generator=g)
    v = env.velocity_at(st[:, :2], env=di)
    o, f = env.observation_at(st, env=di, return_flags=True)
    ou, fu = env.observation_at(st, env=199, return_flags=True)
    for lo in range(0, q, piece):
        sl = slice(lo, lo + piece)
        assert torch.equal(v[sl], env.velocity_at(st[sl, :2], env=di[sl]))
        po, pf = env.observation_at(st[sl], env=di[sl], return_flags=True)
        assert torch.equal(o[sl], po) and torch.equal(f[sl], pf)
        po, pf = env.observation_at(st[sl], env=199, return_flags=True)
        assert torch.equal(ou[sl], po) and torch.equal(fu[sl], pf)


# ---- nothing written ----------------------------------------------------------------------------------------------------------------
def _burst(torch, env, rng):
    q = 500
    st = np.stack([rng.uniform(-2, 52, q), rng.uniform(-2, 52, q), rng.uniform(0, 7, q), rng.uniform(0, 2, q), rng.uniform(-1, 1, q), rng.uniform(-1, 1, q)], axis=1)
    di = _idx(torch, env, rng.randint(env.n_envs, size=q))
    for e in (di, 0, env.n_envs - 1):
        env.velocity_at(st[:, :2], env=e)
        env.observation_at(st, env=e, velocity="given", return_flags=True)
        env.observation_at(st[:, :4], env=e, dtype=torch.float64, return_flags=True)


def test_queries_write_nothing_into_the_handle(torch):
    env = make_env(96, "f64", seed=21)
    env.set_attrs(num_cores=6, num_obs=8, min_start_goal_dis=35.0)
    env.reset()
    for t in range(3):
        env.step(env.random_actions(2, t))
    before = (env.get_state(), env.peek_next_double(), env.get_worlds(), env.obs.clone(), env.get_obs64(), env.reward.clone(), env.done.clone(), env.last_done_count())
    _burst(torch, env, np.random.RandomState(8))
    after = (env.get_state(), env.peek_next_double(), env.get_worlds(), env.obs.clone(), env.get_obs64(), env.reward.clone(), env.done.clone(), env.last_done_count())
    for a, b in zip(before[0], after[0]):
        assert np.array_equal(a, b)
    assert np.array_equal(before[1], after[1])
    for wa, wb in zip(before[2], after[2]):
        assert wa.keys() == wb.keys() and all(np.array_equal(wa[k], wb[k]) for k in wa)
    assert torch.equal(before[3], after[3]) and np.array_equal(before[4], after[4])
    assert torch.equal(before[5], after[5]) and torch.equal(before[6], after[6]) and before[7] == after[7]
    env.close()


def test_rollout_unchanged_by_queries_in_between(torch):
    out = []
    for with_queries in (False, True):
        env = make_env(128, "mixed", seed=33)
        env.reset()
        rng = np.random.RandomState(9)
        traces = []
        for part in range(2):
            if with_queries:
                _burst(torch, env, rng)
            tr = env.rollout(5, action_seed=3, first_step=5 * part, trace=("obs", "reward", "done", "info", "action"))
            traces.append({k: v.clone() for k, v in tr.items()})
        if with_queries:
            _burst(torch, env, rng)
        out.append((traces, env.get_state(), env.peek_next_double()))
        env.close()
    (ta, sa, pa), (tb, sb, pb) = out
    for a, b in zip(ta, tb):
        assert a.keys() == b.keys() and all(torch.equal(a[k], b[k]) for k in a)
    assert all(np.array_equal(x, y) for x, y in zip(sa, sb)) and np.array_equal(pa, pb)


# ---- maps on the device -------------------------------------------------------------------------------------------------------------
def test_flow_field_on_device(torch):
    from distributional_rl_navigation_amd import maps
    worlds = _eval_worlds()
    env = make_env(3, "mixed")
    env.load_worlds(worlds[:3])
    xs, ys, v = maps.flow_field(env, env_index=2, nx=100, ny=100)
    pts = np.stack(np.meshgrid(xs, ys, indexing="xy"), axis=-1).reshape(-1, 2)
    want = env.velocity_at(pts, env=_idx(torch, env, np.full(len(pts), 2))).cpu().numpy().reshape(100, 100, 2)
    assert np.array_equal(v, want) and np.isfinite(v).all() and np.abs(v).max() > 0.1
    env.close()


def test_policy_map_on_device(torch):
    from distributional_rl_navigation_amd import maps
    from distributional_rl_navigation_amd.iqn.agent import IQNAgent
    from distributional_rl_navigation_amd.planners import planner_act_batch
    env = make_env(1, "f64")
    env.load_worlds(_eval_worlds()[:1])
    xs, ys, thetas = np.linspace(2.0, 48.0, 8), np.linspace(2.0, 48.0, 8), np.array([0.0, 2.5])
    poses = maps.pose_grid(xs, ys, thetas, 1.0, env.device)
    obs, flags = env.observation_at(poses, env=0, velocity="current", return_flags=True)
    res = maps.policy_map(maps.planner_policy("APF", env.params), env, 0, xs, ys, thetas, 1.0)
    want = planner_act_batch(obs, "APF", env.params.a[:], env.params.w[:]).cpu().numpy()
    assert res["action"].shape == (2, 8, 8) and np.array_equal(res["action"].reshape(-1), want)
    assert np.array_equal(res["flags"].reshape(-1), flags.cpu().numpy()) and len(np.unique(want)) > 1

    def agent():
        a = IQNAgent(26, 9, device="cuda:0", seed=2, BUFFER_SIZE=1024)
        a.load_model(os.path.join(G, "pretrained_IQN_seed3"), "cuda:0")
        return a
    res = maps.policy_map(maps.iqn_policy(agent(), quantiles=True), env, 0, xs, ys, thetas, 1.0)
    cv = torch.full((obs.shape[0],), 1.0, dtype=torch.float32, device=obs.device)
    a, qt, taus = agent().act_eval_batch(obs, 0.0, cv)
    assert np.array_equal(res["action"].reshape(-1), a.cpu().numpy())
    assert np.array_equal(res["q"].reshape(-1, 9), qt.mean(dim=1).cpu().numpy())
    assert np.array_equal(res["taus"].reshape(-1, 32), taus.reshape(-1, 32).cpu().numpy())
    assert res["quantiles"].shape == (2, 8, 8, 32, 9) and np.array_equal(res["quantiles"].reshape(-1, 32, 9), qt.cpu().numpy())
    assert (res["cvar"] == 1.0).all()
    env.close()
