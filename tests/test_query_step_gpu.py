"""The what-if step and the open-loop rollout on the device (mn_query_rollout, VecMarineNavEnv.step_at / rollout_at / constant_rollout_at,
maps.action_fan / lookahead_map, scripts/replay_evaluations.py): the HIP arithmetic against the reference-made fixtures with nothing in between (G3,
G17: single steps; G2, G8: every step of a trace as a what-if step; G6: stored episodes as one launch), a rollout against chained single steps bit for
bit, the mapping, the poison codes, and the promise that nothing in the handle is written.
Float bound: 1e-9, the project's float64 bound against the reference, on every output, the beams included; the G6 returns as tests/test_env_gpu.py
holds them (1e-9, 1e-6 above 600 steps).  The shared helpers (records of a trace, the bound check) are tests/test_query_step_cpu.py's."""
import ctypes as C
import importlib.util
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import params_sets as PS      # noqa: E402
import test_query_step_cpu as H      # noqa: E402

pytestmark = pytest.mark.gpu

G = os.path.join(os.path.dirname(__file__), "golden")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def torch():
    import torch as t
    if not t.cuda.is_available():
        pytest.skip("no GPU")
    return t


def make_env(n, precision="f64", spec=None, **kw):
    from distributional_rl_navigation_amd import _capi
    from distributional_rl_navigation_amd.marinenav_env.vec_env import VecMarineNavEnv
    return VecMarineNavEnv(n, precision=precision, params=PS.apply(_capi.default_params(), spec or {}), **kw)


def _idx(torch, env, values):
    return torch.as_tensor(np.asarray(values, dtype=np.int32), device=env.device)


def _np(out):
    return tuple(out[k].cpu().numpy() for k in ("state", "obs", "reward")) + (out["done"].cpu().numpy().astype(bool), out["info"].cpu().numpy().astype(np.int64))


def _fixture_worlds(z, rows):
    return [dict(cores=z["cores"][i][:z["n"][i][0]], obstacles=z["obs_tab"][i][:z["n"][i][1]], start=z["start"][i], goal=z["goal"][i],
                 init_theta=0.0, init_speed=0.0) for i in rows]


def _single_steps(torch, z, rows, spec, tag, **masks):
    """Fixture rows as ONE step_at call on an f64 and on a mixed handle: the bounds on the first, bit equality on the second."""
    outs = []
    for precision in ("f64", "mixed"):
        env = make_env(len(rows), precision, spec)
        env.load_worlds(_fixture_worlds(z, rows))
        before = env.get_state()
        out = env.step_at(z["state_in"][rows], z["action"][rows], env=_idx(torch, env, np.arange(len(rows))), episode_timesteps=z["ep_t"][rows],
                          dtype=torch.float64)
        outs.append(_np(out))
        assert all(np.array_equal(a, b) for a, b in zip(before, env.get_state()))      # the handle's own robots did not move
        env.close()
    worst = H.check_steps(tag, outs[0], z["state_out"][rows], z["obs"][rows], z["reward"][rows], z["done"][rows], z["info"][rows], **masks)
    for a, b in zip(*outs):
        assert np.array_equal(a, b, equal_nan=True), tag      # both precisions read the float64 master tables
    return worst


def test_g3_single_steps_on_device(torch):
    z = np.load(os.path.join(G, "g3_single_step.npz"))
    assert len(z["action"]) == 2048
    _single_steps(torch, z, np.arange(2048), {}, "g3 device")


@pytest.mark.parametrize("si", range(len(PS.STEP_SETS)), ids=[n for n, _ in PS.STEP_SETS])
def test_g17_single_steps_on_device(torch, si):
    z = np.load(os.path.join(G, "g17_step_params.npz"))
    rows = np.nonzero(z["set"] == si)[0]
    _single_steps(torch, z, rows, PS.STEP_SETS[si][1], f"g17 device {PS.STEP_SETS[si][0]}", beam_ok=z["beam_stable"][rows], info_ok=z["info_stable"][rows])


def _trace_on_device(torch, z, worlds, spec, tag):
    rec, keep, skipped, starts = H.trace_records(z, worlds)
    print(f"[{tag}] {len(keep)} steps, {skipped} skipped (they follow a reset), {starts} episode starts")
    assert skipped == starts
    env = make_env(len(worlds), "f64", spec)
    env.load_worlds([dict(cores=w["cores"], obstacles=w["obstacles"], start=[5.0, 5.0], goal=w["goal"], init_theta=0.0, init_speed=0.0) for w in worlds])
    done = z["done"].astype(bool)
    episode = (np.cumsum(np.concatenate([[True], done[:-1]])) - 1)[keep]
    out = env.step_at(z["state"][keep - 1], z["actions"][keep], env=_idx(torch, env, episode), episode_timesteps=z["ep_t"][keep - 1], dtype=torch.float64)
    H.check_steps(tag, _np(out), z["state"][keep], z["obs"][keep], z["reward"][keep], z["done"][keep], z["info"][keep])
    env.close()


@pytest.mark.parametrize("fn", H.G2_FILES)
def test_g2_traces_step_by_step_on_device(torch, fn):
    z = np.load(os.path.join(G, fn))
    _trace_on_device(torch, z, H.g2_worlds(z), {}, f"{fn} device")


def test_g8_trace_step_by_step_on_device(torch):
    z = np.load(os.path.join(G, "g8_boundary_trace.npz"))
    _trace_on_device(torch, z, H.g8_worlds(z), H.G8_SPEC, "g8 device")


# ---- G6: stored episodes as one launch --------------------------------------------------------------------------------------------------
def _eval_cfg():
    with open(os.path.join(G, "eval_config_seed3.json")) as f:
        return json.load(f)


def _eval_worlds():
    from distributional_rl_navigation_amd.marinenav_env.vec_env import VecMarineNavEnv
    cfg = _eval_cfg()
    return [VecMarineNavEnv.world_from_eval_config(cfg[f"env_{k}"]) for k in range(len(cfg))]


def _start(worlds, which):
    return np.array([[worlds[k]["start"][0], worlds[k]["start"][1], worlds[k]["init_theta"], worlds[k]["init_speed"]] for k in which])


def test_g6_stored_episodes_as_one_rollout(torch):
    from distributional_rl_navigation_amd.episodes import energy_table, tally
    z = np.load(os.path.join(G, "g6_pretrained_replay.npz"))
    world = np.concatenate([z["greedy_ids"][:, 1], z["adaptive_ids"][:, 1]])
    L = np.concatenate([z["greedy_len"], z["adaptive_len"]])
    acts = np.concatenate([z["greedy_actions"], z["adaptive_actions"]])
    success = np.concatenate([z["greedy_success"], z["adaptive_success"]])
    times = np.concatenate([z["greedy_time"], z["adaptive_time"]])
    stored = np.concatenate([z["greedy_reward"], z["adaptive_reward"]])
    assert len(L) == 36
    worlds = _eval_worlds()
    env = make_env(len(worlds), "f64")
    env.load_worlds(worlds)
    hmax = int(L.max())
    out = env.rollout_at(_start(worlds, world), np.where(acts[:, :hmax] >= 0, acts[:, :hmax], 0), lengths=L, env=_idx(torch, env, world),
                         trace=("reward", "done", "info", "action"), dtype=torch.float64)      # ONE launch, ragged lengths
    steps, info = out["steps"].cpu().numpy(), out["info"].cpu().numpy()
    assert np.array_equal(steps, L)
    assert np.array_equal(info == 4, success)
    np.testing.assert_allclose(0.1 * 10 * steps, times, atol=1e-9)
    t = tally(out["reward_trace"].cpu().numpy(), out["done_trace"].cpu().numpy(), out["info_trace"].cpu().numpy(), out["action_trace"].cpu().numpy(),
              0.99, energy_table(env.params.a[:], env.params.w[:]))
    # an episode the reference cut at 1000 steps is not done: behind its last step the trace says done, so tally counts one filler row of reward 0
    ended = out["done"].cpu().numpy().astype(bool)
    assert np.array_equal(t["length"], np.where(ended, L, np.minimum(L + 1, hmax)))
    err = np.abs(t["ret"] - stored)
    tol = np.where(L > 600, 1e-6, 1e-9)
    print(f"[g6 device] 36 episodes, {int(L.sum())} steps; worst |return - stored| {err[L <= 600].max():.3e} up to 600 steps, {err[L > 600].max(initial=0.0):.3e} above")
    assert (err <= tol).all(), (float(err.max()), np.nonzero(err > tol)[0])
    for i in range(36):
        assert t["actions"][i][:L[i]] == acts[i, :L[i]].tolist()
    env.close()


# ---- a rollout equals chained single steps ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def world64(torch):
    """64 generated worlds (8 cores, 10 obstacles) and 300 queries aimed at them: live poses, with obstacles and goals in reach of a few steps."""
    n, q = 64, 300
    env = make_env(n, "f64", seed=17)
    env.set_attrs(num_cores=8, num_obs=10, min_start_goal_dis=30.0)
    env.reset()
    rng = np.random.RandomState(5)
    ws = env.get_worlds()
    idx = rng.randint(n, size=q).astype(np.int32)
    idx[:2] = [0, n - 1]
    st = np.stack([rng.uniform(0, 50, q), rng.uniform(0, 50, q), rng.uniform(0, 2 * np.pi, q), rng.uniform(0, 2, q)], axis=1)
    for k in range(0, q, 3):      # a third of the queries starts a few metres from its goal or from an obstacle: rollouts that end early
        w = ws[idx[k]]
        c = w["goal"] if k % 2 else w["obstacles"][k % len(w["obstacles"])][:2]
        st[k, :2] = c + rng.uniform(-5, 5, 2)
    yield env, torch.from_numpy(st).to(env.device), idx, rng
    env.close()


TRACES = ("reward", "done", "info", "action", "state", "traj")


def _chain(torch, env, st, env_arg, actions_of_step, n_steps, lengths, ep0):
    """n_steps chained step_at calls, each fed the previous state and counter; a query that is done (or at its length) is carried along unchanged."""
    q = st.shape[0]
    dev = env.device
    state = torch.cat([st, st.new_zeros(q, 2)], dim=1) if st.shape[1] == 4 else st.clone()
    first = env.observation_at(state, env=env_arg, velocity="given", dtype=torch.float64)
    fin = dict(state=state.clone(), obs=first, reward=torch.zeros(q, dtype=torch.float64, device=dev), done=torch.zeros(q, dtype=torch.uint8, device=dev),
               info=torch.zeros(q, dtype=torch.uint8, device=dev), steps=torch.zeros(q, dtype=torch.int32, device=dev))
    rows = []
    for t in range(n_steps):
        live = (fin["done"] == 0) & (t < lengths)
        o = env.step_at(fin["state"], actions_of_step(t), env=env_arg, episode_timesteps=ep0 + t, dtype=torch.float64)
        for k in ("state", "obs", "reward", "done", "info"):
            fin[k] = torch.where(live.reshape((-1,) + (1,) * (o[k].dim() - 1)), o[k], fin[k])
        fin["steps"] = torch.where(live, torch.full_like(fin["steps"], t + 1), fin["steps"])
        rows.append(dict(reward=torch.where(live, o["reward"], torch.zeros_like(o["reward"])), done=torch.where(live, o["done"], torch.ones_like(o["done"])),
                         info=fin["info"].clone(), action=torch.where(live, actions_of_step(t), torch.full_like(actions_of_step(t), -1)),
                         state=fin["state"].clone(), live=live))
    return fin, rows


@pytest.mark.parametrize("form", ["shared", "constant", "per_query"])
@pytest.mark.parametrize("n_steps", [1, 7, 64])
def test_rollout_equals_chained_steps(torch, world64, n_steps, form):
    env, std, idx, _ = world64
    q = std.shape[0]
    di = _idx(torch, env, idx)
    rng = np.random.RandomState(100 + n_steps)
    lengths = torch.from_numpy(rng.randint(0, n_steps + 1, size=q).astype(np.int32)).to(env.device)
    lengths[:8] = n_steps
    ep0 = torch.from_numpy(rng.choice([0, 3, 990, 1000 - n_steps // 2], size=q).astype(np.int32)).to(env.device)      # some reach the 1000-step rule inside
    if form == "shared":
        seq = torch.from_numpy(rng.randint(9, size=n_steps).astype(np.int32)).to(env.device)
        out = env.rollout_at(std, seq, lengths=lengths, env=di, episode_timesteps=ep0, trace=TRACES, dtype=torch.float64)
        act = lambda t: seq[t].expand(q).contiguous()
    elif form == "constant":
        a = torch.from_numpy(rng.randint(9, size=q).astype(np.int32)).to(env.device)
        out = env.constant_rollout_at(std, a, n_steps, lengths=lengths, env=di, episode_timesteps=ep0, trace=TRACES, dtype=torch.float64)
        act = lambda t: a
    else:
        seq = torch.from_numpy(rng.randint(9, size=(q, n_steps)).astype(np.int32)).to(env.device)
        out = env.rollout_at(std, seq, lengths=lengths, env=di, episode_timesteps=ep0, trace=TRACES, dtype=torch.float64)
        act = lambda t: seq[:, t].contiguous()
    fin, rows = _chain(torch, env, std, di, act, n_steps, lengths, ep0)
    for k in ("state", "obs", "reward", "done", "info", "steps"):
        assert torch.equal(out[k], fin[k]), (k, n_steps, form)
    assert not torch.isnan(out["state"]).any() and not torch.isnan(out["obs"]).any()
    for t, row in enumerate(rows):
        for k in ("reward", "done", "info", "action", "state"):
            assert torch.equal(out[k + "_trace"][t], row[k]), (k, t, n_steps, form)
        assert torch.isnan(out["traj_trace"][t][~row["live"]]).all()
        live = row["live"]
        assert torch.equal(out["traj_trace"][t][live][:, -1], row["state"][live][:, :2])      # the last sub-step's position is the step's
    assert int((out["steps"] < lengths).sum()) > 0 or n_steps == 1      # some rollouts ended before their length
    assert out["traj_trace"].shape == (n_steps, q, 10, 2)


def test_zero_length_returns_the_input(torch, world64):
    env, std, idx, _ = world64
    st6 = torch.cat([std[:40], std[:40, :2] * 0.01], dim=1)
    out = env.rollout_at(st6, torch.zeros(5, dtype=torch.int32), lengths=0, env=_idx(torch, env, idx[:40]), dtype=torch.float64)
    assert torch.equal(out["state"], st6) and (out["steps"] == 0).all() and (out["done"] == 0).all() and (out["info"] == 0).all() and (out["reward"] == 0).all()
    assert torch.equal(out["obs"], env.observation_at(st6, env=_idx(torch, env, idx[:40]), velocity="given", dtype=torch.float64))


# ---- mapping ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("q", [1, 65, 257])
def test_batches_equal_single_queries(torch, world64, q):
    env, std, idx, _ = world64
    a = torch.arange(q, dtype=torch.int32, device=env.device) % 9
    out = env.step_at(std[:q], a, env=_idx(torch, env, idx[:q]), dtype=torch.float64)
    o32 = env.step_at(std[:q], a, env=_idx(torch, env, idx[:q]))
    for k in range(q):
        one = env.step_at(std[k:k + 1], int(a[k]), env=int(idx[k]), dtype=torch.float64)      # a shared one-step sequence, one world for all
        for name in ("state", "obs", "reward", "done", "info"):
            assert torch.equal(out[name][k:k + 1], one[name]), (name, k)
    assert o32["obs"].dtype == torch.float32 and torch.equal(o32["obs"], out["obs"].to(torch.float32)) and torch.equal(o32["state"], out["state"])


def test_half_a_million_queries_take_the_stride_loop(torch, world64):
    env, std, idx, _ = world64
    q, piece = 2048 * 256 + 3, 1 << 17
    g = torch.Generator(device=env.device); g.manual_seed(3)
    st = torch.rand(q, 4, dtype=torch.float64, device=env.device, generator=g) * torch.tensor([50.0, 50.0, 6.28, 2.0], dtype=torch.float64, device=env.device)
    di = torch.randint(0, env.n_envs, (q,), dtype=torch.int32, device=env.device, generator=g)
    a = torch.randint(0, 9, (q,), dtype=torch.int32, device=env.device, generator=g)
    whole, uni = env.step_at(st, a, env=di), env.step_at(st, a, env=63)
    for lo in range(0, q, piece):
        sl = slice(lo, lo + piece)
        part, upart = env.step_at(st[sl], a[sl], env=di[sl]), env.step_at(st[sl], a[sl], env=63)
        for name in ("state", "obs", "reward", "done", "info"):
            assert torch.equal(whole[name][sl], part[name]) and torch.equal(uni[name][sl], upart[name]), (name, lo)


@pytest.mark.parametrize("e", [0, 63])
def test_one_world_for_all_equals_an_index_per_query(torch, world64, e):
    env, std, idx, _ = world64
    q = std.shape[0]
    seq = torch.arange(q * 5, dtype=torch.int32, device=env.device).reshape(q, 5) % 9
    a = env.rollout_at(std, seq, env=e, trace=TRACES, dtype=torch.float64)
    b = env.rollout_at(std, seq, env=_idx(torch, env, np.full(q, e)), trace=TRACES, dtype=torch.float64)
    assert a.keys() == b.keys()
    for k in a:
        assert torch.equal(torch.nan_to_num(a[k].to(torch.float64), nan=-7.0), torch.nan_to_num(b[k].to(torch.float64), nan=-7.0)), k


# ---- refusals and poison ----------------------------------------------------------------------------------------------------------------
def test_poison_stays_in_its_own_query(torch, world64):
    from distributional_rl_navigation_amd import _capi
    env, std, idx, _ = world64
    q, hmax = 130, 4
    seq = (torch.arange(q * hmax, dtype=torch.int32, device=env.device).reshape(q, hmax) * 5) % 9
    di = _idx(torch, env, idx[:q])
    ref = env.rollout_at(std[:q], seq, env=di, trace=TRACES, dtype=torch.float64)
    bad_env, st, acts = idx[:q].copy(), std[:q].clone(), seq.clone()
    bad_env[7], bad_env[64] = -1, 64
    st[20, 0] = float("nan"); st[21, 1] = float("inf"); st[22, 2] = 1.0e6; st[23, 2] = -2.0e6; st[24, 3] = float("-inf")
    acts[40, 0] = 9; acts[41, 2] = -1      # the second one after two good steps
    out = env.rollout_at(st, acts, env=_idx(torch, env, bad_env), trace=TRACES, dtype=torch.float64)      # MN_OK: no exception
    hit = [7, 64, 20, 21, 22, 23, 24, 40, 41]
    ok = np.ones(q, bool); ok[hit] = False
    okd = torch.from_numpy(ok).to(env.device)
    for k in out:
        a, b = out[k], ref[k]
        sel = (lambda t: t[okd]) if not k.endswith("_trace") else (lambda t: t[:, okd])
        assert torch.equal(torch.nan_to_num(sel(a).to(torch.float64), nan=-7.0), torch.nan_to_num(sel(b).to(torch.float64), nan=-7.0)), k
    for i in hit:
        assert torch.isnan(out["state"][i]).all() and torch.isnan(out["obs"][i]).all() and torch.isnan(out["reward"][i]) and out["done"][i] == 1, i
    for i in (7, 64):
        assert out["info"][i] == _capi.QUERY_FLAG_BAD_ENV and out["steps"][i] == 0
        assert (out["info_trace"][:, i] == _capi.QUERY_FLAG_BAD_ENV).all() and (out["done_trace"][:, i] == 1).all() and (out["action_trace"][:, i] == -1).all()
        assert (out["reward_trace"][:, i] == 0).all()
    for i in (20, 21, 22, 23, 24, 40):
        assert out["info"][i] == _capi.QUERY_INFO_BAD_STATE and out["steps"][i] == 1
        assert torch.isnan(out["reward_trace"][0, i]) and out["done_trace"][0, i] == 1 and out["action_trace"][0, i] == acts[i, 0]
        assert (out["reward_trace"][1:, i] == 0).all() and (out["action_trace"][1:, i] == -1).all()
    if ref["steps"][41] >= 3:      # the query was alive when the bad action came
        assert out["info"][41] == _capi.QUERY_INFO_BAD_STATE and out["steps"][41] == 3
        assert torch.equal(out["reward_trace"][:2, 41], ref["reward_trace"][:2, 41]) and torch.isnan(out["reward_trace"][2, 41])
    else:
        assert torch.equal(out["steps"][41], ref["steps"][41])
    assert int(ref["steps"][41]) >= 3 or int(ref["steps"][40]) >= 1
    # |theta| just inside the bound is stepped: the loop wraps it as the reference's does
    near = std[:4].clone(); near[:, 2] = torch.tensor([999999.5, -999999.5, 123456.789, -6.5], dtype=torch.float64)
    o = env.step_at(near, 4, env=0, dtype=torch.float64)
    assert torch.isfinite(o["state"]).all() and (o["state"][:, 2] >= 0).all() and (o["state"][:, 2] < 2 * np.pi).all() and (o["info"] <= 4).all()


def test_host_visible_refusals(torch, world64):
    from distributional_rl_navigation_amd import _capi
    env, std, idx, _ = world64
    L, h, s = env.L, env.h, env._stream()
    p = lambda t: C.c_void_p(t.data_ptr())
    st = torch.cat([std[:8], std[:8, :2]], dim=1).contiguous()
    act = torch.zeros(8, dtype=torch.int32, device=env.device)
    so = torch.empty(8, 6, dtype=torch.float64, device=env.device)
    none13 = [None] * 13

    def call(handle=h, env0=0, state=p(st), mode=_capi.QUERY_ACTIONS_CONSTANT, actions=p(act), n_steps=1, nq=8, outs=None):
        outs = outs if outs is not None else [p(so)] + [None] * 12
        return L.mn_query_rollout(handle, None, env0, state, None, mode, actions, n_steps, None, nq, *outs, s)

    def refused(rc, handle=h):
        assert rc == -1 and len(L.mn_last_error(handle)) > 0

    assert call() == 0
    refused(call(handle=None), None)
    refused(call(nq=-1))
    refused(call(env0=64)); refused(call(env0=-1))
    refused(call(outs=none13))
    refused(call(mode=3)); refused(call(mode=-1))
    refused(call(n_steps=-1)); refused(call(n_steps=_capi.QUERY_MAX_STEPS + 1))
    refused(call(state=None)); refused(call(actions=None))
    assert call(nq=0, state=None, actions=None, outs=none13) == 0      # Q = 0: MN_OK, nothing launched, nothing needed
    assert env.step_at(np.zeros((0, 4)), np.zeros(0, np.int32))["obs"].shape == (0, 26)
    with pytest.raises(ValueError):
        env.rollout_at(np.zeros((3, 4)), np.zeros((2, 5), np.int32))
    with pytest.raises(ValueError):
        env.rollout_at(np.zeros((3, 4)), np.zeros(5, np.int32), trace=("obs",))
    with pytest.raises(ValueError):
        env.step_at(np.zeros((3, 4)), np.zeros(3, np.int32), env=np.zeros(2, np.int32))
    with pytest.raises(_capi.MarineNavHipError):
        env.step_at(np.zeros((3, 4)), 0, env=64)


# ---- nothing written --------------------------------------------------------------------------------------------------------------------
def _burst(torch, env, rng):
    q = 400
    st = np.stack([rng.uniform(-2, 52, q), rng.uniform(-2, 52, q), rng.uniform(0, 7, q), rng.uniform(0, 2, q), rng.uniform(-1, 1, q), rng.uniform(-1, 1, q)], axis=1)
    di = _idx(torch, env, rng.randint(env.n_envs, size=q))
    for e in (di, 0, env.n_envs - 1):
        env.step_at(st, rng.randint(9, size=q).astype(np.int32), env=e, episode_timesteps=rng.randint(1002, size=q))
        env.rollout_at(st[:, :4], rng.randint(9, size=(q, 6)).astype(np.int32), lengths=rng.randint(7, size=q), env=e, trace=TRACES, dtype=torch.float64)
        env.constant_rollout_at(st, rng.randint(9, size=q).astype(np.int32), 3, env=e)


def test_rollouts_write_nothing_into_the_handle(torch):
    env = make_env(96, "f64", seed=21)
    env.set_attrs(num_cores=6, num_obs=8, min_start_goal_dis=35.0)
    env.reset()
    for t in range(3):
        env.step(env.random_actions(2, t))
    before = env.save_state().clone()
    obs, reward, done = env.obs.clone(), env.reward.clone(), env.done.clone()
    _burst(torch, env, np.random.RandomState(8))
    assert torch.equal(before, env.save_state())      # byte for byte: pose, counters, tables, RNG rows, done queue
    assert torch.equal(obs, env.obs) and torch.equal(reward, env.reward) and torch.equal(done, env.done)
    env.close()


def test_mn_rollout_unchanged_by_rollout_queries_in_between(torch):
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


# ---- maps and the replay script ---------------------------------------------------------------------------------------------------------
def test_action_fan_on_device(torch):
    from distributional_rl_navigation_amd import maps
    worlds = _eval_worlds()
    env = make_env(2, "mixed")
    env.load_worlds(worlds[:2])
    state = _start(worlds, [1])[0]
    fan = maps.action_fan(env, 1, state, 12)
    assert fan["trajectory"].shape == (9, 120, 2) and fan["reward"].shape == (9, 12) and fan["steps"].shape == (9,)
    for a in range(9):
        one = env.constant_rollout_at(state[None], [a], 12, env=1, trace=("state",), dtype=torch.float64)
        n = int(one["steps"][0])
        assert n == fan["steps"][a] and np.array_equal(fan["state"][a], one["state"][0].cpu().numpy())
        per_step = fan["trajectory"][a].reshape(12, 10, 2)
        assert np.array_equal(per_step[:n, -1], one["state_trace"][:n, 0, :2].cpu().numpy()) and np.isnan(per_step[n:]).all()
    assert len({tuple(np.round(fan["state"][a][:4], 6)) for a in range(9)}) == 9      # nine different end states
    env.close()


def test_lookahead_map_on_device(torch):
    from distributional_rl_navigation_amd import maps
    from distributional_rl_navigation_amd.dqn.policy import DQNPolicy
    pol = DQNPolicy.load(os.path.join(G, "pretrained_DQN_seed3", "q_net.npz"), device="cuda:0")
    env = make_env(1, "f64")
    env.load_worlds(_eval_worlds()[:1])
    xs, ys, thetas = np.linspace(3.0, 47.0, 7), np.linspace(3.0, 47.0, 6), np.array([0.5, 3.0])
    res = maps.lookahead_map(maps.dqn_policy(pol, q=True), env, 0, xs, ys, thetas, 1.0, chunk=100)
    assert res["backup"].shape == (2, 6, 7, 9) and res["q"].shape == (2, 6, 7, 9)
    poses = maps.pose_grid(xs, ys, thetas, 1.0, env.device)
    obs, flags = env.observation_at(poses, env=0, velocity="current", return_flags=True)
    q = pol.q_values(obs).cpu().numpy()
    assert np.array_equal(res["q"].reshape(-1, 9), q) and np.array_equal(res["flags"].reshape(-1), flags.cpu().numpy())
    assert np.array_equal(res["action"].reshape(-1), q.argmax(axis=1))
    gamma = float(env.discount)
    assert gamma == 0.99
    backup = np.zeros((len(poses), 9))
    for k in range(len(poses)):      # pose by pose
        for a in range(9):
            o = env.step_at(poses[k:k + 1], a, env=0)
            qn = pol.q_values(o["obs"]).cpu().numpy().astype(np.float64)
            backup[k, a] = float(o["reward"][0]) + gamma * (1.0 - float(o["done"][0])) * qn.max()
            assert res["reward_next"].reshape(-1, 9)[k, a] == float(o["reward"][0]) and res["done_next"].reshape(-1, 9)[k, a] == int(o["done"][0])
            assert res["info_next"].reshape(-1, 9)[k, a] == int(o["info"][0])
    # the network's rows do not depend on the batch they are in beyond float32 rounding of a row's own arithmetic: same kernel, same row
    assert np.array_equal(res["backup"].reshape(-1, 9), backup)
    assert np.array_equal(res["residual"], res["backup"] - res["q"].astype(np.float64))
    assert np.array_equal(res["lookahead_action"].reshape(-1), backup.argmax(axis=1))
    with pytest.raises(ValueError):
        maps.lookahead_map(maps.planner_policy("APF", env.params), env, 0, xs, ys, thetas, 1.0)
    env.close()


def test_replay_evaluations_script_on_the_g6_subset(torch, tmp_path, capsys):
    spec = importlib.util.spec_from_file_location("replay_evaluations", os.path.join(ROOT, "scripts", "replay_evaluations.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    z = np.load(os.path.join(G, "g6_pretrained_replay.npz"))
    for policy in ("greedy", "adaptive"):
        out = str(tmp_path / f"{policy}.npz")
        mod.main(["--config", os.path.join(G, "eval_config_seed3.json"), "--evaluations", os.path.join(G, "g6_pretrained_replay.npz"), "--subset", policy,
                  "--substeps", "--out", out])
        text = capsys.readouterr().out
        print(text)
        worst = float(text.split("largest |recomputed - stored return| = ")[1].split()[0])
        L = z[f"{policy}_len"]
        assert "success flags that differ: 0" in text and "differ from the stored length in 0" in text
        r = np.load(out)
        assert np.array_equal(r["steps"], L) and np.array_equal(r["success"], z[f"{policy}_success"]) and r["xy"].shape == (18, int(L.max()), 2)
        assert r["traj"].shape == (18, int(L.max()) * 10, 2)
        err = np.abs(r["ret"] - z[f"{policy}_reward"])
        assert worst == pytest.approx(err.max(), rel=1e-3) and (err <= np.where(L > 600, 1e-6, 1e-9)).all(), (worst, err.max())
        np.testing.assert_allclose(r["energy"], z[f"{policy}_energy"], atol=1e-4)
        assert np.isfinite(r["xy"][0, :L[0]]).all() and np.isnan(r["xy"][0, L[0]:]).all()
