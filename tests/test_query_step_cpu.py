"""The what-if step (mn_query_rollout, csrc/mn_query_step_body.h) as far as it goes without a GPU: the C-ABI declaration and its ctypes binding, the
compiled resources of the kernels (hipcc cross-compiles gfx950), the step body itself -- it is __host__ __device__, so tests/query_step_host.hip runs
it on the CPU -- against the reference-made fixtures G3, G17, G2 and G8, and the bookkeeping of maps.lookahead_map with stand-ins for the device calls.
Float bound: 1e-9, the project's float64 bound against the reference, on EVERY output, the beams included (the body is the reference's own slope form,
as observation_at's, which meets 1e-9 on G4); only g17's own `beam_stable` / `info_stable` masks leave anything out."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import params_sets as PS      # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "distributional_rl_navigation_amd", "csrc")
G = os.path.join(ROOT, "tests", "golden")
HIPCC = "/opt/rocm/bin/hipcc"
G2_FILES = ("g2_trace_seed0_default.npz", "g2_trace_seed1_stage0.npz", "g2_trace_seed2_stage2.npz", "g2_trace_seed5_schedule.npz")


def _header():
    with open(os.path.join(ROOT, "include", "marinenav_hip.h")) as f:
        return f.read()


def test_rollout_symbol_declared_and_bound():
    from distributional_rl_navigation_amd import _capi
    text = _header()
    m = re.search(r"\bint mn_query_rollout\(([^;]*)\);", text)
    assert m, "mn_query_rollout is not declared in include/marinenav_hip.h"
    assert [re.sub(r"\s+", " ", a).strip() for a in m.group(1).split(",")] == [
        "mn_handle *h", "const int32_t *env_of_query_dev", "int32_t env0", "const double *state_dev", "const int32_t *episode_timesteps_dev",
        "int32_t action_mode", "const int32_t *actions_dev", "int32_t n_steps", "const int32_t *n_steps_of_query_dev", "int64_t n_queries",
        "double *state_out_dev", "float *obs_dev", "double *obs64_dev", "double *reward_dev", "uint8_t *done_dev", "uint8_t *info_dev", "int32_t *steps_dev",
        "double *reward_trace_dev", "uint8_t *done_trace_dev", "uint8_t *info_trace_dev", "int32_t *action_trace_dev", "double *state_trace_dev",
        "double *traj_trace_dev", "void *stream"]
    sig = {n: (r, a) for n, r, a in _capi.SIGNATURES}
    p, i32, i64 = C.c_void_p, C.c_int32, C.c_int64
    assert sig["mn_query_rollout"] == (C.c_int, [p, p, i32, p, p, i32, p, i32, p, i64] + [p] * 14)
    for name, value in (("MN_QUERY_ACTIONS_SHARED", _capi.QUERY_ACTIONS_SHARED), ("MN_QUERY_ACTIONS_CONSTANT", _capi.QUERY_ACTIONS_CONSTANT),
                        ("MN_QUERY_ACTIONS_PER_QUERY", _capi.QUERY_ACTIONS_PER_QUERY), ("MN_QUERY_INFO_BAD_STATE", _capi.QUERY_INFO_BAD_STATE)):
        m = re.search(name + r" = (\d+)", text)
        assert m and int(m.group(1)) == value, name
    m = re.search(r"#define MN_QUERY_MAX_STEPS (\d+)", text)
    assert m and int(m.group(1)) == _capi.QUERY_MAX_STEPS
    # the poison codes are no MN_INFO_* code and differ from each other
    assert _capi.QUERY_INFO_BAD_STATE > 4 and _capi.QUERY_INFO_BAD_STATE != _capi.QUERY_FLAG_BAD_ENV and _capi.QUERY_INFO_BAD_STATE < 256


def test_rollout_kernels_use_no_scratch_and_no_lds():
    """One lane per query, nothing shared, no indexed private array: scratch 0, VGPR spills 0, LDS 0, at most 256 registers.  The message carries the
    figures DESIGN records."""
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-I../../include", "-I.", "--cuda-device-only", "-ffp-contract=off",
                        "-Rpass-analysis=kernel-resource-usage", "-c", "-o", "/dev/null", "mn_query_step.hip"], cwd=CSRC, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    usage, cur = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"remark: .*Function Name: (\S+)", line)
        if m:
            cur = usage.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:.*?\s([A-Za-z][A-Za-z ]*?)(?: \[[^\]]*\])?: (\d+)", line)
        if m and cur is not None:
            cur[m.group(1).strip()] = int(m.group(2))
    ker = {k: v for k, v in usage.items() if "mn_query_rollout_kernel" in k}
    assert len(ker) == 2 and len(usage) == 2, list(usage)      # <UNIFORM> and nothing else
    figures = "; ".join(f"{k}: VGPRs {v['VGPRs']}, SGPRs {v['TotalSGPRs']}, LDS {v['LDS Size']}, scratch {v['ScratchSize']}" for k, v in ker.items())
    print(figures)
    for v in ker.values():
        assert v["ScratchSize"] == 0 and v["LDS Size"] == 0 and v["VGPRs Spill"] == 0, figures
        assert v["VGPRs"] + v.get("AGPRs", 0) <= 256, figures


# ---- the step body on the CPU -----------------------------------------------------------------------------------------------------------
RECORD = np.dtype([("nc", "<i4"), ("no", "<i4"), ("action", "<i4"), ("ep_t", "<i4"), ("cores", "<f8", (8, 3)), ("obst", "<f8", (10, 3)),
                   ("goal", "<f8", (2,)), ("state", "<f8", (6,))])
assert RECORD.itemsize == 16 + 8 * (24 + 30 + 2 + 6)


@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    exe = str(tmp_path_factory.mktemp("query_step_host") / "query_step_host")
    r = subprocess.run([HIPCC, "--cuda-host-only", "-O2", "-std=c++17", "-ffp-contract=off", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC,
                        "-o", exe, os.path.join(ROOT, "tests", "query_step_host.hip")], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def signed_cores(cores4):
    """[.., 4] = x, y, clockwise, Gamma -> [.., 3] = x, y, +Gamma if clockwise else -Gamma (the master tables' form)."""
    c = np.asarray(cores4, dtype=np.float64)
    return np.concatenate([c[..., :2], np.where(c[..., 2:3] > 0, c[..., 3:4], -c[..., 3:4])], axis=-1)


def records(cores4, n_cores, obst, n_obs, goal, state, action, ep_t):
    n = len(action)
    rec = np.zeros(n, dtype=RECORD)
    rec["nc"], rec["no"], rec["action"], rec["ep_t"] = n_cores, n_obs, action, ep_t
    rec["cores"], rec["obst"], rec["goal"] = signed_cores(cores4), obst, goal
    st = np.asarray(state, dtype=np.float64)
    rec["state"][:, :st.shape[1]] = st
    return rec


def run_host(exe, tmp_path, spec, rec, tag):
    """The body's (state [n, 6], obs [n, 26], reward, done, info) for the records under the parameters `spec` (a params_sets dict)."""
    from distributional_rl_navigation_amd import _capi
    p = PS.apply(_capi.default_params(), spec)
    fin, fout = str(tmp_path / f"{tag}.in"), str(tmp_path / f"{tag}.out")
    with open(fin, "wb") as f:
        f.write(np.array([len(rec), 0], dtype="<i4").tobytes())
        f.write(bytes(p))
        f.write(rec.tobytes())
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    out = np.fromfile(fout, dtype="<f8").reshape(len(rec), 35)
    return out[:, :6], out[:, 6:32], out[:, 32], out[:, 33].astype(bool), out[:, 34].astype(np.int64)


def check_steps(tag, got, ref_state, ref_obs, ref_reward, ref_done, ref_info, beam_ok=None, info_ok=None):
    """done / info equal; state, reward, the observation's head and every beam within 1e-9.  Prints the worst figures before it asserts."""
    state, obs, reward, done, info = got
    n = len(ref_info)
    info_ok = np.ones(n, bool) if info_ok is None else info_ok
    beam_ok = np.ones((n, 11), bool) if beam_ok is None else beam_ok
    e_state = np.abs(state - ref_state).max()
    e_head = np.abs(obs[:, :4] - ref_obs[:, :4]).max()
    e_rew = np.abs(reward - ref_reward)[info_ok].max()
    e_beam = np.abs(obs[:, 4:] - ref_obs[:, 4:])
    e_beam[~np.repeat(beam_ok, 2, axis=1)] = 0.0
    print(f"[{tag}] {n} steps: worst state {e_state:.3e}, head {e_head:.3e}, reward {e_rew:.3e}, beam {e_beam.max():.3e}; "
          f"left out: {int((~info_ok).sum())} info, {int((~beam_ok).sum())} beams")
    assert np.array_equal(done[info_ok], np.asarray(ref_done, bool)[info_ok]) and np.array_equal(info[info_ok], ref_info[info_ok]), tag
    assert np.array_equal(PS.miss(obs)[beam_ok], PS.miss(ref_obs)[beam_ok]), tag
    assert e_state <= 1e-9 and e_head <= 1e-9 and e_rew <= 1e-9, (tag, e_state, e_head, e_rew)
    assert (e_beam <= 1e-9).all(), (tag, float(e_beam.max()), np.argwhere(e_beam > 1e-9)[:5])
    return max(e_state, e_head, e_rew, float(e_beam.max()))


def test_g3_single_steps_on_the_host(host_program, tmp_path):
    z = np.load(os.path.join(G, "g3_single_step.npz"))
    assert len(z["action"]) == 2048
    rec = records(z["cores"], z["n"][:, 0], z["obs_tab"], z["n"][:, 1], z["goal"], z["state_in"], z["action"], z["ep_t"])
    check_steps("g3 host", run_host(host_program, tmp_path, {}, rec, "g3"), z["state_out"], z["obs"], z["reward"], z["done"], z["info"])


@pytest.mark.parametrize("si", range(len(PS.STEP_SETS)), ids=[n for n, _ in PS.STEP_SETS])
def test_g17_single_steps_on_the_host(host_program, tmp_path, si):
    z = np.load(os.path.join(G, "g17_step_params.npz"))
    spec = PS.STEP_SETS[si][1]
    rows = np.nonzero(z["set"] == si)[0]
    assert len(rows) == 256
    rec = records(z["cores"][rows], z["n"][rows][:, 0], z["obs_tab"][rows], z["n"][rows][:, 1], z["goal"][rows], z["state_in"][rows], z["action"][rows],
                  z["ep_t"][rows])
    check_steps(f"g17 host {PS.STEP_SETS[si][0]}", run_host(host_program, tmp_path, spec, rec, "g17"), z["state_out"][rows], z["obs"][rows],
                z["reward"][rows], z["done"][rows], z["info"][rows], beam_ok=z["beam_stable"][rows], info_ok=z["info_stable"][rows])


def trace_records(z, worlds):
    """Every step t of a free-running trace as a what-if step from state[t - 1] with ep_t[t - 1], in the world of its episode (`worlds`: one dict per
    episode, in order).  A step that follows a reset has no state in the fixture to start from and is left out.  Returns (records, kept steps, the
    number left out, the number of episode starts)."""
    done = z["done"].astype(bool)
    T = len(done)
    start = np.concatenate([[True], done[:-1]])      # step t opens an episode
    episode = np.cumsum(start) - 1
    keep = np.nonzero(~start)[0]
    nw = len(worlds)
    assert episode.max() < nw
    cores = np.zeros((nw, 8, 4)); obst = np.zeros((nw, 10, 3)); nc = np.zeros(nw, int); no = np.zeros(nw, int); goal = np.zeros((nw, 2))
    for i, w in enumerate(worlds):
        nc[i], no[i] = len(w["cores"]), len(w["obstacles"])
        cores[i, :nc[i]] = w["cores"]; obst[i, :no[i]] = w["obstacles"]; goal[i] = w["goal"]
    ep = episode[keep]
    rec = records(cores[ep], nc[ep], obst[ep], no[ep], goal[ep], z["state"][keep - 1], z["actions"][keep], z["ep_t"][keep - 1])
    return rec, keep, T - len(keep), int(start.sum())


def g2_worlds(z):
    return [dict(cores=z["world_cores"][i][:z["world_n"][i][0]], obstacles=z["world_obs"][i][:z["world_n"][i][1]], goal=z["world_goal"][i])
            for i in range(len(z["world_n"]))]


def g8_worlds(z):
    """g8 holds no world tables: they are regenerated from its seed (the oracle's reset is pinned to the reference bit for bit by g1 / g16)."""
    from oracle.oracle import OracleEnv
    env = OracleEnv(int(z["seed"]))
    env.set_flags(reset_start_and_goal=False, random_reset_state=True, set_boundary=True)
    env.set_start_goal(z["start"], z["goal"])
    env.set_world_size(8, 8, 25.0)
    worlds = []
    for _ in range(1 + int(z["done"].sum())):
        env.reset()
        w = env.get_world()
        worlds.append(dict(cores=w["cores"].copy(), obstacles=w["obstacles"].copy(), goal=w["goal"].copy()))
    return worlds


G8_SPEC = dict(set_boundary=1, N=5)


@pytest.mark.parametrize("fn", G2_FILES)
def test_g2_traces_step_by_step_on_the_host(host_program, tmp_path, fn):
    z = np.load(os.path.join(G, fn))
    rec, keep, skipped, starts = trace_records(z, g2_worlds(z))
    print(f"[{fn}] {len(keep)} steps, {skipped} skipped (they follow a reset), {starts} episode starts")
    assert skipped == starts
    check_steps(f"{fn} host", run_host(host_program, tmp_path, {}, rec, "g2"), z["state"][keep], z["obs"][keep], z["reward"][keep], z["done"][keep],
                z["info"][keep])


def test_g8_trace_step_by_step_on_the_host(host_program, tmp_path):
    z = np.load(os.path.join(G, "g8_boundary_trace.npz"))
    rec, keep, skipped, starts = trace_records(z, g8_worlds(z))
    print(f"[g8] {len(keep)} steps, {skipped} skipped (they follow a reset), {starts} episode starts")
    assert skipped == starts and (z["info"][keep] == 1).sum() >= 5
    check_steps("g8 host", run_host(host_program, tmp_path, G8_SPEC, rec, "g8"), z["state"][keep], z["obs"][keep], z["reward"][keep], z["done"][keep],
                z["info"][keep])


def test_bad_state_and_bad_action_on_the_host(host_program, tmp_path):
    z = np.load(os.path.join(G, "g3_single_step.npz"))
    k = np.arange(6)
    state = np.zeros((6, 6)); state[:, :4] = z["state_in"][k]
    action = z["action"][k].copy()
    state[1, 0] = np.nan; state[2, 2] = 1e6; state[3, 3] = np.inf; action[4] = 9; state[5, 2] = -999999.5
    rec = records(z["cores"][k], z["n"][k][:, 0], z["obs_tab"][k], z["n"][k][:, 1], z["goal"][k], state, action, z["ep_t"][k])
    st, obs, rew, done, info = run_host(host_program, tmp_path, {}, rec, "bad")
    for i in (1, 2, 3, 4):
        assert np.isnan(st[i]).all() and np.isnan(obs[i]).all() and np.isnan(rew[i]) and done[i] and info[i] == 64, i
    for i in (0, 5):      # a heading just inside the bound is wrapped by the loop, like the reference's
        assert np.isfinite(st[i]).all() and np.isfinite(obs[i]).all() and 0.0 <= st[i, 2] < 2 * np.pi and info[i] in (0, 1, 2, 3, 4), i
    assert np.abs(st[0] - z["state_out"][0]).max() <= 1e-9


# ---- lookahead_map with stand-ins -------------------------------------------------------------------------------------------------------
def test_lookahead_map_order_chunks_and_backup():
    from distributional_rl_navigation_amd import maps
    xs, ys, thetas = np.arange(5) * 1.5, np.arange(3) + 10.0, np.array([0.25, 2.0])
    seen, stepped, chunks = [], [], []

    def observe(st):
        assert st.dtype == torch.float64 and st.shape[1] == 4
        seen.append(st.clone())
        obs = torch.zeros(st.shape[0], 26, dtype=torch.float32)
        obs[:, :4] = st.to(torch.float32)
        return obs, (st[:, 0] > 4.0).to(torch.uint8)

    def step(st, a):
        assert st.dtype == torch.float64 and st.shape[1] == 4 and a.dtype == torch.int32 and a.shape == (st.shape[0],) and (a == a[0]).all()
        stepped.append((st.shape[0], int(a[0])))
        obs = torch.zeros(st.shape[0], 26, dtype=torch.float32)
        obs[:, 0] = (st[:, 0] + a).to(torch.float32); obs[:, 1] = st[:, 1].to(torch.float32)      # x' = x + a
        done = ((a == 8) | (st[:, 0] == 0.0)).to(torch.uint8)
        return dict(obs=obs, reward=st[:, 1] * 0.5 - a.to(torch.float64), done=done, info=done * 3, state=None)

    def policy(obs):      # Q(s, b) = x + y / 8 - b / 4: max over b is at b = 0
        chunks.append(obs.shape[0])
        b = torch.arange(9, dtype=torch.float32)
        return dict(action=torch.full((obs.shape[0],), 2, dtype=torch.int32), q=obs[:, 0:1] + obs[:, 1:2] / 8 - b[None, :] / 4)

    res = maps.lookahead_map(policy, None, 0, xs, ys, thetas, 0.75, gamma=0.5, chunk=7, observe=observe, step=step)
    # 30 poses in chunks of 7; per chunk one policy call on the poses and nine on the next observations, the actions in order
    assert chunks == [7] * 40 + [2] * 10
    assert stepped == [(m, a) for m in (7, 7, 7, 7, 2) for a in range(9)]
    want = np.array([[x, y, t, 0.75] for t in thetas for y in ys for x in xs])
    assert np.array_equal(torch.cat(seen).numpy(), want)      # theta slowest, then y, then x
    for k, tail, dt in (("q", (9,), np.float32), ("backup", (9,), np.float64), ("residual", (9,), np.float64), ("reward_next", (9,), np.float64),
                        ("done_next", (9,), np.uint8), ("info_next", (9,), np.uint8), ("action", (), np.int32), ("lookahead_action", (), np.int32),
                        ("flags", (), np.uint8)):
        assert res[k].shape == (2, 3, 5) + tail and res[k].dtype == dt, (k, res[k].shape, res[k].dtype)
    for it, t in enumerate(thetas):
        for iy, y in enumerate(ys):
            for ix, x in enumerate(xs):
                q = np.float32(x) + np.float32(y) / 8 - np.arange(9, dtype=np.float32) / 4
                assert np.array_equal(res["q"][it, iy, ix], q) and res["action"][it, iy, ix] == 2 and res["flags"][it, iy, ix] == (x > 4.0)
                for a in range(9):
                    r, d = y * 0.5 - a, (a == 8) or x == 0.0
                    best_next = float(np.float32(x + a) + np.float32(y) / 8)      # max_b Q(s', b), s' = (x + a, y)
                    backup = r + 0.5 * (0.0 if d else 1.0) * best_next
                    assert res["reward_next"][it, iy, ix, a] == r and res["done_next"][it, iy, ix, a] == d and res["info_next"][it, iy, ix, a] == 3 * d
                    assert res["backup"][it, iy, ix, a] == backup, (x, y, a)
                    assert res["residual"][it, iy, ix, a] == backup - float(q[a])
                assert res["lookahead_action"][it, iy, ix] == int(np.argmax(res["backup"][it, iy, ix]))


def test_lookahead_map_refuses_a_policy_without_q():
    from distributional_rl_navigation_amd import maps
    observe = lambda st: (torch.zeros(st.shape[0], 26), torch.zeros(st.shape[0], dtype=torch.uint8))
    step = lambda st, a: dict(obs=torch.zeros(st.shape[0], 26), reward=torch.zeros(st.shape[0], dtype=torch.float64),
                              done=torch.zeros(st.shape[0], dtype=torch.uint8), info=torch.zeros(st.shape[0], dtype=torch.uint8))
    with pytest.raises(ValueError):
        maps.lookahead_map(lambda obs: dict(action=torch.zeros(obs.shape[0], dtype=torch.int32)), None, 0, [0.0, 1.0], [0.0], [0.0], 1.0, gamma=0.9,
                           observe=observe, step=step)
