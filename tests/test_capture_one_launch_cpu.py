"""Captured experiment episodes from the episode launches (mn_set_trajectory_trace, mn_rollout_iqn_eval, run_experiment(capture=True,
one_launch=True)): what can be checked without a GPU -- the C-ABI declarations, bindings and exports, the new kernel's resource budget from
hipcc's remarks, and the one `ep_data` builder on synthetic traces against per-episode slices written out here."""
import ctypes
import json
import os
import re
import subprocess
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "distributional_rl_navigation_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"


def test_header_declares_capi_binds_and_library_exports():
    with open(os.path.join(ROOT, "include", "marinenav_hip.h")) as f:
        src = f.read()
    assert re.search(r"int mn_rollout_iqn_eval\(mn_handle \*h, mn_iqn_ctx \*ctx", src)
    assert re.search(r"int mn_set_trajectory_trace\(mn_handle \*h, double \*traj_trace_dev, int32_t n_steps, int32_t n_substeps\)", src)
    from distributional_rl_navigation_amd import _capi
    sig = {s[0]: s for s in _capi.SIGNATURES}
    assert len(sig["mn_rollout_iqn_eval"][2]) == 21          # mn_rollout_iqn_rows' 19 + the quantile and tau traces
    assert len(sig["mn_set_trajectory_trace"][2]) == 4
    # the entry points this adds to stay as they were
    assert (len(sig["mn_rollout_iqn"][2]), len(sig["mn_rollout_iqn_rows"][2]), len(sig["mn_rollout_dqn"][2]), len(sig["mn_rollout_policy"][2])) == (17, 19, 13, 10)
    if not os.path.exists(_capi.LIB_PATH):
        _capi.build()
    lib = ctypes.CDLL(_capi.LIB_PATH)
    assert hasattr(lib, "mn_rollout_iqn_eval") and hasattr(lib, "mn_set_trajectory_trace")


def _image_floats():
    """sp::OFF_FB (iqn_act_split.h), the floats of the full split-f16 weight image incl. the output layer's MFMA operands, from the network's shapes:
    26 inputs -> 208 features (13 tiles of 16) x 64 cos -> 64 -> 64 -> 9."""
    F, H, T1, KB2 = 208, 64, 13, 7
    u4 = T1 * 2 * 2 * 64 + 4 * KB2 * 2 * 64 + 4 * 2 * 2 * 64          # f16 A operands of layers 1-3 in 16-byte units: [tile][kb][hi, lo][64 lanes]
    off = u4 * 4                                                        # ... in floats
    off += 4 * 64 * 4                                                   # W4 (f32 output layer)
    off += F + H + H + 16                                               # b1 b2 b3 b4
    off += F + 16                                                       # bounds B1, constants
    off += 6 * 176 * 4 + 64 + F                                         # sensor encoder, velocity / goal encoders, encoder biases
    acting = off                                                        # sp::ACT_IMG_FLOATS
    off += 2 * 2 * 64 * 4                                               # W4 as an MFMA A operand: [2 kb][hi, lo][64 lanes] x 8 halves
    return acting, off, F


def test_eval_kernel_has_no_scratch_and_fits_the_cu_lds():
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-I../../include", "-I.", "--cuda-device-only",
           "-Rpass-analysis=kernel-resource-usage", "-c", "-o", "/dev/null", "-ffp-contract=fast-honor-pragmas", "-fno-slp-vectorize", "mn_rollout_iqn_eval.hip"]
    r = subprocess.run(cmd, cwd=CSRC, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    out, cur = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            cur = out.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+)", line)
        if m and cur is not None:
            cur[m.group(1).strip()] = int(m.group(2))
    assert not [k for k in out if "mn_rollout_iqn_kernel" in k], list(out)      # the acting episode kernel's two instantiations live in mn_rollout_iqn.hip only
    ks = {k: v for k, v in out.items() if "mn_episode_iqn_eval_kernel" in k}
    assert len(ks) == 2, list(out)          # <double, parity, 8 lanes> and <float, compact, 8 lanes>
    acting, full, F = _image_floats()
    assert acting == 37840                  # the acting image the existing episode kernel's test counts
    dynamic = (full + F + 32) * 4           # the full weight image + one feature buffer + the observation row
    for k, v in ks.items():
        assert v["ScratchSize"] == 0, (k, v)
        assert v["LDS Size"] + dynamic <= 163840, (k, v)


def _synthetic(seed, T=40, n=12, N=5):
    rng = np.random.RandomState(seed)
    length = rng.randint(1, T + 1, size=n)
    length[0] = T; length[1] = T; length[2] = 1              # some envs run to T, one ends at once
    alive = np.arange(T)[:, None] < length[None, :]
    action = np.where(alive, rng.randint(0, 9, size=(T, n)), -1).astype(np.int32)
    nan32, nan64 = np.float32("nan"), np.float64("nan")
    traj = np.where(alive[:, :, None, None], rng.standard_normal((T, n, N, 2)), nan64)
    cvar = np.where(alive, rng.random_sample((T, n)).astype(np.float32), nan32).astype(np.float32)
    quantiles = np.where(alive[:, :, None, None], rng.standard_normal((T, n, 32, 9)).astype(np.float32), nan32).astype(np.float32)
    taus = np.where(alive[:, :, None], rng.random_sample((T, n, 32)).astype(np.float32), nan32).astype(np.float32)
    return length, dict(action=action, traj=traj, cvar=cvar, quantiles=quantiles, taus=taus)


def _params():
    return types.SimpleNamespace(width=50.0, height=50.0, core_r=0.5, v_rel_max=1.0, p=0.8, v_range=[5.0, 10.0], obs_r_range=[1.0, 3.0], clear_r=10.0,
                                 goal_dis=2.0, timestep_penalty=-1.0, collision_penalty=-50.0, goal_reward=100.0, discount=0.99, dt=0.05, N=5,
                                 robot_r=0.8, max_speed=2.0, a=[-0.4, 0.0, 0.4], w=[-0.5, 0.0, 0.5], sonar_range=10.0, sonar_angle=2.0, num_beams=11)


def _worlds(n, rng):
    return [dict(start=np.array([5.0, 5.0]), goal=np.array([45.0, 45.0]), cores=rng.random_sample((3, 4)), obstacles=rng.random_sample((2, 3)),
                 init_theta=0.7, init_speed=0.0) for _ in range(n)]


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_ep_data_builder_equals_per_episode_slices(seed):
    """action_history has the episode's L actions and trajectory its N x L sub-step positions; actions_cvars L entries, actions_quantiles [L][1][32][9],
    actions_taus [L][1][32][1]: each exactly the plain slice of the traces, whatever lies behind the episode's end (NaN here)."""
    from distributional_rl_navigation_amd.experiments import ep_data_from_traces
    N = 5
    length, tr = _synthetic(seed, N=N)
    n = len(length)
    worlds = _worlds(n, np.random.RandomState(100 + seed))
    eps = ep_data_from_traces(tr, length, worlds, _params(), seed=15)
    assert len(eps) == n
    for i, ep in enumerate(eps):
        L = int(length[i])
        rb = ep["robot"]
        want_actions = [int(tr["action"][t, i]) for t in range(L)]
        want_traj = [[float(tr["traj"][t, i, s, 0]), float(tr["traj"][t, i, s, 1])] for t in range(L) for s in range(N)]
        want_cv = [float(tr["cvar"][t, i]) for t in range(L)]
        want_q = [[[[float(tr["quantiles"][t, i, k, a]) for a in range(9)] for k in range(32)]] for t in range(L)]
        want_t = [[[[float(tr["taus"][t, i, k])] for k in range(32)]] for t in range(L)]
        assert rb["action_history"] == want_actions and len(rb["action_history"]) == L
        assert rb["trajectory"] == want_traj and len(rb["trajectory"]) == N * L
        assert rb["actions_cvars"] == want_cv
        assert rb["actions_quantiles"] == want_q and np.array(rb["actions_quantiles"]).shape == (L, 1, 32, 9)
        assert rb["actions_taus"] == want_t and np.array(rb["actions_taus"]).shape == (L, 1, 32, 1)
        assert ep["env"]["seed"] == 15 and ep["env"]["start"] == [5.0, 5.0] and rb["N"] == N
        assert ep["env"]["cores"]["positions"] == [[float(r[0]), float(r[1])] for r in worlds[i]["cores"]]
    s = json.dumps(eps)
    assert "NaN" not in s                   # nothing behind an episode's end was looked at
    assert json.loads(s) == eps


def test_ep_data_of_planner_and_dqn_rows_has_no_iqn_keys():
    from distributional_rl_navigation_amd.experiments import ep_data_from_traces
    length, tr = _synthetic(7)
    tr = {k: tr[k] for k in ("action", "traj")}          # what the APF / BA / DQN producers trace
    eps = ep_data_from_traces(tr, length, _worlds(len(length), np.random.RandomState(3)), _params())
    for i, ep in enumerate(eps):
        assert not {"actions_cvars", "actions_quantiles", "actions_taus"} & set(ep["robot"])
        assert len(ep["robot"]["action_history"]) == length[i] and len(ep["robot"]["trajectory"]) == 5 * length[i]
    json.dumps(eps)


def test_trace_buffers_know_the_capture_traces():
    import torch
    from distributional_rl_navigation_amd.episodes import trace_buffers
    tr = trace_buffers(7, 3, "cpu", ("action", "cvar", "quantiles", "taus", "traj"), n_substeps=5)
    assert tr["quantiles"].shape == (7, 3, 32, 9) and tr["quantiles"].dtype == torch.float32 and bool(torch.isnan(tr["quantiles"]).all())
    assert tr["taus"].shape == (7, 3, 32) and tr["taus"].dtype == torch.float32 and bool(torch.isnan(tr["taus"]).all())
    assert tr["traj"].shape == (7, 3, 5, 2) and tr["traj"].dtype == torch.float64 and bool(torch.isnan(tr["traj"]).all())
