"""The query entry points and the map helpers, as far as they go without a GPU: the C-ABI declarations and their ctypes binding, the grids of
`maps.flow_field`, the order / chunking / shapes of `maps.policy_map` (with stand-ins for the device calls), and the resources of the query
kernels where they are compiled (hipcc cross-compiles gfx950 without a GPU): no scratch, no LDS."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "distributional_rl_navigation_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"


def _prototype(name):
    with open(os.path.join(ROOT, "include", "marinenav_hip.h")) as f:
        text = f.read()
    m = re.search(r"\bint " + name + r"\(([^;]*)\);", text)
    assert m, f"{name} is not declared in include/marinenav_hip.h"
    return [re.sub(r"\s+", " ", a).strip() for a in m.group(1).split(",")]


def test_query_symbols_declared_and_bound():
    from distributional_rl_navigation_amd import _capi
    assert _prototype("mn_query_velocity") == [
        "mn_handle *h", "const int32_t *env_of_query_dev", "int32_t env0", "const double *xy_dev", "int64_t n_queries", "double *v_dev", "void *stream"]
    assert _prototype("mn_query_observation") == [
        "mn_handle *h", "const int32_t *env_of_query_dev", "int32_t env0", "const double *state_dev", "int32_t velocity_mode", "int64_t n_queries",
        "float *obs_dev", "double *obs64_dev", "uint8_t *flags_dev", "void *stream"]
    sig = {n: (r, a) for n, r, a in _capi.SIGNATURES}
    p, i32, i64 = C.c_void_p, C.c_int32, C.c_int64
    assert sig["mn_query_velocity"] == (C.c_int, [p, p, i32, p, i64, p, p])
    assert sig["mn_query_observation"] == (C.c_int, [p, p, i32, p, i32, i64, p, p, p, p])
    with open(os.path.join(ROOT, "include", "marinenav_hip.h")) as f:
        text = f.read()
    for name, value in (("MN_QUERY_VELOCITY_GIVEN", _capi.QUERY_VELOCITY_GIVEN), ("MN_QUERY_VELOCITY_FROM_CURRENT", _capi.QUERY_VELOCITY_FROM_CURRENT),
                        ("MN_QUERY_FLAG_COLLISION", _capi.QUERY_FLAG_COLLISION), ("MN_QUERY_FLAG_OUTSIDE", _capi.QUERY_FLAG_OUTSIDE),
                        ("MN_QUERY_FLAG_GOAL", _capi.QUERY_FLAG_GOAL), ("MN_QUERY_FLAG_BAD_ENV", _capi.QUERY_FLAG_BAD_ENV)):
        m = re.search(name + r" = (\d+)", text)
        assert m and int(m.group(1)) == value, name
    assert (_capi.QUERY_FLAG_COLLISION, _capi.QUERY_FLAG_OUTSIDE, _capi.QUERY_FLAG_GOAL, _capi.QUERY_FLAG_BAD_ENV) == (1, 2, 4, 0x80)


class _Params:
    width, height = 50.0, 40.0


class _FieldEnv:
    """Stand-in for VecMarineNavEnv.velocity_at: v = (x + 100 env, y)."""
    params = _Params()

    def velocity_at(self, xy, env=0):
        xy = np.asarray(xy)
        assert xy.ndim == 2 and xy.shape[1] == 2
        return torch.from_numpy(np.stack([xy[:, 0] + 100.0 * env, xy[:, 1]], axis=1))


@pytest.mark.parametrize("n,margin", [(100, 0.0), (110, 2.5)])      # the two grids of env_visualizer.plot_graph
def test_flow_field_grids(n, margin):
    from distributional_rl_navigation_amd import maps
    xs, ys, v = maps.flow_field(_FieldEnv(), env_index=3, nx=n, ny=n, margin=margin)
    assert xs.shape == (n,) and ys.shape == (n,) and v.shape == (n, n, 2) and v.dtype == np.float64
    assert xs[0] == -margin and xs[-1] == 50.0 + margin and ys[0] == -margin and ys[-1] == 40.0 + margin
    assert np.array_equal(xs, np.linspace(-margin, 50.0 + margin, n)) and np.array_equal(ys, np.linspace(-margin, 40.0 + margin, n))
    # v[iy][ix] is the field at (xs[ix], ys[iy]), in the world asked for
    assert np.array_equal(v[:, :, 0], np.broadcast_to(xs[None, :] + 300.0, (n, n)))
    assert np.array_equal(v[:, :, 1], np.broadcast_to(ys[:, None], (n, n)))


def test_flow_field_rectangular():
    from distributional_rl_navigation_amd import maps
    xs, ys, v = maps.flow_field(_FieldEnv(), nx=7, ny=4)
    assert v.shape == (4, 7, 2) and np.array_equal(v[2, :, 0], xs) and np.array_equal(v[:, 5, 1], ys)


def test_policy_map_order_chunks_and_shapes():
    from distributional_rl_navigation_amd import maps
    xs, ys, thetas = np.arange(5) * 1.5, np.arange(3) + 10.0, np.array([0.25, 2.0])
    seen, chunks = [], []

    def observe(st):
        assert st.dtype == torch.float64 and st.shape[1] == 4
        seen.append(st.clone())
        obs = torch.zeros(st.shape[0], 26, dtype=torch.float32)
        obs[:, :4] = st.to(torch.float32)
        return obs, (st[:, 0] > 4.0).to(torch.uint8)

    def policy(obs):
        assert obs.dtype == torch.float32 and obs.shape[1] == 26
        chunks.append(obs.shape[0])
        m = obs.shape[0]
        return dict(action=(obs[:, 0] * 2).to(torch.int32), q=obs[:, 1:3].repeat(1, 2).reshape(m, 4), quantiles=obs[:, 2].reshape(m, 1, 1).expand(m, 3, 2))

    res = maps.policy_map(policy, None, 0, xs, ys, thetas, 0.75, chunk=7, observe=observe)
    assert chunks == [7, 7, 7, 7, 2]      # 30 poses in chunks of 7
    poses = torch.cat(seen).numpy()
    # theta is the slowest index, then y, then x
    want = np.array([[x, y, t, 0.75] for t in thetas for y in ys for x in xs])
    assert np.array_equal(poses, want)
    assert res["action"].shape == (2, 3, 5) and res["q"].shape == (2, 3, 5, 4) and res["quantiles"].shape == (2, 3, 5, 3, 2) and res["flags"].shape == (2, 3, 5)
    assert res["action"].dtype == np.int32 and res["flags"].dtype == np.uint8
    for it, t in enumerate(thetas):
        for iy, y in enumerate(ys):
            for ix, x in enumerate(xs):
                assert res["action"][it, iy, ix] == int(np.float32(x) * 2)
                assert np.array_equal(res["q"][it, iy, ix], np.float32([y, t, y, t]))
                assert (res["quantiles"][it, iy, ix] == np.float32(t)).all()
                assert res["flags"][it, iy, ix] == (x > 4.0)


def test_policy_map_refuses_a_short_policy_output():
    from distributional_rl_navigation_amd import maps
    observe = lambda st: (torch.zeros(st.shape[0], 26), torch.zeros(st.shape[0], dtype=torch.uint8))
    with pytest.raises(ValueError):
        maps.policy_map(lambda obs: dict(action=torch.zeros(1)), None, 0, [0.0, 1.0], [0.0], [0.0], 1.0, observe=observe)


def test_query_kernels_use_no_scratch_and_no_lds():
    """One lane per query and nothing shared between lanes: the kernels are built to hold no indexed array (mn_query_body.h), so a compiler or source
    change that sends one to scratch -- or to LDS, where hipcc puts a promoted private array -- fails here.  The message carries the figures DESIGN records."""
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-I../../include", "-I.", "--cuda-device-only", "-ffp-contract=off",
                        "-Rpass-analysis=kernel-resource-usage", "-c", "-o", "/dev/null", "mn_query.hip"], cwd=CSRC, capture_output=True, text=True, timeout=900)
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
    vel = {k: v for k, v in usage.items() if "mn_query_velocity_kernel" in k}
    obs = {k: v for k, v in usage.items() if "mn_query_observation_kernel" in k}
    assert len(vel) == 2 and len(obs) == 4, list(usage)      # <UNIFORM>, <UNIFORM, FROM_CURRENT>
    figures = "; ".join(f"{k}: VGPRs {v['VGPRs']}, SGPRs {v['TotalSGPRs']}, LDS {v['LDS Size']}, scratch {v['ScratchSize']}" for k, v in {**vel, **obs}.items())
    print(figures)
    for k, v in {**vel, **obs}.items():
        assert v["ScratchSize"] == 0 and v["LDS Size"] == 0 and v["VGPRs Spill"] == 0, figures
        assert v["VGPRs"] + v.get("AGPRs", 0) <= 256, figures
