"""IQN evaluation episodes in one launch (mn_rollout_iqn): what can be checked without a GPU -- the C-ABI declaration and binding, the kernel's
resource budget from hipcc's remarks, and the evaluation bookkeeping built from the launch's traces against the per-step loop's formulas."""
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "distributional_rl_navigation_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"


def test_header_declares_and_capi_binds():
    with open(os.path.join(ROOT, "include", "marinenav_hip.h")) as f:
        assert re.search(r"int mn_rollout_iqn\(mn_handle \*h, mn_iqn_ctx \*ctx", f.read())
    from distributional_rl_navigation_amd import _capi
    sig = {s[0]: s for s in _capi.SIGNATURES}
    assert "mn_rollout_iqn" in sig and len(sig["mn_rollout_iqn"][2]) == 17


def test_kernel_has_no_scratch_and_fits_the_cu_lds():
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-I../../include", "-I.", "--cuda-device-only",
           "-Rpass-analysis=kernel-resource-usage", "-c", "-o", "/dev/null", "-ffp-contract=fast-honor-pragmas", "-fno-slp-vectorize", "mn_rollout_iqn.hip"]
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
    ks = {k: v for k, v in out.items() if "mn_rollout_iqn_kernel" in k}
    assert len(ks) == 2, list(out)          # <double, parity, 8 lanes> and <float, compact, 8 lanes>
    dynamic = (37840 + 208 + 32) * 4        # the acting weight image + one feature buffer + the observation row (mn_rollout_iqn.hip)
    for k, v in ks.items():
        assert v["ScratchSize"] == 0, (k, v)
        assert v["LDS Size"] + dynamic <= 163840, (k, v)


def _loop_reference(reward, done, info, action, discount, energy_tab, dt, N):
    """IQNAgent.evaluation_vec's loop body, as written there, on CPU tensors fed from the traces."""
    import torch
    T, n = reward.shape
    etab = torch.from_numpy(energy_tab)
    alive = torch.ones(n, dtype=torch.bool)
    ret = torch.zeros(n, dtype=torch.float64)
    length = torch.zeros(n, dtype=torch.int64)
    energy = torch.zeros(n, dtype=torch.float64)
    last_info = torch.zeros(n, dtype=torch.uint8)
    acts = torch.full((T, n), -1, dtype=torch.int32)
    for t in range(T):
        a = torch.from_numpy(action[t]).clamp(0, 8)      # (the loop's dead rows carry some action; masked either way)
        r = torch.from_numpy(reward[t]); d = torch.from_numpy(done[t]); i = torch.from_numpy(info[t])
        ret += torch.where(alive, (discount ** t) * r.double(), torch.zeros_like(ret))
        length += alive.long()
        energy += torch.where(alive, etab[a.long()].double(), torch.zeros_like(energy))
        acts[t] = torch.where(alive, a, torch.full_like(a, -1))
        last_info = torch.where(alive, i, last_info)
        alive = alive & ~d.bool()
        if not bool(alive.any()):
            break
    acts_h = acts.numpy(); length_h = length.numpy()
    return ([[int(x) for x in acts_h[:length_h[k], k]] for k in range(n)], [float(x) for x in ret.numpy()],
            [bool(x) for x in (last_info == 4).numpy()], [float(dt * N * l) for l in length_h], [float(x) for x in energy.numpy()])


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_trace_bookkeeping_equals_loop(seed):
    from distributional_rl_navigation_amd.iqn.agent import evaluation_from_traces
    rng = np.random.RandomState(seed)
    T, n = 200, 30
    ends = rng.randint(1, T + 40, size=n)              # some envs run past the traces
    ends[0] = min(T, ends.max())
    t_idx = np.arange(T)[:, None]
    alive_before = t_idx < ends[None, :]
    done = (t_idx >= ends[None, :] - 1).astype(np.uint8)
    info = np.where(t_idx == ends[None, :] - 1, rng.randint(2, 5, size=(T, n)), 0).astype(np.uint8)
    info = np.where(t_idx > ends[None, :] - 1, info[np.minimum(ends - 1, T - 1), np.arange(n)][None, :], info).astype(np.uint8)
    reward = np.where(alive_before, rng.standard_normal((T, n)).astype(np.float32), 0).astype(np.float32)
    action = np.where(alive_before, rng.randint(0, 9, size=(T, n)), -1).astype(np.int32)
    steps = int(min(T, ends.max()))
    a_tab = np.array([-0.4, 0.0, 0.4], dtype=np.float32); w_tab = np.array([-0.5235988, 0.0, 0.5235988], dtype=np.float32)
    e_a = np.abs(a_tab / a_tab.max()); e_w = np.abs(w_tab / w_tab.max())
    energy_tab = (e_a.reshape(3, 1) + e_w.reshape(1, 3)).reshape(-1).astype(np.float32)
    got = evaluation_from_traces(reward[:steps], done[:steps], info[:steps], action[:steps], 0.99, energy_tab, 0.05, 10)
    want = _loop_reference(reward, done, info, action, 0.99, energy_tab, 0.05, 10)
    assert got == want
