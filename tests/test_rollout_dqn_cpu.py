"""DQN evaluation episodes in one launch (mn_rollout_dqn) and per-row cvar / adaptive flags for the IQN episode launch (mn_rollout_iqn_rows): what
can be checked without a GPU -- the C-ABI declarations, bindings and exports, the DQN episode kernel's resource budget from hipcc's remarks, the
evaluation bookkeeping built from the launch's traces against train_dqn.evaluate's loop formulas, and the driver's flag."""
import ctypes
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "distributional_rl_navigation_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
IMAGE_BYTES = 126912      # mn_dqn_image_floats() * 4: the weight image in dynamic LDS


def test_header_declares_capi_binds_library_exports():
    with open(os.path.join(ROOT, "include", "marinenav_hip.h")) as f:
        src = f.read()
    assert re.search(r"int mn_rollout_dqn\(mn_handle \*h, const float \*const \*weights, float \*image_dev, int32_t repack, int32_t n_steps", src)
    assert re.search(r"int mn_rollout_iqn_rows\(mn_handle \*h, mn_iqn_ctx \*ctx", src)
    assert re.search(r"int32_t adaptive, const float \*cvar_row_dev, const uint8_t \*adaptive_row_dev, float \*obs_dev", src)
    from distributional_rl_navigation_amd import _capi
    sig = {s[0]: s for s in _capi.SIGNATURES}
    assert len(sig["mn_rollout_dqn"][2]) == 13
    assert len(sig["mn_rollout_iqn_rows"][2]) == 19
    assert len(sig["mn_rollout_iqn"][2]) == 17      # unchanged
    if not os.path.exists(_capi.LIB_PATH):
        _capi.build()
    lib = ctypes.CDLL(_capi.LIB_PATH)
    assert hasattr(lib, "mn_rollout_dqn") and hasattr(lib, "mn_rollout_iqn_rows")
    assert lib.mn_dqn_image_floats() * 4 == IMAGE_BYTES


def _makefile_flags(target):
    """The hipcc flags of `target`'s recipe in csrc/Makefile, variables expanded."""
    with open(os.path.join(CSRC, "Makefile")) as f:
        mk = f.read()
    m = re.search(rf"^{re.escape(target)}:.*\n\t\$\(HIPCC\) (.*) -c \$< -o \$@", mk, flags=re.M)
    assert m, target
    var = dict(re.findall(r"^(\w+) \??= (.*)$", mk, flags=re.M))
    flags = m.group(1)
    for _ in range(3):
        flags = re.sub(r"\$\((\w+)\)", lambda v: var[v.group(1)], flags)
    return flags.split()


def test_kernel_has_no_scratch_and_fits_the_cu_lds():
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    flags = _makefile_flags("mn_rollout_dqn.o")
    assert "-ffp-contract=off" in flags and "-fno-slp-vectorize" in flags      # the step body's flags (mn_rollout.o)
    cmd = [HIPCC] + flags + ["--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c", "-o", "/dev/null", "mn_rollout_dqn.hip"]
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
    ks = {k: v for k, v in out.items() if "mn_rollout_dqn_kernel" in k}
    assert len(ks) == 2, list(out)          # <double, parity, 8 lanes> and <float, compact, 8 lanes>
    for k, v in ks.items():
        assert v["ScratchSize"] == 0, (k, v)
        assert v["LDS Size"] + IMAGE_BYTES <= 163840, (k, v)


def _loop_reference(reward, done, info, action, discount, energy_tab, dt, N):
    """train_dqn.evaluate's loop body and result dict, as written there, on CPU tensors fed from the traces."""
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
    acts_h, length_h = acts.numpy(), length.numpy()
    return dict(rewards=ret.numpy(), successes=(last_info == 4).numpy(),
                times=np.array([dt * N * l for l in length_h], dtype=np.float64), energies=energy.numpy(),
                actions=[[int(x) for x in acts_h[:length_h[i], i]] for i in range(n)])


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_trace_bookkeeping_equals_loop(seed):
    from distributional_rl_navigation_amd.train_dqn import evaluation_from_rollout
    rng = np.random.RandomState(seed)
    T, n = 200, 30
    # seeds 0-1: some episodes run past the T steps of the launch; seeds 2-3: every episode ends early, the traces go on (reward 0, done 1, action -1)
    ends = rng.randint(1, T + 40, size=n) if seed < 2 else rng.randint(1, T - 50, size=n)
    t_idx = np.arange(T)[:, None]
    alive_before = t_idx < ends[None, :]
    done = (t_idx >= ends[None, :] - 1).astype(np.uint8)
    info = np.where(t_idx == ends[None, :] - 1, rng.randint(2, 5, size=(T, n)), 0).astype(np.uint8)
    info = np.where(t_idx > ends[None, :] - 1, info[np.minimum(ends - 1, T - 1), np.arange(n)][None, :], info).astype(np.uint8)
    reward = np.where(alive_before, rng.standard_normal((T, n)).astype(np.float32), 0).astype(np.float32)
    action = np.where(alive_before, rng.randint(0, 9, size=(T, n)), -1).astype(np.int32)
    a_tab = np.array([-0.4, 0.0, 0.4], dtype=np.float32); w_tab = np.array([-0.5235988, 0.0, 0.5235988], dtype=np.float32)
    e_a = np.abs(a_tab / a_tab.max()); e_w = np.abs(w_tab / w_tab.max())
    energy_tab = (e_a.reshape(3, 1) + e_w.reshape(1, 3)).reshape(-1).astype(np.float32)
    got = evaluation_from_rollout(dict(reward=reward, done=done, info=info, action=action), 0.99, energy_tab, 0.05, 10)
    want = _loop_reference(reward, done, info, action, 0.99, energy_tab, 0.05, 10)
    assert sorted(got) == sorted(want)
    for k in ("rewards", "successes", "times", "energies"):
        assert got[k].dtype == want[k].dtype and got[k].tolist() == want[k].tolist(), k
    assert got["actions"] == want["actions"]
    assert (max(len(a) for a in got["actions"]) == T) == (seed < 2)


def test_train_dqn_dry_run_reports_eval_one_launch(tmp_path):
    cfg = tmp_path / "config_DQN.json"
    cfg.write_text(json.dumps({"agent": "DQN", "seed": [0, 1], "total_timesteps": 3_000_000, "eval_freq": 10_000, "save_dir": str(tmp_path)}))
    out = {}
    for extra in ((), ("--eval-one-launch",)):
        r = subprocess.run([sys.executable, "-m", "distributional_rl_navigation_amd.train_dqn", "-C", str(cfg), "--dry-run", *extra],
                           cwd=ROOT, capture_output=True, text=True, timeout=300, env=dict(os.environ, CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES=""))
        assert r.returncode == 0, r.stderr[-2000:]
        out[extra] = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
    assert [t["eval_one_launch"] for t in out[()]] == [False, False]
    assert [t["eval_one_launch"] for t in out[("--eval-one-launch",)]] == [True, True]
    assert [t["plan"] for t in out[()]] == [t["plan"] for t in out[("--eval-one-launch",)]]      # the flag changes no plan
