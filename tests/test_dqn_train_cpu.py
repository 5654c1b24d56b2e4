"""CPU-side checks of the DQN baseline's fused gradient step (csrc/dqn_train.hip) and of its training driver (train_dqn): the kernel's
resource budget where it is compiled, the workspace size and flat parameter layout the C-ABI documents, and the driver's plan for the
reference's config_DQN.json values (`--dry-run`, no GPU)."""
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
# config_DQN.json of the reference, written out here (the reference tree is not part of the repository)
CONFIG_DQN = {"agent": "DQN", "seed": [0, 1, 2, 3, 4], "total_timesteps": 3_000_000, "eval_freq": 10_000, "save_dir": "dqn_runs"}


def test_dqn_train_kernel_has_no_scratch_and_at_most_256_registers():
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-I../../include", "-I.", "-ffp-contract=off", "--cuda-device-only",
           "-Rpass-analysis=kernel-resource-usage", "-c", "-o", os.devnull, "dqn_train.hip"]
    r = subprocess.run(cmd, cwd=CSRC, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    usage, cur = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            cur = usage.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+)", line)
        if m and cur is not None:
            cur[m.group(1).strip()] = int(m.group(2))
    ks = [k for k in usage if "dqn_train_step_kernel" in k]
    assert ks, list(usage)
    for k in ks:
        v = usage[k]
        assert v["ScratchSize"] == 0 and v["VGPRs"] + v.get("AGPRs", 0) <= 256, (k, v)


def test_workspace_size_and_flat_layout():
    from distributional_rl_navigation_amd import _capi
    from distributional_rl_navigation_amd.dqn import DQNPolicy
    from distributional_rl_navigation_amd.dqn.fused_train import MAX_BATCH, P_TOTAL, PARAM_NAMES
    if not os.path.exists(_capi.LIB_PATH):
        _capi.build()
    L = _capi.lib()
    for b in (1, 5, 16, 17, 32, 100, 255, 256):
        assert L.mn_dqn_train_workspace_floats(b) >= -(-b // 16) * P_TOTAL + -(-b // 16), b
    assert L.mn_dqn_train_workspace_floats(0) < 0 and L.mn_dqn_train_workspace_floats(MAX_BATCH + 1) < 0
    pol = DQNPolicy(device="cpu")
    named = list(pol.q_net.named_parameters())
    assert tuple(n for n, _ in named) == PARAM_NAMES and len(named) == 18
    assert sum(p.numel() for _, p in named) == P_TOTAL == 27650
    # the kernel's offsets (csrc/dqn_train.hip O_*) are the running sums of this order
    offs = np.cumsum([0] + [p.numel() for _, p in named])[:-1]
    src = open(os.path.join(CSRC, "dqn_train.hip")).read()
    for name, want in zip(("O_VW", "O_VB", "O_GW", "O_GB", "O_SW", "O_SB", "O_HW", "O_HB", "O_H2W", "O_H2B", "O_OW", "O_OB", "O_Q0W", "O_Q0B",
                           "O_Q2W", "O_Q2B", "O_Q4W", "O_Q4B"), offs):
        assert re.search(rf"\b{name} = {want}\b", src), (name, want)


def _dry_run(tmp_path, *extra):
    cfg = tmp_path / "config_DQN.json"
    cfg.write_text(json.dumps(CONFIG_DQN))
    r = subprocess.run([sys.executable, "-m", "distributional_rl_navigation_amd.train_dqn", "-C", str(cfg), "--dry-run", *extra],
                       cwd=ROOT, capture_output=True, text=True, timeout=300, env=dict(os.environ, CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES=""))
    assert r.returncode == 0, r.stderr[-2000:]
    return [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]


def test_train_dqn_dry_run_plan_for_config_dqn(tmp_path):
    trials = _dry_run(tmp_path, "--n-envs", "4096", "--batch", "256")
    assert [t["seed"] for t in trials] == [0, 1, 2, 3, 4] and all(t["fused"] for t in trials)
    for t in trials:
        p = t["plan"]
        ref_samples = 3_000_000 * 32
        assert abs(p["samples"] - ref_samples) <= 0.01 * ref_samples, p
        assert p["total_grad_steps"] * 256 == p["samples"]
        assert p["target_sync_grad_steps"] == 1250
        assert p["learning_starts_vector_steps"] == 3
        assert t["eps_start"] == 1.0 and abs(t["eps_end"] - 0.05) < 1e-9
        assert p["n_evals"] == 30 and p["eval_every_vector_steps"] * 30 <= p["vector_steps"]
    from distributional_rl_navigation_amd.train_dqn import exploration_rate, make_plan
    p = trials[0]["plan"]
    assert exploration_rate(p["vector_steps"] // 20, p) == pytest.approx(0.525)
    assert exploration_rate(p["vector_steps"] // 2, p) == 0.05
    assert make_plan(dict(CONFIG_DQN, seed=0), 1024, 32)["learning_starts_vector_steps"] == 10
    assert _dry_run(tmp_path, "--torch-train", "--n-evals", "2")[0]["plan"]["n_evals"] == 2
