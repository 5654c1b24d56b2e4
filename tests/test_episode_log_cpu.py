"""The training-episode log without a GPU: the gfx950 library exports `mn_episode_log`, its kernel needs neither scratch nor LDS (taken from
hipcc's resource remarks as tests/test_kernel_resources_cpu.py takes them), and the numpy twin `episode_log.replay_traces` gives hand-computed
records and summary rows."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from distributional_rl_navigation_amd.episode_log import N_INFO, replay_traces, rows_to_arrays, summarize

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "distributional_rl_navigation_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"


def test_library_exports_the_symbol_and_binds_it():
    from distributional_rl_navigation_amd import _capi
    if not os.path.exists(_capi.LIB_PATH):
        _capi.build()
    assert hasattr(ctypes.CDLL(_capi.LIB_PATH), "mn_episode_log")
    sig = {s[0]: s for s in _capi.SIGNATURES}["mn_episode_log"]
    assert len(sig[2]) == 19      # include/marinenav_hip.h: 19 parameters


def test_kernel_has_no_scratch_and_no_lds():
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-I../../include", "-I.", "--cuda-device-only",
                        "-Rpass-analysis=kernel-resource-usage", "-c", "-o", "/dev/null", "-ffp-contract=off", "mn_episode_log.hip"],
                       cwd=CSRC, capture_output=True, text=True, timeout=900)
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
    ks = {k: v for k, v in usage.items() if "mn_episode_log_kernel" in k}
    assert len(ks) == 1
    for k, v in ks.items():
        assert v["ScratchSize"] == 0 and v["LDS Size"] == 0 and v["VGPRs Spill"] == 0, (k, v)


D = 0.5      # (a discount whose powers are exact in binary: the hand-computed returns below are exact)
REWARD = np.array([[1.0, 2.0, -1.0],
                   [0.0, 4.0, -1.0],
                   [8.0, 8.0, -1.0],
                   [2.0, 16.0, -1.0]], dtype=np.float32)
DONE = np.array([[1, 0, 0],      # env 0 ends at step 0 ...
                 [0, 1, 0],      # ... env 1 at step 1 ...
                 [1, 0, 0],      # ... env 0 again at step 2 (two ends in one env) ...
                 [0, 1, 0]], dtype=np.uint8)      # ... env 1 again at step 3; env 2 never ends
INFO = np.array([[4, 0, 0], [0, 3, 0], [2, 0, 0], [0, 4, 0]], dtype=np.uint8)
EPS = np.array([1.0, 0.75, 0.5, 0.25], dtype=np.float32)


def test_replay_traces_on_hand_written_traces():
    rec, (ret, disc, length) = replay_traces(REWARD, DONE, INFO, D, EPS, first_step=10)
    # canonical order (step, env): env 0 @ 10, env 1 @ 11, env 0 @ 12, env 1 @ 13
    assert rec["step"].tolist() == [10, 11, 12, 13] and rec["env"].tolist() == [0, 1, 0, 1]
    assert rec["length"].tolist() == [1, 2, 2, 2]
    assert rec["info"].tolist() == [4, 3, 2, 4]
    assert rec["ret"].tolist() == [1.0, 2.0 + 0.5 * 4.0, 0.0 + 0.5 * 8.0, 8.0 + 0.5 * 16.0]
    assert rec["eps"].tolist() == [1.0, 0.75, 0.5, 0.25]
    assert [rec[k].dtype for k in ("step", "env", "length", "info", "ret", "eps")] == [np.int64, np.int32, np.int32, np.uint8, np.float64, np.float32]
    # env 2 never ended: no record, its running state goes on; env 0 is one step into its third episode, env 1 was just reset
    assert 2 not in rec["env"]
    assert ret.tolist() == [2.0, 0.0, -1.0 - 0.5 - 0.25 - 0.125] and disc.tolist() == [0.5, 1.0, 0.0625] and length.tolist() == [1, 0, 4]
    # continuing from a state = one call over all steps
    a, st = replay_traces(REWARD[:2], DONE[:2], INFO[:2], D, EPS[:2], first_step=10)
    b, st2 = replay_traces(REWARD[2:], DONE[2:], INFO[2:], D, EPS[2:], first_step=12, state=st)
    for k in rec:
        assert np.array_equal(np.concatenate([a[k], b[k]]), rec[k])
    assert all(np.array_equal(x, y) for x, y in zip(st2, (ret, disc, length)))


def test_the_return_is_the_running_product_not_the_power():
    """disc *= discount rounds at every step; with discount 0.99 it leaves the power's value within a few steps.  The record is the former."""
    T = 60
    reward = np.ones((T, 1), np.float32)
    done = np.zeros((T, 1), np.uint8); done[-1] = 1
    rec, _ = replay_traces(reward, done, np.full((T, 1), 2, np.uint8), 0.99, np.zeros(T))
    ret, disc = 0.0, 1.0
    for _ in range(T):
        ret += disc * 1.0
        disc *= 0.99
    assert rec["ret"][0] == ret and rec["length"][0] == T


def test_summary_rows_by_hand():
    rec, _ = replay_traces(REWARD, DONE, INFO, D, EPS)
    row = summarize(rec, 1234)
    assert row["timestep"] == 1234 and row["episodes"] == 4
    assert row["info_counts"].tolist() == [0, 0, 1, 1, 2] and len(row["info_counts"]) == N_INFO
    assert row["return_mean"] == (1.0 + 4.0 + 4.0 + 16.0) / 4 and row["length_mean"] == 7 / 4 and row["eps_mean"] == 2.5 / 4
    assert row["return_std"] == float(np.sqrt(((1 - 6.25) ** 2 + 2 * (4 - 6.25) ** 2 + (16 - 6.25) ** 2) / 4))
    empty = summarize(replay_traces(REWARD[:1, 2:], DONE[:1, 2:], INFO[:1, 2:], D, EPS[:1])[0], 7)
    assert empty["episodes"] == 0 and np.isnan(empty["return_mean"]) and empty["info_counts"].tolist() == [0] * N_INFO
    arrays = rows_to_arrays([row, empty])
    assert arrays["timesteps"].tolist() == [1234, 7] and arrays["episodes"].tolist() == [4, 0] and arrays["info_counts"].shape == (2, N_INFO)
