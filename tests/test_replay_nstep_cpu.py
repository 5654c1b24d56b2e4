"""The n-step window of the replay ring without a GPU (iqn/replay_buffer.py, the torch path -- the yardstick of the HIP kernel): nstep_mode "episode"
EQUALS a plain per-stream restatement of the rule (replay_nstep_cases.PlainNstep: a deque per stream, np.float32 arithmetic in the rule's order) after
every add; "reference" still is the reference's window (golden G15, and the same restatement); states round-trip inside a filling window; states written
before there were modes load as "reference"; a mode mismatch is refused by name."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import replay_nstep_cases as H      # noqa: E402

from distributional_rl_navigation_amd.iqn.replay_buffer import ReplayBuffer      # noqa: E402

K, ADDS = 3, 40


def _add(buf, stream, t):
    obs, act, rew, nxt, dn = stream
    buf.add_batch(torch.from_numpy(obs[t]), torch.from_numpy(act[t]).long(), torch.from_numpy(rew[t]), torch.from_numpy(nxt[t]),
                  torch.from_numpy(dn[t]).float())


def _run_against_plain(mode, n_step, pattern, capacity, k=K, adds=ADDS, seed=0):
    stream = H.make_stream(adds, k, n_step, pattern, seed)
    buf = ReplayBuffer(capacity, 8, "cpu", seed=5, gamma=H.GAMMA, n_step=n_step, nstep_mode=mode)
    plain = H.PlainNstep(capacity, k, n_step, mode)
    for t in range(adds):
        _add(buf, stream, t)
        plain.add(H.rows_of(stream, t))
        H.same_as_plain(buf, plain)
    assert buf.size == min(capacity, k * (adds - n_step + 1))
    return buf


@pytest.mark.parametrize("n_step", [2, 3, 4])
@pytest.mark.parametrize("pattern", H.DONE_PATTERNS)
@pytest.mark.parametrize("mode", ["episode", "reference"])
def test_torch_window_equals_the_plain_restatement(mode, n_step, pattern):
    """k = 3 streams, 40 adds: ring contents, ptr and size after every add.  Capacity 50: the ring wraps, and (3 does not divide 50) it wraps inside an add."""
    _run_against_plain(mode, n_step, pattern, capacity=50, seed=n_step)


@pytest.mark.parametrize("mode", ["episode", "reference"])
def test_a_call_larger_than_the_ring_keeps_its_newest_rows(mode):
    _run_against_plain(mode, 3, "random", capacity=5, k=8, adds=12, seed=9)


def test_episode_mode_by_hand():
    """One stream, n_step = 3, gamma = 0.5, rewards 1, 2, 4, 8, 16 with the episode ending at the third step: the three windows that contain the end are cut
    there (returns 1 + 1 + 1, 2 + 2, 4; next state of the third step; done), the window behind it starts clean."""
    buf = ReplayBuffer(8, 2, "cpu", seed=0, gamma=0.5, n_step=3, nstep_mode="episode")
    ref = ReplayBuffer(8, 2, "cpu", seed=0, gamma=0.5, n_step=3)
    assert ref.nstep_mode == "reference"
    for t, (r, d) in enumerate(zip((1.0, 2.0, 4.0, 8.0, 16.0, 32.0), (0, 0, 1, 0, 0, 0))):
        for b in (buf, ref):
            b.add(np.full(26, t, np.float32), t, r, np.full(26, t + 0.5, np.float32), bool(d))
    assert buf.size == ref.size == 4
    assert buf.rewards[:4, 0].tolist() == [1 + 1 + 1, 2 + 2, 4, 8 + 8 + 8] and ref.rewards[:4, 0].tolist() == [3, 6, 12, 24]
    assert buf.dones[:4, 0].tolist() == [1, 1, 1, 0] and ref.dones[:4, 0].tolist() == [1, 0, 0, 0]
    assert buf.next_states[:4, 0].tolist() == [2.5, 2.5, 2.5, 5.5] and ref.next_states[:4, 0].tolist() == [2.5, 3.5, 4.5, 5.5]
    assert buf.states[:4, 0].tolist() == ref.states[:4, 0].tolist() == [0, 1, 2, 3] and buf.actions[:4, 0].tolist() == [0, 1, 2, 3]


def test_reference_mode_still_meets_the_golden_window():
    """Golden G15 (the reference's own n-step ReplayBuffer) under test_replay_golden.py's bounds: contents equal, returns within 1e-6 -- with the mode named."""
    Z = np.load(os.path.join(os.path.dirname(__file__), "golden", "g15_replay_nstep.npz"))
    cap, n_step, gamma = int(Z["capacity"]), int(Z["n_step"]), float(Z["gamma"])
    buf = ReplayBuffer(cap, 8, "cpu", seed=5, gamma=gamma, n_step=n_step, nstep_mode="reference")
    for i in range(len(Z["in_actions"])):
        buf.add(Z["in_states"][i], int(Z["in_actions"][i]), float(Z["in_rewards"][i]), Z["in_next"][i], bool(Z["in_dones"][i]))
        assert len(buf) == Z["sizes"][i]
    order = (torch.arange(buf.size) + (buf.ptr if buf.size == buf.capacity else 0)) % buf.capacity
    s, a, r, ns, d = (t[order].numpy() for t in (buf.states, buf.actions, buf.rewards, buf.next_states, buf.dones))
    assert np.array_equal(s, Z["mem_states"].astype(np.float32)) and np.array_equal(ns, Z["mem_next"].astype(np.float32))
    assert np.array_equal(a[:, 0], Z["mem_actions"]) and np.array_equal(d[:, 0], Z["mem_dones"].astype(np.float32))
    np.testing.assert_allclose(r[:, 0], Z["mem_rewards"], rtol=0, atol=1e-6)
    assert "ns" not in buf._hist and "d" not in buf._hist      # the two further window arrays are episode mode's


@pytest.mark.parametrize("mode", ["episode", "reference"])
def test_state_round_trip_inside_a_filling_window(mode):
    stream = H.make_stream(8, 4, 3, "random", seed=2)
    a = ReplayBuffer(64, 8, "cpu", seed=5, gamma=H.GAMMA, n_step=3, nstep_mode=mode)
    _add(a, stream, 0); _add(a, stream, 1)
    assert a.size == 0 and a._hist["count"] == 2
    sd = a.state_dict()
    assert sd["nstep_mode"] == mode and sorted(sd["hist"]) == (["a", "count", "d", "ns", "r", "s"] if mode == "episode" else ["a", "count", "r", "s"])
    b = ReplayBuffer(64, 8, "cpu", seed=77, gamma=H.GAMMA, n_step=3, nstep_mode=mode)
    b.load_state_dict(sd)
    for t in range(2, 8):
        _add(a, stream, t); _add(b, stream, t)
        H.same_rings(a, b)
    assert a.size == 24
    assert torch.equal(a.sample_indices(8), b.sample_indices(8))


def test_a_state_without_a_mode_loads_as_reference():
    stream = H.make_stream(6, 4, 3, "random", seed=3)
    a = ReplayBuffer(64, 8, "cpu", seed=5, gamma=H.GAMMA, n_step=3)
    _add(a, stream, 0); _add(a, stream, 1)
    sd = a.state_dict()
    del sd["nstep_mode"]      # the format before there were modes: hist = {s, a, r, count}
    assert sorted(sd["hist"]) == ["a", "count", "r", "s"]
    b = ReplayBuffer(64, 8, "cpu", seed=1, gamma=H.GAMMA, n_step=3)
    b.load_state_dict(sd)
    for t in range(2, 6):
        _add(a, stream, t); _add(b, stream, t)
        H.same_rings(a, b)
    with pytest.raises(ValueError, match="nstep_mode"):
        ReplayBuffer(64, 8, "cpu", seed=1, gamma=H.GAMMA, n_step=3, nstep_mode="episode").load_state_dict(sd)


def test_a_mode_mismatch_is_refused_by_name():
    e = ReplayBuffer(64, 8, "cpu", seed=5, gamma=H.GAMMA, n_step=3, nstep_mode="episode")
    r = ReplayBuffer(64, 8, "cpu", seed=5, gamma=H.GAMMA, n_step=3, nstep_mode="reference")
    with pytest.raises(ValueError, match="'episode'.*'reference'"):
        r.load_state_dict(e.state_dict())
    with pytest.raises(ValueError, match="'reference'.*'episode'"):
        e.load_state_dict(r.state_dict())
    with pytest.raises(ValueError, match="nstep_mode"):
        ReplayBuffer(64, 8, "cpu", seed=5, gamma=H.GAMMA, n_step=3, nstep_mode="sliding")


def test_window_kernels_compile_for_gfx950_without_scratch_and_without_a_fused_multiply_add():
    """Both instantiations: no scratch, no LDS, the registers DESIGN records (20 / 22 VGPRs) with some room; in the ISA of replay.hip every float32 multiply
    and add stands alone (the return's product rounds before the sum) -- no fused or packed form anywhere in the file.  The C-ABI is bound as declared."""
    import ctypes
    import re
    import subprocess
    from distributional_rl_navigation_amd import _capi
    sig = {s[0]: s for s in _capi.SIGNATURES}["mn_replay_append_nstep"]
    assert len(sig[2]) == 23 and sig[2][12] is _capi.MnNstepGamma and ctypes.sizeof(_capi.MnNstepGamma) == 4 * _capi.NSTEP_MAX == 64
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "marinenav_hip.h")).read()
    assert re.search(r"#define MN_NSTEP_MAX 16\b", header) and "#define MN_NSTEP_REFERENCE 0" in header and "#define MN_NSTEP_EPISODE 1" in header
    hipcc, csrc = "/opt/rocm/bin/hipcc", os.path.join(os.path.dirname(_capi.LIB_PATH), "csrc")
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-I../../include", "-I.", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage",
           "-S", "-o", "-", "replay.hip"]
    r = subprocess.run(cmd, cwd=csrc, capture_output=True, text=True, timeout=600)
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
    kernels = {k: v for k, v in usage.items() if "replay_append_nstep_kernel" in k}
    assert len(kernels) == 2, list(usage)      # <EPISODE = false>, <EPISODE = true>
    for k, v in kernels.items():
        assert v["ScratchSize"] == 0 and v["LDS Size"] == 0 and v["VGPRs"] <= 32, (k, v)
    isa = r.stdout
    assert len(re.findall(r"\bv_mul_f32", isa)) >= 2 and len(re.findall(r"\bv_add_f32", isa)) >= 2
    assert not re.search(r"\bv_(fma|fmac|mac|mad|pk_fma|pk_mul|pk_add)_f32", isa)


def test_the_mode_reaches_the_ring_from_the_agent_and_the_trainer():
    from distributional_rl_navigation_amd import train_iqn as T
    from distributional_rl_navigation_amd.iqn.agent import IQNAgent
    ag = IQNAgent(26, 9, n_step=3, n_step_mode="episode", BATCH_SIZE=8, BUFFER_SIZE=64, device="cpu", seed=1)
    assert ag.memory.nstep_mode == "episode" and ag.memory.n_step == 3
    assert IQNAgent(26, 9, BATCH_SIZE=8, BUFFER_SIZE=64, device="cpu", seed=1).memory.nstep_mode == "reference"
    assert T.run_shaping_args()["n_step_mode"] == "reference" and T.run_shaping_args(n_step=3, n_step_mode="episode")["n_step_mode"] == "episode"
    # a checkpoint written before the key existed still resumes (only keys present on both sides are compared); another mode is refused by name
    old = {k: v for k, v in T.run_shaping_args(n_step=3).items() if k != "n_step_mode"}
    T.check_resumable(dict(plan={}, args=old), {}, T.run_shaping_args(n_step=3))
    with pytest.raises(ValueError, match="n_step_mode"):
        T.check_resumable(dict(plan={}, args=T.run_shaping_args(n_step=3)), {}, T.run_shaping_args(n_step=3, n_step_mode="episode"))
