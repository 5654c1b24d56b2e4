"""The float64 statement of the DQN gradient step (tests/dqn_train_f64.py) before it judges a kernel: pinned to the reference's own step (G11) and to torch's
Adam with history; every input of tests/test_dqn_train_f64_gpu.py satisfies, by the helper alone, the condition its GPU case relies on (the bisected clip-threshold
factors among them); and the bars reject deliberately wrong steps (computed by the helper itself, float64 numbers only) on named cases."""
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import dqn_train_f64 as H      # noqa: E402

from distributional_rl_navigation_amd.dqn import DQNAgent      # noqa: E402
from distributional_rl_navigation_amd.dqn.fused_train import PARAM_NAMES, P_TOTAL      # noqa: E402


def _cpu_agent(c):
    ag = DQNAgent(device="cpu", seed=H.NET_SEED, batch_size=c.B, buffer_size=4)
    ag.q_net.load_state_dict(c.local.state_dict())
    ag.q_net_target.load_state_dict(c.target.state_dict())
    return ag


def _eager(ag, exp):
    """One eager float32 step of `ag` on the batch -> the namespace compare_step takes."""
    loss = ag.train(exp)
    ps = list(ag.q_net.parameters())
    st = [ag.optimizer.state[p] for p in ps]
    return SimpleNamespace(loss=float(loss), grad=H.flat([p.grad for p in ps]), params=H.flat(ps), m=H.flat([s["exp_avg"] for s in st]),
                           v=H.flat([s["exp_avg_sq"] for s in st]), t=int(float(st[0]["step"])))


def test_flat_order_and_offsets_are_the_kernels():
    c = H.case("sweep_B2")
    names = [n for n, _ in c.local.named_parameters()]
    assert tuple(names) == PARAM_NAMES and H.P_TOTAL == P_TOTAL == sum(p.numel() for p in c.local.parameters())
    off, offs = 0, {}
    for n, p in c.local.named_parameters():
        offs[n] = off
        off += p.numel()
    assert offs["features_extractor.sensor_encoder.weight"] == H.O_SW and offs["features_extractor.sensor_encoder.bias"] == H.O_SB
    assert offs["q_net.4.weight"] == H.O_Q4W and offs["q_net.4.bias"] == H.O_Q4B and H.O_Q4B + 9 == P_TOTAL
    assert H.output_rows(8) == ((P_TOTAL - 9 - 64, P_TOTAL - 9), P_TOTAL - 1)


def test_helper_reproduces_the_reference_step_g11():
    """Same tolerances as tests/test_dqn_cpu.py holds the float32 path to against G11 (the reference's own DQN.train step)."""
    Z = np.load(os.path.join(H.GOLDEN, "g11_dqn_train.npz"))
    ag = DQNAgent(device="cpu", buffer_size=4, batch_size=32)
    ag.load(os.path.join(H.GOLDEN, "pretrained_DQN_seed3", "q_net.npz"))
    ag.q_net_target.load_state_dict({k[len("tgt_"):]: torch.from_numpy(Z[k]) for k in Z.files if k.startswith("tgt_")})
    exp = tuple(torch.from_numpy(Z["batch_" + k]) for k in ("observations", "actions", "rewards", "next_observations", "dones"))
    r = H.dqn_f64_step(ag.q_net, ag.q_net_target, exp, H.GAMMA)
    np.testing.assert_allclose(r.loss, float(Z["loss"]), rtol=1e-6)
    np.testing.assert_allclose(r.grad, np.concatenate([Z["grad_" + n].ravel() for n in PARAM_NAMES]), rtol=1e-4, atol=1e-6)
    np.testing.assert_allclose(r.params, np.concatenate([Z["after_" + n].ravel() for n in PARAM_NAMES]), rtol=0, atol=2e-6)
    assert r.norm > H.MAX_NORM and abs(np.linalg.norm(r.grad) - H.MAX_NORM) < 1e-5 and r.t == 1 and r.grad.shape == (P_TOTAL,)


def test_helper_adam_with_history_is_torch_adam():
    """A second and a third step from the moments and step count of the agent's own optimizer: the helper's bias correction and moment updates are torch's."""
    c = H.history_batch(1)
    ag = _cpu_agent(c)
    e = _eager(ag, c.exp)
    for k in (2, 3):
        exp = H.history_batch(k).exp
        r = H.dqn_f64_step(ag.q_net, ag.q_net_target, exp, H.GAMMA, m=e.m, v=e.v, t=e.t)
        e = _eager(ag, exp)
        assert r.t == e.t == k
        np.testing.assert_allclose(r.loss, e.loss, rtol=1e-5)
        np.testing.assert_allclose(r.grad, e.grad, rtol=1e-4, atol=1e-6)
        np.testing.assert_allclose(r.params, e.params, rtol=0, atol=2e-6)
        np.testing.assert_allclose(r.m, e.m, rtol=1e-4, atol=1e-7)
        np.testing.assert_allclose(r.v, e.v, rtol=1e-4, atol=1e-12)
        assert np.abs(r.params - r.p0).max() > 0.5 * H.LR


@pytest.mark.parametrize("name", list(H.CASES))
def test_case_inputs_meet_their_conditions(name):
    """Norm side of 10 (the bisected factors of the threshold pairs land in 8.0-9.6 / 10.4-12.0), Huber branch share and the distance from |d| = 1, actions,
    dones and sonar columns, from the float64 helper alone."""
    c = H.case(name)
    r = H.case_f64(c)
    H.assert_conditions(name, c, r)
    assert tuple(x.dtype for x in c.exp) == (torch.float32, torch.int64, torch.float32, torch.float32, torch.float32)
    assert all(x.shape == s for x, s in zip(c.exp, ((c.B, 26), (c.B, 1), (c.B, 1), (c.B, 26), (c.B, 1))))


def _history(defect=None):
    """Cases d and e along an (eager, CPU) trajectory: per step k (HISTORY_STEPS + 1: the late step, counter set to LATE_T) the float64 step, the float64 step with
    `defect`, and the eager step, all from the state the step meets."""
    c = H.history_batch(1)
    ag = _cpu_agent(c)
    z = np.zeros(H.P_TOTAL)
    m, v, t = z, z, 0
    out = []
    for k in range(1, H.HISTORY_STEPS + 2):
        exp = H.history_batch(k).exp
        if k == H.HISTORY_STEPS + 1:
            for p in ag.q_net.parameters():
                ag.optimizer.state[p]["step"].fill_(float(H.LATE_T))
            t = H.LATE_T
        ref = H.dqn_f64_step(ag.q_net, ag.q_net_target, exp, H.GAMMA, m=m, v=v, t=t)
        bad = H.dqn_f64_step(ag.q_net, ag.q_net_target, exp, H.GAMMA, m=m, v=v, t=t, defect=defect) if defect else None
        e = _eager(ag, exp)
        m, v, t = e.m, e.v, e.t
        out.append((k, ref, bad, e))
    return out


def test_history_batches_meet_their_conditions():
    """Cases d and e at the states an eager run meets: no step near the clip threshold, non-zero moments from step 2 on, the late step at t = 100 000 where both
    bias corrections are 1 to the last bit."""
    for k, ref, _, e in _history():
        H.assert_margin(f"history step {k}", ref)
        assert ref.t == e.t == (k if k <= H.HISTORY_STEPS else H.LATE_T + 1)
        H.compare_step(ref, _as_f32_result(ref), e, f"history step {k}")
    assert ref.t == 100_000 and 1 - H.B1 ** ref.t == 1.0 and 1 - H.B2 ** ref.t == 1.0
    assert np.abs(ref.p0 - H.flat(H.history_batch(1).local.parameters())).max() > 5 * H.LR


def test_clip_threshold_pair_is_one_batch_on_both_sides():
    """The pair at B = 32: one batch, two factors.  The unclipped step's ||p.grad|| is the raw norm, the clipped step's is 10 norm / (norm + 1e-6) -- by the helper
    and by the eager step."""
    lo, hi = H.case("threshold_lo_B32"), H.case("threshold_hi_B32")
    assert all(torch.equal(x, y) for x, y in zip(lo.exp, hi.exp))
    assert not torch.equal(lo.local.q_net[4].weight, hi.local.q_net[4].weight)
    rl, rh = H.case_f64(lo), H.case_f64(hi)
    assert 8.0 <= rl.norm <= 9.6 and 10.4 <= rh.norm <= 12.0
    assert abs(np.linalg.norm(rl.grad) - rl.norm) <= 1e-12 * rl.norm
    want = 10.0 * rh.norm / (rh.norm + 1e-6)
    assert abs(np.linalg.norm(rh.grad) - want) <= 1e-12 * want and want < 10.0
    el, eh = _eager(_cpu_agent(lo), lo.exp), _eager(_cpu_agent(hi), hi.exp)
    assert abs(np.linalg.norm(el.grad) - rl.norm) <= 1e-5 * rl.norm and abs(np.linalg.norm(eh.grad) - want) <= 1e-5 * want


def test_last_tile_case_row_8_comes_from_its_one_row():
    """Case f: q_net.4's row of action 8 gets its gradient from the last row alone -- 1 / 17 of what a batch of that one row gives."""
    c = H.case("last_tile_B17")
    r = H.case_f64(c)
    one = H.dqn_f64_step(c.local, c.target, tuple(x[16:] for x in c.exp), H.GAMMA)
    assert r.norm < H.MAX_NORM and one.norm < H.MAX_NORM
    (lo, hi), b = H.output_rows(8)
    np.testing.assert_allclose(r.grad[lo:hi], one.grad[lo:hi] / 17, rtol=1e-12, atol=0)
    np.testing.assert_allclose(r.grad[b], one.grad[b] / 17, rtol=1e-12)
    assert r.grad[b] != 0


# ---- the tests can fail ---------------------------------------------------------------------------------------------------------------------------
def _as_f32_result(r):
    """A float64 result of the helper as a float32 step would hand it over (rounded to float32: the error of a perfect kernel's stores)."""
    f = lambda x: np.asarray(x, dtype=np.float32).astype(np.float64)
    return SimpleNamespace(loss=float(np.float32(r.loss)), grad=f(r.grad), m=f(r.m), v=f(r.v), params=f(r.params), t=r.t)


def _rejected(ref, wrong, eager, what):
    with pytest.raises(AssertionError) as e:
        H.compare_step(ref, wrong, eager, what)
    return str(e.value)


# defect -> the cases that must reject it (first steps, from zero moments; t_stuck cannot show there: test_t_stuck_shows_only_with_history)
REJECTED_ON = {
    "always_clip": ("sweep_B32", "sweep_B256", "all_quadratic_B32", "threshold_lo_B2", "threshold_lo_B32", "threshold_lo_B256"),
    "mse_everywhere": ("all_linear_B32", "all_linear_B256", "sweep_B32"),
    "done_ignored": ("all_done_B32", "all_done_B256", "last_tile_B17"),
    "target_is_local": ("none_done_B32", "none_done_B256", "sweep_B100"),
    "mean_over_tiles": ("sweep_B1", "sweep_B2", "sweep_B15", "sweep_B17", "sweep_B31", "sweep_B33", "sweep_B100", "sweep_B255", "last_tile_B17"),
    "eps_inside_sqrt": ("sweep_B32", "sweep_B256", "all_quadratic_B32"),      # (small gradient entries: sqrt(1e-8) = 1e-4 is of their size)
}


@pytest.fixture(scope="module")
def steps():
    """name -> (float64 step, eager float32 step) of the named cases, computed once."""
    out = {}
    for name in sorted({n for ns in REJECTED_ON.values() for n in ns} | {"sweep_B16", "sweep_B32", "sweep_B256"}):
        c = H.case(name)
        out[name] = (c, H.case_f64(c), _eager(_cpu_agent(c), c.exp))
    return out


def test_bars_accept_correct_steps(steps):
    """The float64 step rounded to float32, and the eager float32 step itself, pass on every case a defect is shown on."""
    for name, (c, ref, eager) in steps.items():
        H.compare_step(ref, _as_f32_result(ref), eager, name)
        H.compare_step(ref, eager, eager, name)


@pytest.mark.parametrize("defect", list(REJECTED_ON))
def test_bars_reject_a_wrong_step(steps, defect):
    for name in REJECTED_ON[defect]:
        c, ref, eager = steps[name]
        msg = _rejected(ref, _as_f32_result(H.case_f64(c, defect=defect)), eager, f"{name} {defect}")
        print(msg)


def test_mean_over_tiles_is_invisible_at_whole_tiles(steps):
    """Dividing by 16 ceil(B / 16) is dividing by B at B = 16, 32, 256: why the sweep has 15, 17, 31, 33, 255."""
    for name in ("sweep_B16", "sweep_B32", "sweep_B256"):
        c, ref, eager = steps[name]
        bad = H.case_f64(c, defect="mean_over_tiles")
        assert bad.loss == ref.loss and np.array_equal(bad.grad, ref.grad) and np.array_equal(bad.params, ref.params)


def test_t_stuck_shows_only_with_history():
    """Bias corrections of step 1 forever: the first step is the correct one bit for bit; every later step of the history, and the late step, is rejected -- and so
    is a step counter that does not advance."""
    for k, ref, bad, eager in _history("t_stuck"):
        if k == 1:
            assert np.array_equal(bad.params, ref.params) and np.array_equal(bad.m, ref.m)
            continue
        assert "param" in _rejected(ref, _as_f32_result(bad), eager, f"history step {k} t_stuck")
    stuck = _as_f32_result(ref)
    stuck.t = 1
    assert "Adam step" in _rejected(ref, stuck, eager, "late step, counter stuck")


def test_exact_zero_helpers_reject_a_leak():
    # a gradient that leaks into the row of an action nobody took
    c = H.case("one_action0_B32")
    ref = H.case_f64(c)
    H.assert_untaken_actions_untouched(_as_f32_result(ref), ref.p0, 0)
    H.assert_untaken_actions_untouched(_eager(_cpu_agent(c), c.exp), ref.p0, 0)
    (lo, _), b = H.output_rows(5)
    for field in ("grad", "m", "v", "params"):
        for pos in (lo + 3, b):
            bad = _as_f32_result(ref)
            getattr(bad, field)[pos] += 1e-12
            with pytest.raises(AssertionError):
                H.assert_untaken_actions_untouched(bad, ref.p0, 0)
    with pytest.raises(AssertionError):
        H.assert_untaken_actions_untouched(_as_f32_result(ref), ref.p0, 8)
    # observations without a sonar return: same for sensor_encoder.weight
    c = H.case("no_sonar_states_B32")
    ref = H.case_f64(c)
    H.assert_sensor_weight_untouched(_as_f32_result(ref), ref.p0)
    H.assert_sensor_weight_untouched(_eager(_cpu_agent(c), c.exp), ref.p0)
    bad = _as_f32_result(ref)
    bad.grad[H.SENSOR_W.start + 7] = 1e-20
    with pytest.raises(AssertionError):
        H.assert_sensor_weight_untouched(bad, ref.p0)
    with pytest.raises(AssertionError):      # (with a sonar return the weight does learn)
        c = H.case("sweep_B32")
        ref = H.case_f64(c)
        H.assert_sensor_weight_untouched(_as_f32_result(ref), ref.p0)
