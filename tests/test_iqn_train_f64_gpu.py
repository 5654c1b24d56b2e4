"""The fused IQN gradient step (csrc/iqn_train.hip, iqn/fused_train.py) against a float64 statement of the same step (tests/iqn_train_f64.py), with
eager float32 PyTorch as the yardstick of how large float32 error is on each input: fused and eager start from the SAME training state and are both
measured against float64; the kernel is never its own yardstick.  Every batch size the bitwise tests cover in every launch form, the unclipped branch
and both sides of the clip threshold, Adam with history one step at a time, the n-step discount, the edges of the loss phase and the in-launch draw
from the replay ring.  The inputs and the conditions they meet are asserted without a GPU in tests/test_iqn_train_f64_cpu.py.
MN_IQN_F64_TABLE=<file>: the error table of the run (profiles/iqn_train_f64_errors.txt)."""
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import iqn_train_f64 as H      # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_ROWS = []


@pytest.fixture(scope="module")
def torch():
    import torch as t
    if not t.cuda.is_available():
        pytest.skip("no GPU")
    yield t
    path = os.environ.get("MN_IQN_F64_TABLE")
    if path and _ROWS:
        import ctypes as C
        from distributional_rl_navigation_amd import _capi
        out = (C.c_double * 5)()
        rc = _capi.lib().mn_probe_mfma_clock(C.c_double(50.0), out, C.c_void_p(t.cuda.current_stream(t.device(DEV)).cuda_stream))
        with open(path, "w") as f:
            f.write("# tests/test_iqn_train_f64_gpu.py: |fused - float64| and |eager float32 - float64| of one IQN gradient step from the same state, per case and quantity\n"
                    "# (max = largest entry, rms over all 35 785; 'param big' = |fused - eager| where |g64| > 100 x the gradient bar, 'param rest' = the same elsewhere as a share of its bar)\n"
                    f"# device: {t.cuda.get_device_name(0)}, clock under f16 matrix load (mn_probe_mfma_clock) {out[1] if rc == 0 else float('nan'):.3f} GHz\n")
            f.write("\n".join(_ROWS) + "\n")


def _agent(torch, c, buffer_size=64, **attrs):
    """A fused agent on the device with the case's networks; `attrs`: two_launch_step / one_launch_step."""
    from distributional_rl_navigation_amd.iqn.agent import IQNAgent
    ag = IQNAgent(26, 9, BATCH_SIZE=c.B, n_step=c.n_step, seed=H.NET_SEED, BUFFER_SIZE=buffer_size, device=DEV)
    assert ag.use_fused_train
    ag.qnetwork_local.load_state_dict(c.local.state_dict())
    ag.qnetwork_target.load_state_dict(c.target.state_dict())
    for k, v in attrs.items():
        setattr(ag, k, v)
    ag._fused_trainer()
    return ag


def _on_device(c):
    return tuple(x.to(DEV) for x in c.exp), c.tt.to(DEV), c.tl.to(DEV)


class _State:
    """Snapshot / restore of a fused agent's whole training state (parameters, target, Adam moments and step)."""

    def __init__(self, ag):
        ft = ag._fused_trainer()
        self.ag, self.t = ag, [x.clone() for x in (ft.local, ft.target, ft.exp_avg, ft.exp_avg_sq, ft.step_dev)]

    def restore(self):
        from distributional_rl_navigation_amd.iqn.fused_act import weights_changed
        ft = self.ag._fused
        for d, s in zip((ft.local, ft.target, ft.exp_avg, ft.exp_avg_sq, ft.step_dev), self.t):
            d.copy_(s)
        self.ag._train_path = "hip"      # the device counter is authoritative: the next eager step takes it over
        weights_changed(self.ag.qnetwork_local)


def _result(ag, loss):
    ft = ag._fused
    ag._enter_train_path("hip")      # (after an eager step: the optimizer's step count back into the device counter)
    ps = list(ag.qnetwork_local.parameters())
    return SimpleNamespace(loss=float(loss), grad=H.flat([p.grad for p in ps]), params=H.flat(ps), m=H.flat([ft.exp_avg]), v=H.flat([ft.exp_avg_sq]),
                           t=int(ft.step_dev.item()))


def _f64(ag, exp, tt, tl):
    ft = ag._fused
    return H.f64_step(ag.qnetwork_local, ag.qnetwork_target, exp, tt, tl, H.GAMMA ** ag.n_step, m=ft.exp_avg, v=ft.exp_avg_sq, t=int(ft.step_dev.item()))


def _fused_step(ag, exp, tt, tl):
    ag.use_fused_train = True
    return _result(ag, ag.train(exp, tt, tl))


def _eager_step(ag, exp, tt, tl):
    ag.use_fused_train = False
    try:
        return _result(ag, ag.train(exp, tt, tl))
    finally:
        ag.use_fused_train = True


def _compare(ag, state, exp, tt, tl, label, fused=None):
    """Float64, the fused step and the eager step from `state`, the two float32 steps against float64 (H.compare_step); `fused`: a fused result
    taken from `state` already.  Leaves the agent at the eager result.  Returns (float64 result, fused result, eager result, bars)."""
    state.restore()
    ref = _f64(ag, exp, tt, tl)
    w = H.kink_window(ref)
    assert ref.min_abs_td >= w and ref.min_kink >= w, (label, ref.min_abs_td, ref.min_kink, w)
    if fused is None:
        fused = _fused_step(ag, exp, tt, tl)
        state.restore()
    eager = _eager_step(ag, exp, tt, tl)
    assert ag._fused.timeouts() == 0
    n0 = len(_ROWS)
    try:
        bars = H.compare_step(ref, fused, eager, label, _ROWS)
    finally:
        print("\n".join(_ROWS[n0:]))
    return ref, fused, eager, bars


def _run_case(torch, name, label=None, **attrs):
    c = H.case(name)
    ag = _agent(torch, c, **attrs)
    exp, tt, tl = _on_device(c)
    state = _State(ag)
    ref, fused, eager, bars = _compare(ag, state, exp, tt, tl, label or name)
    cond = H.CASES[name][1]
    if cond.get("clipped") is not None:      # the input is on the side of the threshold the CPU file asserts
        assert (ref.norm > 0.52) if cond["clipped"] else (ref.norm < 0.45), (name, ref.norm)
    return SimpleNamespace(c=c, ag=ag, state=state, exp=exp, tt=tt, tl=tl, ref=ref, fused=fused, eager=eager, bars=bars)


# ---- a. every batch size, every launch form -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", H.SWEEP)
def test_batch_sweep_default_plan(torch, B):
    r = _run_case(torch, f"sweep_B{B}")
    assert r.ag._fused.launches_per_step(B) == (1 if B % 256 == 0 and B <= 256 else 2)


@pytest.mark.parametrize("form", ["three", "one"])
@pytest.mark.parametrize("B", [16, 18, 48, 100, 128, 256, 384, 1024])
def test_batch_sweep_other_launch_forms(torch, B, form):
    """Three separate launches, and the one-launch step where the library takes it (batch a multiple of 16, a CU per workgroup; two launches otherwise)."""
    attrs = dict(two_launch_step=False) if form == "three" else dict(two_launch_step=True, one_launch_step=True)
    r = _run_case(torch, f"sweep_B{B}", label=f"sweep_B{B} ({form})", **attrs)
    assert r.ag._fused.launches_per_step(B) == (3 if form == "three" else 1 if B in (16, 48, 128, 256) else 2)


def test_clipped_step_at_batch_256(torch):
    _run_case(torch, "sweep_B256_clipped")


# ---- b. the unclipped branch ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,delta", [(2, 0.0), (32, 0.0), (256, 0.0), (32, 0.2), (256, 0.2)])
@pytest.mark.parametrize("form", ["default", "three"])
def test_unclipped_step(torch, B, delta, form):
    """Small TD errors, gradient norm below 0.45: coef = 1, p.grad is the raw gradient.  A step that scaled by 0.5 / norm regardless would be off by more than the bar."""
    r = _run_case(torch, f"unclipped_B{B}_d{delta}", label=f"unclipped_B{B}_d{delta} ({form})", **(dict(two_launch_step=False) if form == "three" else {}))
    ref = r.ref
    assert ref.norm < 0.45 and abs(np.linalg.norm(r.fused.grad) - ref.norm) <= 1e-5 * ref.norm
    if_clipped = ref.grad * (H.MAX_NORM / (ref.norm + 1e-6))
    assert np.abs(if_clipped - ref.grad).max() > 100 * r.bars.grad
    assert np.abs(r.fused.grad - if_clipped).max() > 100 * r.bars.grad


# ---- c. both sides of the threshold -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", list(H.THRESHOLD_DELTA))
def test_both_sides_of_the_clip_threshold(torch, B):
    """One input scaled to a float64 norm of 0.40-0.48 and to 0.52-0.60: the fused step takes the branch float64 dictates; clipped, unclipped, clipped from one
    state: coef is recomputed every step (the third step is the first, bit for bit)."""
    lo, hi = H.case(f"threshold_lo_B{B}"), H.case(f"threshold_hi_B{B}")
    ag = _agent(torch, hi)
    state = _State(ag)
    out = []
    for c, name in ((hi, "hi"), (lo, "lo"), (hi, "hi again")):
        exp, tt, tl = _on_device(c)
        ref, fused, eager, bars = _compare(ag, state, exp, tt, tl, f"threshold_B{B} {name}")
        out.append((ref, fused))
        n = float(np.linalg.norm(fused.grad))
        if name == "lo":
            assert 0.40 <= ref.norm <= 0.48 and abs(n - ref.norm) <= 1e-5 * ref.norm and n < 0.49
        else:
            assert 0.52 <= ref.norm <= 0.60 and abs(n - 0.5) <= 1e-5
    a, b = out[0][1], out[2][1]
    assert a.loss == b.loss and all(np.array_equal(getattr(a, k), getattr(b, k)) for k in ("grad", "params", "m", "v"))


# ---- d. Adam with history, one step at a time ------------------------------------------------------------------------------------------------------
def test_adam_with_history_one_step_at_a_time(torch):
    """12 fused steps from a fresh agent; steps 2, 3, 7 and 12 are each taken fused / eager / float64 from the state in front of them (moments and step count go
    into the float64 step: no trajectory divergence enters): bias correction at t > 1, exp_avg and exp_avg_sq against something other than the kernel."""
    first = H.history_batch(1)
    ag = _agent(torch, first)
    for k in range(1, 13):
        c = H.settle_case(H.history_batch(k), ag.qnetwork_local, ag.qnetwork_target)
        assert int(ag._fused.step_dev.item()) == k - 1
        if k in (2, 3, 7, 12):
            state = _State(ag)
            ref, fused, eager, _ = _compare(ag, state, c.exp, c.tt, c.tl, f"history_B64 step {k}")
            assert ref.t == fused.t == eager.t == k and np.abs(ref.m).max() > 0 and float(state.t[2].abs().max()) > 0
            state.restore()
        _fused_step(ag, c.exp, c.tt, c.tl)
    assert int(ag._fused.step_dev.item()) == 12 and ag._fused.timeouts() == 0


# ---- e. the n-step discount -----------------------------------------------------------------------------------------------------------------------------
def test_n_step_discount_is_gamma_cubed(torch):
    r = _run_case(torch, "n_step3_B64")
    assert r.ag.n_step == 3 and r.c.gamma_n == H.GAMMA ** 3
    one = H.f64_step(r.c.local.to(DEV), r.c.target.to(DEV), r.exp, r.tt, r.tl, H.GAMMA)      # what gamma ** 1 would give: the bars can tell the exponents apart
    assert abs(r.fused.loss - one.loss) > 100 * r.bars.loss and np.abs(r.fused.grad - one.grad).max() > 100 * r.bars.grad


# ---- f. edges of the loss phase -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [32, 256])
def test_all_rows_terminal(torch, B):
    """done = 1 everywhere: y = reward exactly, whatever the (finite) target network and next states hold -- bit for bit."""
    r = _run_case(torch, f"all_done_B{B}")
    ag, ft = r.ag, r.ag._fused
    r.state.restore()
    g = torch.Generator().manual_seed(77)
    with torch.no_grad():
        ft.target.add_((0.3 * torch.randn(ft.target.shape, generator=g)).to(DEV))
    assert not torch.equal(ft.target, r.state.t[1]) and bool(torch.isfinite(ft.target).all())
    exp2 = list(r.exp)
    exp2[3] = (torch.randn(B, 26, generator=g) * 7).to(DEV)
    f2 = _fused_step(ag, tuple(exp2), r.tt, r.tl)
    assert f2.loss == r.fused.loss and all(np.array_equal(getattr(f2, k), getattr(r.fused, k)) for k in ("grad", "params", "m", "v"))


@pytest.mark.parametrize("B", [32, 256])
@pytest.mark.parametrize("edge", ["none_done", "all_linear", "all_quadratic", "no_sonar_next"])
def test_loss_phase_edges(torch, B, edge):
    r = _run_case(torch, f"{edge}_B{B}")
    if edge == "all_linear":
        assert r.ref.lin_share == 1.0
    if edge == "all_quadratic":
        assert r.ref.lin_share == 0.0


@pytest.mark.parametrize("B", [32, 256])
@pytest.mark.parametrize("action", [0, 8])
def test_one_action_in_the_whole_batch(torch, B, action):
    r = _run_case(torch, f"one_action{action}_B{B}")
    H.assert_untaken_actions_untouched(r.fused, r.ref.p0, action)
    H.assert_untaken_actions_untouched(r.eager, r.ref.p0, action)


def test_every_action_present(torch):
    r = _run_case(torch, "every_action_B32")
    for a in range(9):
        (lo, hi), b = H.output_rows(a)
        assert np.abs(r.fused.grad[lo:hi]).max() > 0 and r.fused.grad[b] != 0


@pytest.mark.parametrize("B", [32, 256])
def test_states_without_a_sonar_return(torch, B):
    r = _run_case(torch, f"no_sonar_states_B{B}")
    H.assert_sensor_weight_untouched(r.fused, r.ref.p0)
    H.assert_sensor_weight_untouched(r.eager, r.ref.p0)


# ---- g. from the ring -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [100, 512])
def test_step_drawn_from_the_ring(torch, B):
    """train_from_memory(): the rows and taus the launch drew for itself (ft._idx, ft._taus), gathered here, through the float64 step -- the in-launch draw and
    gather against float64, not only against ft.step.  The draw depends on the generator state and the ring's size alone, so it is looked at first (ft.sample,
    generator state put back) and the rewards of exactly those rows are settled clear of the loss kinks before the step runs."""
    c = H.build_case("random", 2048, seed=900 + B, settle=False)
    c.B = B
    ag = _agent(torch, c, buffer_size=4096)
    s_, a_, r_, n_, d_ = (x.to(DEV) for x in c.exp)
    ag.memory.add_batch(s_, a_.view(-1), r_.view(-1), n_, d_.view(-1))
    m, ft = ag.memory, ag._fused
    rng = ft.rng_state.clone()
    idx, taus = (x.clone() for x in ft.sample(m.size, B))
    ft.rng_state.copy_(rng)
    assert idx.unique().numel() == B and int(idx.min()) >= 0 and int(idx.max()) < 2048
    rows = lambda: (m.states[idx], m.actions[idx], m.rewards[idx], m.next_states[idx], m.dones[idx])
    m.rewards[idx] = H.settle_rewards(ag.qnetwork_local, ag.qnetwork_target, rows(), taus[0], taus[1], H.GAMMA)
    state = _State(ag)
    fused = _result(ag, ag.train_from_memory())
    assert torch.equal(ft._idx[B], idx) and torch.equal(ft._taus[B], taus) and int(ft.rng_state[1]) == int(rng[1]) + 1
    _compare(ag, state, rows(), taus[0], taus[1], f"ring_B{B}", fused=fused)
