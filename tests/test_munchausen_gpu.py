"""The Munchausen target on the device (`iqn_munch_fwdbwd_kernel`, csrc/iqn_train.hip; include/marinenav_hip.h, "Munchausen target") against the float64 statement
of tests/iqn_train_munch_f64.py: the targets through `targets_out`, the whole step under `H.compare_step` with eager float32 (`IQNAgent.compute_loss` + torch Adam)
as the yardstick, the anchor to the plain kernel, the draws against their host twin, the agent's routing and the trainer's stop and resume."""
import ctypes as C
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import iqn_train_f64 as H              # noqa: E402
import iqn_train_munch_f64 as HM       # noqa: E402
import rng_twin as R                   # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
INVALID = -1      # MN_ERR_INVALID
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def torch():
    import torch as t
    if not t.cuda.is_available():
        pytest.skip("no GPU")
    return t


def _agent(torch, c, **attrs):
    from distributional_rl_navigation_amd.iqn.agent import IQNAgent
    ag = IQNAgent(26, 9, BATCH_SIZE=c.B, n_step=c.n_step, seed=H.NET_SEED, BUFFER_SIZE=64, device=DEV, munchausen=True, m_alpha=c.alpha, m_tau=c.te, m_clip=c.lo)
    ag.qnetwork_local.load_state_dict(c.local.state_dict())
    ag.qnetwork_target.load_state_dict(c.target.state_dict())
    for k, v in attrs.items():
        setattr(ag, k, v)
    ag._fused_trainer()
    return ag


def _dev(c):
    return SimpleNamespace(exp=tuple(x.to(DEV).contiguous() for x in c.exp), tt=c.tt.to(DEV), tm=c.tm.to(DEV), tl=c.tl.to(DEV))


class _State:
    def __init__(self, ag):
        ft = ag._fused_trainer()
        self.ag, self.t = ag, [x.clone() for x in (ft.local, ft.target, ft.exp_avg, ft.exp_avg_sq, ft.step_dev, ft.rng_state)]
        self.grad_steps = ag.grad_steps

    def restore(self):
        from distributional_rl_navigation_amd.iqn.fused_act import weights_changed
        ft = self.ag._fused
        for d, s in zip((ft.local, ft.target, ft.exp_avg, ft.exp_avg_sq, ft.step_dev, ft.rng_state), self.t):
            d.copy_(s)
        self.ag._train_path = "hip"
        self.ag.grad_steps = self.grad_steps
        weights_changed(self.ag.qnetwork_local)


def _result(ag, loss, y=None):
    ft = ag._fused
    ag._enter_train_path("hip")
    ps = list(ag.qnetwork_local.parameters())
    return SimpleNamespace(loss=float(loss), grad=H.flat([p.grad for p in ps]), params=H.flat(ps), m=H.flat([ft.exp_avg]), v=H.flat([ft.exp_avg_sq]),
                           t=int(ft.step_dev.item()), y=None if y is None else y.detach().double().cpu().numpy())


def _fused(torch, ag, d, want_targets=True):
    ft = ag._fused_trainer()
    ag._enter_train_path("hip")
    idx = torch.arange(d.exp[0].shape[0], dtype=torch.int64, device=DEV)
    out = ft.step_munch(d.exp, idx, d.tt, d.tm, d.tl, want_targets=want_targets)
    return _result(ag, *out) if want_targets else _result(ag, out)


def _eager(torch, ag, d):
    """IQNAgent.train's PyTorch step: compute_loss with the option, clip, torch Adam."""
    from distributional_rl_navigation_amd.iqn.fused_act import weights_changed
    ag._enter_train_path("torch")
    ag.optimizer.zero_grad(set_to_none=False)
    loss, y = ag.compute_loss(d.exp, d.tt, d.tl, taus_munch=d.tm, want_targets=True)
    loss.backward()
    torch.nn.utils.clip_grad_norm_(ag.qnetwork_local.parameters(), 0.5)
    ag.optimizer.step()
    weights_changed(ag.qnetwork_local)
    return _result(ag, loss.detach(), y)


def _f64(ag, d):
    ft = ag._fused
    return HM.f64_step_munch(ag.qnetwork_local, ag.qnetwork_target, d.exp, d.tt, d.tm, d.tl, H.GAMMA ** ag.n_step, ag.m_alpha, ag.m_tau, ag.m_clip,
                             m=ft.exp_avg, v=ft.exp_avg_sq, t=int(ft.step_dev.item()))


def _compare(torch, ag, state, d, label, order=("eager", "fused")):
    """Float64, eager and fused from `state`, y and the step under their bars; leaves the agent at the result of the step named last in `order`."""
    state.restore()
    ref = _f64(ag, d)
    out = {}
    for which in order:
        state.restore()
        out[which] = (_fused if which == "fused" else _eager)(torch, ag, d)
    rows = []
    try:
        HM.compare_targets(ref.y, out["fused"].y, out["eager"].y, label, rows)
        H.compare_step(ref, out["fused"], out["eager"], label, rows)
    finally:
        print("\n".join(rows))
    return ref, out["fused"], out["eager"]


# ---- 1. the targets ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", HM.BATCHES)
def test_targets_against_float64(torch, B):
    rows = []
    try:
        for te in (0.03, 1.0):
            for lo in (-1.0, "mid"):
                c = HM.build(B, te=te, lo=lo, settle=False)
                ag, d = _agent(torch, c), _dev(c)
                ref = HM.case_f64(c)
                fused = _fused(torch, ag, d)
                with torch.no_grad():
                    eager = ag.td_targets(d.exp, d.tt, d.tm).view(B, H.N).double().cpu().numpy()
                clamped = int((ref.x < c.lo).sum())
                assert clamped == B // 2 if lo == "mid" else True
                HM.compare_targets(ref.y, fused.y, eager, f"B{B}_te{te}_lo{c.lo:.4f}_clamped{clamped}", rows)
    finally:
        print("\n".join(rows))


# ---- 2. the whole step --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(HM.STEP_CASES))
def test_step_against_float64(torch, name):
    c = HM.step_case(name)
    ag, d = _agent(torch, c), _dev(c)
    ref, fused, eager = _compare(torch, ag, _State(ag), d, name)
    HM.assert_conditions(name, c, ref)


# ---- 3. anchor: every row done, alpha = 0 -> the plain kernel's step ------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [2, 32])
def test_all_done_without_bonus_is_the_plain_kernel_bit_for_bit(torch, B):
    c = HM.build(B, alpha=0.0, dones=1, settle=False)
    ag, d = _agent(torch, c, two_launch_step=False), _dev(c)      # the separate launches: mn_iqn_train_grad + mn_iqn_train_adam
    state = _State(ag)
    ft = ag._fused
    idx = torch.arange(B, dtype=torch.int64, device=DEV)
    plain = _result(ag, ft.step(d.exp, idx, d.tt, d.tl))
    state.restore()
    munch = _fused(torch, ag, d)
    for k in ("grad", "params", "m", "v"):
        assert np.array_equal(getattr(plain, k), getattr(munch, k)), k
    assert plain.loss == munch.loss and plain.t == munch.t == 1
    assert np.array_equal(munch.y, np.broadcast_to(d.exp[2].double().cpu().numpy(), (B, H.N)))


# ---- 4. / 5. position independence; targets_out given or not ------------------------------------------------------------------------------------
def test_reversed_batch_gives_reversed_targets_bit_for_bit(torch):
    c = HM.build(18, lo="mid", settle=False)
    ag, d = _agent(torch, c), _dev(c)
    state = _State(ag)
    y = _fused(torch, ag, d).y
    rev = SimpleNamespace(exp=tuple(x.flip(0).contiguous() for x in d.exp), tt=d.tt.flip(0).contiguous(), tm=d.tm.flip(0).contiguous(), tl=d.tl.flip(0).contiguous())
    state.restore()
    assert np.array_equal(_fused(torch, ag, rev).y, y[::-1])


def test_targets_out_does_not_change_the_gradient(torch):
    c = HM.build(32, lo="mid", settle=False)
    ag, d = _agent(torch, c), _dev(c)
    state = _State(ag)
    a = _fused(torch, ag, d, want_targets=True)
    state.restore()
    b = _fused(torch, ag, d, want_targets=False)
    for k in ("grad", "params", "m", "v"):
        assert np.array_equal(getattr(a, k), getattr(b, k)), k
    assert a.loss == b.loss


# ---- 6. invalid arguments -----------------------------------------------------------------------------------------------------------------------
def test_invalid_arguments_launch_nothing(torch):
    from distributional_rl_navigation_amd import _capi
    B = 32
    c = HM.build(B, settle=False)
    ag, d = _agent(torch, c), _dev(c)
    ft = ag._fused
    s, a, r, ns, dn = d.exp
    idx = torch.arange(B, dtype=torch.int64, device=DEV)
    grad = torch.full_like(ft.grad, -7.0)
    loss = torch.full((1,), -7.0, device=DEV)
    y = torch.full((B, H.N), -7.0, device=DEV)
    ws = ft._workspace(B)
    ws0 = ws.clone()
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    ptrs = dict(s=s, ns=ns, a=a, r=r, dn=dn, idx=idx, tt=d.tt, tm=d.tm, tl=d.tl, pl=ft.local, pt=ft.target, ws=ws, grad=grad, loss=loss)

    def call(batch=B, num_taus=H.N, alpha=0.9, te=0.03, lo=-1.0, null=None, targets=y):
        q = {k: (None if k == null else v) for k, v in ptrs.items()}
        return _capi.lib().mn_iqn_train_grad_munch(*(p(q[k]) for k in ("s", "ns", "a", "r", "dn", "idx", "tt", "tm", "tl", "pl", "pt", "ws", "grad", "loss")), batch, num_taus,
                                                   C.c_float(H.GAMMA), C.c_float(alpha), C.c_float(te), C.c_float(lo), p(targets), _capi.stream_ptr(ag.device))
    nan, inf = float("nan"), float("inf")
    bad = [dict(batch=31), dict(batch=1026), dict(batch=0), dict(num_taus=7), dict(num_taus=32), dict(te=0.0), dict(te=-0.03), dict(te=nan), dict(te=inf),
           dict(lo=1e-3), dict(lo=nan), dict(alpha=-0.1), dict(alpha=nan), dict(alpha=inf)] + [dict(null=k) for k in ptrs]
    for kw in bad:
        assert call(**kw) == INVALID, kw
    torch.cuda.synchronize()
    assert bool((grad == -7.0).all()) and bool((loss == -7.0).all()) and bool((y == -7.0).all()) and torch.equal(ws, ws0)
    assert call() == 0 and call(targets=None) == 0 and call(lo=-inf) == 0 and call(lo=0.0, alpha=0.0) == 0
    torch.cuda.synchronize()
    assert bool((grad != -7.0).any()) and bool((y != -7.0).all())


# ---- 7. the draws -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [2, 32, 256])
def test_sample_three_tau_sets_equals_the_twin(torch, B):
    c = HM.build(2, settle=False)
    ft = _agent(torch, c)._fused
    seed, n = int(ft.rng_state[0]), 2053
    ft.rng_state[1] = 5
    idx3, taus3 = (x.clone() for x in ft.sample(n, B, tau_sets=3))
    assert ft.rng_state.cpu().tolist() == [seed, 6] and taus3.shape == (3, B, 8)
    base = R.sample_base(seed, 5)
    assert idx3.cpu().tolist() == R.perm_row(base, n, np.arange(B)).tolist()
    assert np.array_equal(taus3.cpu().numpy().reshape(-1), R.sample_taus(base, 3 * B * 8))
    ft.rng_state[1] = 5
    idx2, taus2 = ft.sample(n, B)
    assert ft.rng_state.cpu().tolist() == [seed, 6] and taus2.shape == (2, B, 8)
    assert torch.equal(idx2, idx3) and torch.equal(taus2, taus3[:2])
    with pytest.raises(ValueError, match="tau_sets"):
        ft.sample(n, B, tau_sets=4)


# ---- 8. twelve steps with Adam history ----------------------------------------------------------------------------------------------------------
def test_twelve_steps_fused_and_eager_against_float64(torch):
    c0 = HM.build(64, lo="mid", settle=False)
    ag = _agent(torch, c0)
    for k in range(1, 13):
        hb = H.history_batch(k)
        raw = HM.munch_case(hb, te=c0.te, lo=c0.lo, settle=False)
        d = _dev(raw)
        # rewards settled at the state this step meets, as H.settle_case does
        exp = list(d.exp)
        exp[2] = HM.settle_rewards(ag.qnetwork_local, ag.qnetwork_target, d.exp, d.tt, d.tm, d.tl, raw.gamma_n, ag.m_alpha, ag.m_tau, ag.m_clip)
        d.exp = tuple(exp)
        ref, fused, eager = _compare(torch, ag, _State(ag), d, f"history_step_{k}")
        w = H.kink_window(ref)
        assert ref.min_abs_td >= w and ref.min_kink >= w and ref.t == k
        assert 0 < int((ref.x < ag.m_clip).sum()) < 64      # both branches of the clamp in every step
        if k == 6:
            ag._fused.target.copy_(ag._fused.local)


# ---- 9. the agent's routing; a fresh process resumes ----------------------------------------------------------------------------------------------
N_ROWS, STEPS, SAVE_AT = 2053, 12, 5
OPTION = dict(m_alpha=0.7, m_tau=0.05, m_clip=-0.5)      # (away from the defaults: the values must travel)


def _ring_agent(torch):
    from distributional_rl_navigation_amd.iqn.agent import IQNAgent
    ag = IQNAgent(26, 9, BATCH_SIZE=32, seed=H.NET_SEED, BUFFER_SIZE=N_ROWS, device=DEV, munchausen=True, **OPTION)
    g = torch.Generator().manual_seed(77)
    s, a, r, ns, dn = H.random_batch(N_ROWS, g)
    ag.memory.add_batch(s.to(DEV), a.view(-1).to(DEV), r.view(-1).to(DEV), ns.to(DEV), dn.view(-1).to(DEV))
    with torch.no_grad():
        for p in ag.qnetwork_target.parameters():
            p.add_(0.05 * torch.randn(p.shape, generator=g).to(DEV))
    ag._fused_trainer()
    return ag


def _bits(ag, loss):
    ft = ag._fused
    return dict(local=ft.local.cpu(), exp_avg=ft.exp_avg.cpu(), exp_avg_sq=ft.exp_avg_sq.cpu(), step=ft.step_dev.cpu(), loss=loss.detach().cpu().reshape(1).clone(),
                rng=ft.rng_state.cpu())


def test_train_from_memory_is_sample_step_finish_and_resumes_in_a_fresh_process(torch, tmp_path):
    ag = _ring_agent(torch)
    m, ft = ag.memory, ag._fused
    ring = (m.states, m.actions, m.rewards, m.next_states, m.dones)
    assert m.size == N_ROWS
    loss = None
    for k in range(STEPS):
        if k == SAVE_AT:
            torch.save(dict(agent=ag.state_dict(), ring=m.state_dict(), option=OPTION), tmp_path / "state.pt")
        s0 = _State(ag)
        loss = ag.train_from_memory().clone()
        routed = _bits(ag, loss)
        s0.restore()
        idx, taus = ft.sample(m.size, 32, tau_sets=3)
        manual = _bits(ag, ft.step_munch(ring, idx, taus[0], taus[1], taus[2]))
        ag.grad_steps += 1
        for key, v in routed.items():
            assert torch.equal(v, manual[key]), (k, key)
        assert int(ft.rng_state[1]) == k + 1 and ag.grad_steps == k + 1
    straight = _bits(ag, loss)
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "munchausen_resume_child.py"), str(tmp_path / "state.pt"), str(STEPS - SAVE_AT), str(tmp_path / "out.pt")],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-3000:]
    resumed = torch.load(tmp_path / "out.pt")
    for key, v in straight.items():
        assert torch.equal(v, resumed[key]), key
    with pytest.raises(ValueError, match="munchausen"):
        ft.step_sampled(ring, m.size, 32)


# ---- 10. the whole trainer with --munchausen: stop, resume in a fresh process, compare with the uninterrupted run ---------------------------------------
import test_resume_gpu as RG      # noqa: E402  (its toy runs, its child-process launcher and its byte-for-byte file comparison)

M_ARGS = ["--munchausen", "--m-alpha", "0.7", "--m-tau", "0.05", "--m-clip", "-0.5"]


def test_trainer_with_munchausen_stopped_and_resumed_writes_the_files_of_the_straight_run(torch, tmp_path):
    case = dict(RG.LEARNER, args=RG.LEARNER["args"] + ["--n-step", "3", "--n-step-mode", "episode"] + M_ARGS)
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    seed_a, seed_b = (os.path.join(d, "runs", "training_toy", "seed_3") for d in (a, b))
    RG._train(a, case, "--dump-final-state", "final.pt")                                  # A: straight through
    out = RG._train(b, case, "--stop-after", str(RG.STOP))                                # B: stopped behind step 30
    assert f"stopped after vector step {RG.STOP} of {case['vector_steps']}" in out
    ck = torch.load(os.path.join(seed_b, "checkpoint.pt"), map_location="cpu", weights_only=False)
    assert ck["args"]["munchausen"] == dict(alpha=0.7, tau=0.05, clip=-0.5) and int(ck["agent"]["counters"]["grad_steps"]) > 0
    # a resume that leaves --munchausen out is another run: refused, and the key is named
    cmd = [sys.executable, "-m", "distributional_rl_navigation_amd.train_iqn", "-C", "config.json", "-D", DEV, "--run-name", "toy",
           *[x for x in case["args"] if x not in M_ARGS], *RG.COMMON, "--resume", os.path.join("runs", "training_toy")]
    r = subprocess.run(cmd, cwd=b, env=dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", "")), capture_output=True, text=True, timeout=240)
    assert r.returncode != 0 and "other arguments: munchausen was" in r.stderr, r.stderr[-1500:]
    out = RG._train(b, case, "--resume", os.path.join("runs", "training_toy"), "--dump-final-state", "final.pt")      # C: a fresh process continues B's directory
    assert f"continuing from vector step {RG.STOP} (checkpoint.pt)" in out
    files_a = sorted(os.listdir(seed_a))
    assert {"completed.json", "network_params.pth", "greedy_evaluations.npz", "trial_config.json"} <= set(files_a)
    assert sorted(set(os.listdir(seed_b)) - {"checkpoint.pt", "checkpoint.prev.pt"}) == files_a
    for f in files_a:
        RG._same_file(os.path.join(seed_a, f), os.path.join(seed_b, f), f)
    RG._same_file(os.path.join(a, "final.pt"), os.path.join(b, "final.pt"), "final.pt")
