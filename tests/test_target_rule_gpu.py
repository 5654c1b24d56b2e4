"""The greedy-on-mean and Double-IQN targets on the device (`iqn_rule_fwdbwd_kernel<RULE>`, csrc/iqn_train.hip; include/marinenav_hip.h, "Target rules") against
the float64 statement of tests/iqn_train_rule_f64.py: a* through `select_out` exactly, the targets through `targets_out` and the whole step under
`HM.compare_targets` / `H.compare_step` with eager float32 (`IQNAgent.compute_loss` + torch Adam) as the yardstick, the bit-for-bit anchors to the plain kernel
and between the two rules, ties, the refused arguments, the agent's routing and the trainer's stop and resume."""
import copy
import ctypes as C
import json
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import iqn_train_f64 as H              # noqa: E402
import iqn_train_munch_f64 as HM       # noqa: E402
import iqn_train_rule_f64 as HR        # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
INVALID = -1      # MN_ERR_INVALID
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BITS = ("grad", "params", "m", "v")


@pytest.fixture(scope="module")
def torch():
    import torch as t
    if not t.cuda.is_available():
        pytest.skip("no GPU")
    return t


def _agent(torch, c, rule=None, **attrs):
    from distributional_rl_navigation_amd.iqn.agent import IQNAgent
    ag = IQNAgent(26, 9, BATCH_SIZE=c.B, n_step=c.n_step, seed=H.NET_SEED, BUFFER_SIZE=64, device=DEV, target_rule=c.rule if rule is None else rule)
    ag.qnetwork_local.load_state_dict(c.local.state_dict())
    ag.qnetwork_target.load_state_dict(c.target.state_dict())
    for k, v in attrs.items():
        setattr(ag, k, v)
    ag._fused_trainer()
    return ag


def _dev(c):
    return SimpleNamespace(exp=tuple(x.to(DEV).contiguous() for x in c.exp), tt=c.tt.to(DEV), ts=c.ts.to(DEV), tl=c.tl.to(DEV))


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


def _result(ag, loss, y=None, sel=None):
    ft = ag._fused
    ag._enter_train_path("hip")
    ps = list(ag.qnetwork_local.parameters())
    return SimpleNamespace(loss=float(loss), grad=H.flat([p.grad for p in ps]), params=H.flat(ps), m=H.flat([ft.exp_avg]), v=H.flat([ft.exp_avg_sq]),
                           t=int(ft.step_dev.item()), y=None if y is None else y.detach().double().cpu().numpy(),
                           y32=None if y is None else y.detach().cpu().numpy().copy(), a_star=None if sel is None else sel.detach().cpu().numpy().astype(np.int64),
                           raw=dict(loss=ft.loss.detach().cpu().numpy().copy().view(np.uint32), grad=ft.grad.detach().cpu().numpy().copy().view(np.uint32),
                                    params=ft.local.detach().cpu().numpy().copy().view(np.uint32), m=ft.exp_avg.detach().cpu().numpy().copy().view(np.uint32),
                                    v=ft.exp_avg_sq.detach().cpu().numpy().copy().view(np.uint32)))


def _fused(torch, ag, d, want=True):
    ft = ag._fused_trainer()
    ag._enter_train_path("hip")
    idx = torch.arange(d.exp[0].shape[0], dtype=torch.int64, device=DEV)
    out = ft.step_rule(d.exp, idx, d.tt, d.ts if ag.target_rule == "double" else None, d.tl, want_targets=want, want_select=want)
    return _result(ag, *out) if want else _result(ag, out)


def _eager(torch, ag, d):
    """IQNAgent.train's PyTorch step: compute_loss with the option, clip, torch Adam."""
    from distributional_rl_navigation_amd.iqn.fused_act import weights_changed
    ag._enter_train_path("torch")
    ag.optimizer.zero_grad(set_to_none=False)
    loss, y = ag.compute_loss(d.exp, d.tt, d.tl, taus_select=d.ts, want_targets=True)
    loss.backward()
    torch.nn.utils.clip_grad_norm_(ag.qnetwork_local.parameters(), 0.5)
    ag.optimizer.step()
    weights_changed(ag.qnetwork_local)
    return _result(ag, loss.detach(), y)


def _f64(ag, d):
    ft = ag._fused
    return HR.f64_step_rule(ag.qnetwork_local, ag.qnetwork_target, d.exp, d.tt, d.ts, d.tl, H.GAMMA ** ag.n_step, ag.target_rule,
                            m=ft.exp_avg, v=ft.exp_avg_sq, t=int(ft.step_dev.item()))


def _compare(torch, ag, state, d, label, order=("eager", "fused")):
    """Float64, eager and fused from `state`: a* exactly, y and the step under their bars; leaves the agent at the result of the step named last in `order`."""
    state.restore()
    ref = _f64(ag, d)
    out = {}
    for which in order:
        state.restore()
        out[which] = (_fused if which == "fused" else _eager)(torch, ag, d)
    rows = []
    try:
        assert np.array_equal(out["fused"].a_star, ref.a_star), label
        HM.compare_targets(ref.y, out["fused"].y, out["eager"].y, label, rows)
        H.compare_step(ref, out["fused"], out["eager"], label, rows)
    finally:
        print("\n".join(rows))
    return ref, out["fused"], out["eager"]


def _same_bits(a, b, keys=("loss",) + BITS):
    for k in keys:
        assert np.array_equal(a.raw[k], b.raw[k]), k
    assert a.t == b.t


# ---- 1. the targets and the chosen actions ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rule", HR.RULES)
@pytest.mark.parametrize("B", HR.BATCHES)
def test_targets_and_select_out_against_float64(torch, B, rule):
    c = HR.build(B, rule, settle=False)
    ag, d = _agent(torch, c), _dev(c)
    ref = HR.case_f64(c)
    fused = _fused(torch, ag, d)
    with torch.no_grad():
        eager = ag.td_targets(d.exp, d.tt, taus_select=d.ts).view(B, H.N).double().cpu().numpy()
    rows = []
    try:
        assert fused.a_star.shape == (B,) and np.array_equal(fused.a_star, ref.a_star)      # every element: nothing is left out
        HM.compare_targets(ref.y, fused.y, eager, f"B{B}_{rule}_distinct{len(set(ref.a_star.tolist()))}", rows)
    finally:
        print("\n".join(rows))


# ---- 2. the whole step --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rule", HR.RULES)
@pytest.mark.parametrize("name", list(HR.STEP_CASES))
def test_step_against_float64(torch, name, rule):
    c = HR.step_case(name, rule)
    ag, d = _agent(torch, c), _dev(c)
    ref, fused, eager = _compare(torch, ag, _State(ag), d, f"{name}_{rule}")
    HR.assert_conditions(name, c, ref)


@pytest.mark.parametrize("rule", HR.RULES)
def test_twelve_steps_fused_and_eager_against_float64(torch, rule):
    ag = _agent(torch, HR.build(HR.HISTORY_B, rule, settle=False))
    for k in range(1, HR.HISTORY_STEPS + 1):
        c = HR.history_case(k, ag.qnetwork_local, ag.qnetwork_target, rule)      # admitted and settled at the state this step meets
        ref, fused, eager = _compare(torch, ag, _State(ag), _dev(c), f"history_step_{k}_{rule}")
        w = H.kink_window(ref)
        assert ref.min_abs_td >= w and ref.min_kink >= w and ref.t == k
        if k == 6:
            ag._fused.target.copy_(ag._fused.local)


# ---- 3. bit-for-bit anchors ---------------------------------------------------------------------------------------------------------------------------
def _plain(torch, ag, d):
    idx = torch.arange(d.exp[0].shape[0], dtype=torch.int64, device=DEV)
    return _result(ag, ag._fused.step(d.exp, idx, d.tt, d.tl))


@pytest.mark.parametrize("rule", HR.RULES)
@pytest.mark.parametrize("B", [2, 32])
def test_all_done_is_the_plain_kernel_bit_for_bit(torch, B, rule):
    c = HR.build(B, rule, dones=1, settle=False)
    ag, d = _agent(torch, c, two_launch_step=False), _dev(c)      # the separate launches: mn_iqn_train_grad + mn_iqn_train_adam
    state = _State(ag)
    plain = _plain(torch, ag, d)
    state.restore()
    ruled = _fused(torch, ag, d)
    _same_bits(plain, ruled)
    assert plain.t == 1
    assert np.array_equal(ruled.y32.view(np.uint32), np.broadcast_to(d.exp[2].cpu().numpy(), (B, H.N)).copy().view(np.uint32))


@pytest.mark.parametrize("B", [2, 32])
def test_mean_with_one_dominant_action_is_the_plain_kernel_bit_for_bit(torch, B):
    """The bias of one action of the target's output layer raised by 1e3: it wins every sample and the mean, so the per-sample max IS the chosen quantile."""
    c = HR.build(B, "mean", settle=False)
    c.target = copy.deepcopy(c.target)
    with torch.no_grad():
        c.target.output_layer.bias[6] += 1e3
    ag, d = _agent(torch, c, two_launch_step=False), _dev(c)
    state = _State(ag)
    plain = _plain(torch, ag, d)
    state.restore()
    mean = _fused(torch, ag, d)
    _same_bits(plain, mean)
    assert (mean.a_star == 6).all()


@pytest.mark.parametrize("B", [2, 18, 32])
def test_double_with_equal_weights_and_equal_taus_is_mean_bit_for_bit(torch, B):
    c = HR.build(B, "double", settle=False)
    c.target = copy.deepcopy(c.local)
    c.ts = c.tt.clone()
    d = _dev(c)
    double = _fused(torch, _agent(torch, c, rule="double"), d)
    mean = _fused(torch, _agent(torch, c, rule="mean"), d)
    _same_bits(double, mean)
    assert np.array_equal(double.a_star, mean.a_star) and np.array_equal(double.y32.view(np.uint32), mean.y32.view(np.uint32))
    assert len(set(mean.a_star.tolist())) > 1 or B == 2


@pytest.mark.parametrize("rule", HR.RULES)
def test_reversed_batch_gives_reversed_targets_and_choices_bit_for_bit(torch, rule):
    c = HR.build(18, rule, settle=False)
    ag, d = _agent(torch, c), _dev(c)
    state = _State(ag)
    a = _fused(torch, ag, d)
    rev = SimpleNamespace(exp=tuple(x.flip(0).contiguous() for x in d.exp), tt=d.tt.flip(0).contiguous(), ts=d.ts.flip(0).contiguous(), tl=d.tl.flip(0).contiguous())
    state.restore()
    b = _fused(torch, ag, rev)
    assert np.array_equal(b.y32.view(np.uint32), a.y32[::-1].copy().view(np.uint32)) and np.array_equal(b.a_star, a.a_star[::-1])
    assert len(set(a.a_star.tolist())) > 1


@pytest.mark.parametrize("rule", HR.RULES)
def test_the_outputs_do_not_change_the_gradient(torch, rule):
    c = HR.build(32, rule, settle=False)
    ag, d = _agent(torch, c), _dev(c)
    state = _State(ag)
    a = _fused(torch, ag, d, want=True)
    state.restore()
    b = _fused(torch, ag, d, want=False)
    _same_bits(a, b)


# ---- 4. ties --------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rule", HR.RULES)
@pytest.mark.parametrize("B", [2, 18, 32])
def test_ties_take_the_first_index(torch, B, rule):
    c = HR.tie_case(B, rule)
    ag, d = _agent(torch, c), _dev(c)
    ref = HR.case_f64(c)
    fused = _fused(torch, ag, d)
    with torch.no_grad():
        eager = ag.td_targets(d.exp, d.tt, taus_select=d.ts).view(B, H.N).double().cpu().numpy()
    assert (ref.a_star == 2).all() and (fused.a_star == 2).all()
    HM.compare_targets(ref.y, fused.y, eager, f"tie_B{B}_{rule}")
    if rule == "double":      # y follows action 2 (bias +10), not action 5 (bias -10)
        wrong = HR.case_f64(c, defect="last_index_ties")
        assert np.abs(fused.y - ref.y).max() < 1e-2 < 1.0 < np.abs(wrong.y - ref.y)[(d.exp[4].view(-1) == 0).cpu().numpy()].min()


# ---- 5. invalid arguments -------------------------------------------------------------------------------------------------------------------------------
def test_invalid_arguments_launch_nothing(torch):
    from distributional_rl_navigation_amd import _capi
    B = 32
    c = HR.build(B, "double", settle=False)
    ag, d = _agent(torch, c), _dev(c)
    ft = ag._fused
    s, a, r, ns, dn = d.exp
    idx = torch.arange(B, dtype=torch.int64, device=DEV)
    grad = torch.full_like(ft.grad, -7.0)
    loss = torch.full((1,), -7.0, device=DEV)
    y = torch.full((B, H.N), -7.0, device=DEV)
    sel = torch.full((B,), -7, dtype=torch.int32, device=DEV)
    ws = ft._workspace(B)
    ws0 = ws.clone()
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    ptrs = dict(s=s, ns=ns, a=a, r=r, dn=dn, idx=idx, pl=ft.local, pt=ft.target, ws=ws, grad=grad, loss=loss, tt=d.tt, ts=d.ts, tl=d.tl)

    def call(batch=B, num_taus=H.N, rule=2, null=None, targets=y, select=sel):
        q = {k: (None if k == null else v) for k, v in ptrs.items()}
        return _capi.lib().mn_iqn_train_grad_rule(*(p(q[k]) for k in ("s", "ns", "a", "r", "dn", "idx", "pl", "pt", "ws", "grad", "loss", "tt", "ts", "tl")), batch, num_taus,
                                                  C.c_float(H.GAMMA), rule, p(targets), p(select), _capi.stream_ptr(ag.device))
    bad = [dict(batch=31), dict(batch=1026), dict(batch=0), dict(batch=-2), dict(num_taus=7), dict(num_taus=32), dict(rule=0), dict(rule=3), dict(rule=-1)]
    bad += [dict(null=k) for k in ptrs] + [dict(null=k, rule=1) for k in ptrs if k != "ts"]
    for kw in bad:
        assert call(**kw) == INVALID, kw
    torch.cuda.synchronize()
    assert bool((grad == -7.0).all()) and bool((loss == -7.0).all()) and bool((y == -7.0).all()) and bool((sel == -7).all())
    assert torch.equal(ws.view(torch.int32), ws0.view(torch.int32))      # word for word
    assert call() == 0 and call(targets=None) == 0 and call(select=None) == 0 and call(rule=1, null="ts") == 0 and call(rule=1) == 0
    torch.cuda.synchronize()
    assert bool((grad != -7.0).any()) and bool((y != -7.0).all()) and bool(((sel >= 0) & (sel <= 8)).all())


# ---- 6. the agent's routing ------------------------------------------------------------------------------------------------------------------------------
N_ROWS, STEPS = 2053, 6


def _ring_agent(torch, rule):
    from distributional_rl_navigation_amd.iqn.agent import IQNAgent
    ag = IQNAgent(26, 9, BATCH_SIZE=32, seed=H.NET_SEED, BUFFER_SIZE=N_ROWS, device=DEV, target_rule=rule)
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


@pytest.mark.parametrize("rule", HR.RULES)
def test_train_from_memory_is_sample_step_finish(torch, rule):
    ag = _ring_agent(torch, rule)
    m, ft = ag.memory, ag._fused
    ring = (m.states, m.actions, m.rewards, m.next_states, m.dones)
    sets = 3 if rule == "double" else 2
    for k in range(STEPS):
        s0 = _State(ag)
        routed = _bits(ag, ag.train_from_memory().clone())
        s0.restore()
        idx, taus = ft.sample(m.size, 32, tau_sets=sets)
        assert taus.shape == (sets, 32, 8)
        manual = _bits(ag, ft.step_rule(ring, idx, taus[0], taus[2] if rule == "double" else None, taus[1]))
        ag.grad_steps += 1
        for key, v in routed.items():
            assert torch.equal(v, manual[key]), (k, key)
        assert int(ft.rng_state[1]) == k + 1 and ag.grad_steps == k + 1
    with pytest.raises(ValueError, match="target_rule.*step_sampled"):
        ft.step_sampled(ring, m.size, 32)
    # injected taus through IQNAgent.train: the same step as step_rule on an arange
    s0 = _State(ag)
    idx, taus = (x.clone() for x in ft.sample(m.size, 32, tau_sets=3))
    exp = (m.states[idx], m.actions[idx].view(-1, 1), m.rewards[idx].view(-1, 1), m.next_states[idx], m.dones[idx].view(-1, 1))
    s0.restore()
    a = _bits(ag, ag.train(exp, taus[0], taus[1], taus_select=taus[2] if rule == "double" else None).clone())
    s0.restore()
    b = _bits(ag, ft.step_rule(ring, idx, taus[0], taus[2] if rule == "double" else None, taus[1]))
    for key in ("local", "exp_avg", "exp_avg_sq", "loss"):
        assert torch.equal(a[key], b[key]), key


# ---- 7. the whole trainer: stop, resume in a fresh process, compare with the uninterrupted run ---------------------------------------------------------------
import test_resume_gpu as RG      # noqa: E402  (its toy runs and its byte-for-byte file comparison)


def _child(cwd, case, *extra, ok=True):
    """One train_iqn run in a child process of its own (tests/target_rule_resume_child.py) in `cwd`."""
    os.makedirs(cwd, exist_ok=True)
    with open(os.path.join(cwd, "config.json"), "w") as f:
        json.dump(dict(agent="IQN", seed=3, save_dir="runs", **case["config"]), f)
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "target_rule_resume_child.py"), DEV, *case["args"], *RG.COMMON, *extra], cwd=cwd, env=env,
                       capture_output=True, text=True, timeout=240)
    assert (r.returncode == 0) == ok, (r.stdout[-1500:], r.stderr[-3000:])
    return r.stdout if ok else r.stderr


def _same_run(a, b, extra_b=()):
    seed_a, seed_b = (os.path.join(d, "runs", "training_toy", "seed_3") for d in (a, b))
    files_a = sorted(os.listdir(seed_a))
    assert {"completed.json", "network_params.pth", "greedy_evaluations.npz", "trial_config.json"} <= set(files_a)
    assert sorted(set(os.listdir(seed_b)) - set(extra_b)) == files_a
    for f in files_a:
        RG._same_file(os.path.join(seed_a, f), os.path.join(seed_b, f), f)
    RG._same_file(os.path.join(a, "final.pt"), os.path.join(b, "final.pt"), "final.pt")


@pytest.mark.parametrize("rule", HR.RULES)
def test_trainer_stopped_and_resumed_writes_the_files_of_the_straight_run(torch, tmp_path, rule):
    case = dict(RG.LEARNER, args=RG.LEARNER["args"] + ["--n-step", "3", "--n-step-mode", "episode", "--target-rule", rule])
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    _child(a, case, "--dump-final-state", "final.pt")                                  # A: straight through
    out = _child(b, case, "--stop-after", str(RG.STOP))                                # B: stopped behind step 30
    assert f"stopped after vector step {RG.STOP} of {case['vector_steps']}" in out
    ck = torch.load(os.path.join(b, "runs", "training_toy", "seed_3", "checkpoint.pt"), map_location="cpu", weights_only=False)
    assert ck["args"]["target_rule"] == rule and int(ck["agent"]["counters"]["grad_steps"]) > 0
    # a resume under another rule is another run: refused, and the key is named
    other = dict(case, args=[x for x in case["args"] if x not in ("--target-rule", rule)])
    err = _child(b, other, "--resume", os.path.join("runs", "training_toy"), ok=False)
    assert "other arguments: target_rule was" in err, err[-1500:]
    out = _child(b, case, "--resume", os.path.join("runs", "training_toy"), "--dump-final-state", "final.pt")      # C: a fresh process continues B's directory
    assert f"continuing from vector step {RG.STOP} (checkpoint.pt)" in out
    _same_run(a, b, extra_b=("checkpoint.pt", "checkpoint.prev.pt"))


def test_trainer_with_target_rule_max_writes_the_files_of_a_run_without_the_flag(torch, tmp_path):
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    _child(a, RG.LEARNER, "--dump-final-state", "final.pt")
    _child(b, dict(RG.LEARNER, args=RG.LEARNER["args"] + ["--target-rule", "max"]), "--dump-final-state", "final.pt")
    _same_run(a, b)
