"""A float64 statement of ONE IQN gradient step (thirdparty/IQN/agent.py:269-304 + clip_grad_norm_(0.5) + torch.optim.Adam), the inputs of the
cases tests/test_iqn_train_f64_{cpu,gpu}.py run, and the bars a float32 step is held to against it.  Plain helper module, no fixtures.

    y[b,j]    = r[b] + gamma_n * max_a Z_target(next[b], tau_t[b,j])[a] * (1 - done[b])
    td[b,i,j] = y[b,j] - Z_local(s[b], tau_l[b,i])[a_b]
    huber     = where(|td| <= 1, 0.5 td^2, |td| - 0.5)
    loss      = (|tau_l[b,i] - 1[td < 0]| * huber).sum(i).mean(j).mean(b)
    norm      = ||grad||_2 ; coef = min(1, 0.5 / (norm + 1e-6)) ; g = coef * grad
    m' = 0.9 m + 0.1 g ; v' = 0.999 v + 0.001 g^2 ; t' = t + 1
    p' = p - lr / (1 - 0.9^t') * m' / (sqrt(v') / sqrt(1 - 0.999^t') + 1e-8)

The networks are deep copies cast to double (their `pis` buffer keeps its float32 values: the same function, evaluated exactly); nothing goes
through IQNAgent.compute_loss or F.huber_loss.  All inputs are built with CPU generators, so the CPU file (which asserts the condition a case
relies on: norm side of 0.5, Huber branch share, distance from the loss kinks) and the GPU file (which moves them to the device) see the same
numbers.

Kinks.  1[td < 0] and |td| <= 1 are discontinuities of the gradient: two float32 evaluations on different sides differ by far more than
rounding (the ReLUs are kinks too; those cannot be excluded by construction and are the reason the bar is eager's own error, not a number).  Every case therefore keeps min |td| and min ||td| - 1| at least KINK * max(1, max |y|) away.  A seed search cannot deliver that
beyond a few dozen rows (B = 1024 has 65 536 td entries and ~80 of them inside the window for any seed), so `settle_rewards` constructs it: the
64 td entries of a row move together with its reward, and each row's reward is shifted by the smallest multiple of half the window (at most 200
windows, ~2 % of max |y|) that puts all 64 clear of the three kinks by 1.5 windows.  The condition itself is asserted, from `f64_step`
alone, on the float32 rewards the kernel gets."""
import copy
import math
from types import SimpleNamespace

import numpy as np
import torch

from distributional_rl_navigation_amd.iqn.model import ObsEncoder

GAMMA, LR, MAX_NORM, B1, B2, EPS, N = 0.99, 1e-4, 0.5, 0.9, 0.999, 1e-8, 8
KINK = 1e-4
NET_SEED = 3


def flat(tensors):
    return torch.cat([t.detach().reshape(-1) for t in tensors]).double().cpu().numpy()


def _quantiles(net64, obs, taus):
    return net64(obs.double(), taus.shape[1], 1.0, taus=taus.double())[0]      # [B, N, A]


def _td(local64, target64, exp, tt, tl, gamma_n):
    states, actions, rewards, next_states, dones = exp
    B = states.shape[0]
    with torch.no_grad():
        z_next = _quantiles(target64, next_states, tt).max(dim=2)[0]                                          # [B, N] over j
        y = rewards.double().view(B, 1) + gamma_n * z_next * (1.0 - dones.double().view(B, 1))               # [B, N]
    z = _quantiles(local64, states, tl).gather(2, actions.view(B, 1, 1).expand(B, tl.shape[1], 1)).squeeze(2)    # [B, N] over i
    return y.unsqueeze(1) - z.unsqueeze(2), y                                                                 # td[b, i, j]


def f64_step(local, target, exp, taus_target, taus_local, gamma_n, m=None, v=None, t=0, lr=LR, defect=None):
    """One step in float64 from `local` / `target` (ObsEncoder, any device, not modified).  Returns a namespace: loss, norm (before the clip), grad
    (clipped, flat), params, m, v (flat, after the step), t (after), p0 (flat, before) and three facts about the INPUT: lin_share (share of td
    entries on the linear Huber branch), min_abs_td, min_kink (= min ||td| - 1|), max_abs_y.
    `defect`: None, or one deliberate mistake -- "always_clip", "linear_huber", "t_stuck" -- with which the CPU file shows that the bars reject a
    wrong step (tests of the tests; float64 numbers only)."""
    local64, target64 = copy.deepcopy(local).double(), copy.deepcopy(target).double()
    params = list(local64.parameters())
    td, y = _td(local64, target64, exp, taus_target, taus_local, gamma_n)
    a = td.abs()
    huber = a - 0.5 if defect == "linear_huber" else torch.where(a <= 1.0, 0.5 * td * td, a - 0.5)
    weight = (taus_local.double().unsqueeze(2) - (td.detach() < 0).double()).abs()
    loss = (weight * huber).sum(dim=1).mean(dim=1).mean()
    grads = torch.autograd.grad(loss, params)
    g = torch.cat([x.reshape(-1) for x in grads])
    norm = float(torch.linalg.vector_norm(g))
    coef = MAX_NORM / (norm + 1e-6)
    if defect != "always_clip":
        coef = min(1.0, coef)
    g = g * coef
    p0 = torch.cat([p.detach().reshape(-1) for p in params])
    dev = p0.device
    m0 = torch.zeros_like(p0) if m is None else torch.as_tensor(m, dtype=torch.float64, device=dev).reshape(-1)
    v0 = torch.zeros_like(p0) if v is None else torch.as_tensor(v, dtype=torch.float64, device=dev).reshape(-1)
    t1 = int(t) + 1
    tb = 1 if defect == "t_stuck" else t1
    m1 = B1 * m0 + (1 - B1) * g
    v1 = B2 * v0 + (1 - B2) * g * g
    p1 = p0 - lr / (1 - B1 ** tb) * m1 / (v1.sqrt() / math.sqrt(1 - B2 ** tb) + EPS)
    tdd = td.detach()
    n = lambda x: x.cpu().numpy()
    return SimpleNamespace(loss=float(loss.detach()), norm=norm, grad=n(g), params=n(p1), m=n(m1), v=n(v1), t=t1, p0=n(p0),
                           lin_share=float((tdd.abs() > 1.0).double().mean()), min_abs_td=float(tdd.abs().min()),
                           min_kink=float((tdd.abs() - 1.0).abs().min()), max_abs_y=float(y.abs().max()))


def kink_window(r):
    return KINK * max(1.0, r.max_abs_y)


# ---- inputs (CPU generators) ------------------------------------------------------------------------------------------------------------------------
def make_nets(gen, seed=NET_SEED):
    """Seeded local network and a target that differs from it (local + 0.05 randn), float32 on the CPU."""
    local, target = ObsEncoder(26, 9, seed), ObsEncoder(26, 9, seed)
    with torch.no_grad():
        for p in target.parameters():
            p.add_(0.05 * torch.randn(p.shape, generator=gen))
    return local, target


def random_batch(B, g):
    """tests/test_iqn_gpu.py::_random_batch, drawn on a CPU generator."""
    obs = torch.randn(B, 26, generator=g) * 5
    obs[:, 4:] = torch.where(torch.rand(B, 22, generator=g) < 0.5, torch.zeros(()), obs[:, 4:])
    return [obs, torch.randint(0, 9, (B, 1), generator=g), torch.randn(B, 1, generator=g) * 3,
            obs + 0.3 * torch.randn(B, 26, generator=g), (torch.rand(B, 1, generator=g) < 0.1).float()]


def small_td_rewards(local, target, exp, tt, tl, gamma_n, delta, g):
    """r[b] = mean_i Z_local(s_b, tau_l)[a_b] - gamma_n (1 - done_b) mean_j max_a Z_target(next_b, tau_t) + delta * randn (float64 forward)."""
    exp0 = list(exp)
    exp0[2] = torch.zeros_like(exp[2])
    td, _ = _td(copy.deepcopy(local).double(), copy.deepcopy(target).double(), exp0, tt, tl, gamma_n)      # = y0[b,j] - z[b,i]
    B = exp[0].shape[0]
    noise = torch.randn(B, 1, generator=g).double()
    return (-td.detach().mean(dim=(1, 2)).view(B, 1) + delta * noise).float()


def settle_rewards(local, target, exp, tt, tl, gamma_n):
    """Shift each row's reward by the smallest k * w / 2 (|k| <= 400, w = the kink window) for which its 64 td entries stay 1.5 w clear of 0 and +-1
    (module docstring).  Returns the float32 rewards."""
    td, y = _td(copy.deepcopy(local).double(), copy.deepcopy(target).double(), exp, tt, tl, gamma_n)
    td = td.detach().reshape(td.shape[0], -1).cpu().numpy()
    w = KINK * max(1.0, float(y.abs().max())) * 1.03      # (the shifts may raise max |y| by up to 2 %)
    ks = np.zeros(801)
    ks[1::2], ks[2::2] = np.arange(1, 401), -np.arange(1, 401)
    shifts = ks * (w / 2)
    r = exp[2].double().cpu().clone()
    for b in range(td.shape[0]):
        x = td[b][None, :] + shifts[:, None]
        clear = np.minimum(np.abs(x), np.abs(np.abs(x) - 1.0)).min(axis=1) >= 1.5 * w
        k = int(np.argmax(clear))
        assert clear[k], f"row {b}: no reward shift clears the kinks"
        r[b, 0] += shifts[k]
    return r.float().to(exp[2].device)


def build_case(kind, B, seed=None, delta=0.0, n_step=1, reward_scale=1.0, action=None, dones=None, zero_sonar=None, settle=True):
    """One input: networks, batch, taus.  kind: "random" (_random_batch-style) or "small_td" (rewards from a float64 forward + delta * randn).
    reward_scale multiplies the rewards; action: every row takes this action, or "all" = every action at least once; dones: 0 / 1 for every
    row; zero_sonar: "states" / "next_states" with columns 4..25 zero.  `settle`: keep the rewards clear of the loss kinks."""
    g = torch.Generator().manual_seed(1000 + B if seed is None else seed)
    local, target = make_nets(g)
    exp = random_batch(B, g)
    tt, tl = torch.rand(B, N, generator=g), torch.rand(B, N, generator=g)
    gamma_n = GAMMA ** n_step
    if action == "all":
        exp[1] = (torch.arange(B) % 9)[torch.randperm(B, generator=g)].view(B, 1)
    elif action is not None:
        exp[1] = torch.full((B, 1), int(action), dtype=torch.int64)
    if dones is not None:
        exp[4] = torch.full((B, 1), float(dones))
    if zero_sonar == "states":
        exp[0][:, 4:] = 0.0
    elif zero_sonar == "next_states":
        exp[3][:, 4:] = 0.0
    if kind == "small_td":
        exp[2] = small_td_rewards(local, target, exp, tt, tl, gamma_n, delta, g)
    else:
        assert kind == "random"
    exp[2] = exp[2] * reward_scale
    if settle:
        exp[2] = settle_rewards(local, target, exp, tt, tl, gamma_n)
    return SimpleNamespace(local=local, target=target, exp=tuple(exp), tt=tt, tl=tl, gamma_n=gamma_n, n_step=n_step, B=B)


def case_f64(c, **kw):
    return f64_step(c.local, c.target, c.exp, c.tt, c.tl, c.gamma_n, **kw)


# ---- the cases ------------------------------------------------------------------------------------------------------------------------------------
SWEEP = (2, 16, 18, 48, 100, 128, 256, 384, 512, 1024)
# delta of "small_td" for which the float64 norm lands in 0.40-0.48 / 0.52-0.60 (bisection on f64_step, on the CPU)
THRESHOLD_DELTA = {2: (0.234375, 0.3046875), 32: (0.5625, 0.75)}

# name -> (build_case keywords, conditions): clipped True / False = norm above 0.52 / below 0.45 (None: whichever, but 0.01 away from 0.5); norm = (lo, hi);
# lin_share = exact share of td entries on the linear Huber branch; actions = number of distinct actions
CASES = {}
for _B in SWEEP:      # a. (with these seeds the batches up to 128 clip and those from 256 on do not)
    CASES[f"sweep_B{_B}"] = (dict(kind="random", B=_B), dict(clipped=_B <= 128))
CASES["sweep_B256_clipped"] = (dict(kind="random", B=256, seed=7), dict(clipped=True))
for _B, _d in ((2, 0.0), (32, 0.0), (256, 0.0), (32, 0.2), (256, 0.2)):      # b.
    CASES[f"unclipped_B{_B}_d{_d}"] = (dict(kind="small_td", B=_B, delta=_d), dict(clipped=False))
for _B, (_lo, _hi) in THRESHOLD_DELTA.items():      # c.
    CASES[f"threshold_lo_B{_B}"] = (dict(kind="small_td", B=_B, delta=_lo), dict(norm=(0.40, 0.48)))
    CASES[f"threshold_hi_B{_B}"] = (dict(kind="small_td", B=_B, delta=_hi), dict(norm=(0.52, 0.60)))
# (d. the batches of the 12-step history are settled at the state they meet: history_batch / settle_case)
CASES["n_step3_B64"] = (dict(kind="random", B=64, n_step=3), dict())      # e.
for _B in (32, 256):      # f.
    CASES[f"all_done_B{_B}"] = (dict(kind="random", B=_B, dones=1), dict())
    CASES[f"none_done_B{_B}"] = (dict(kind="random", B=_B, dones=0), dict())
    CASES[f"all_linear_B{_B}"] = (dict(kind="random", B=_B, reward_scale=30.0), dict(lin_share=1.0))
    CASES[f"all_quadratic_B{_B}"] = (dict(kind="small_td", B=_B, delta=0.05), dict(lin_share=0.0, clipped=False))
    CASES[f"one_action0_B{_B}"] = (dict(kind="random", B=_B, action=0), dict(actions=1))
    CASES[f"one_action8_B{_B}"] = (dict(kind="random", B=_B, action=8), dict(actions=1))
    CASES[f"no_sonar_states_B{_B}"] = (dict(kind="random", B=_B, zero_sonar="states"), dict())
    CASES[f"no_sonar_next_B{_B}"] = (dict(kind="random", B=_B, zero_sonar="next_states"), dict())
CASES["every_action_B32"] = (dict(kind="random", B=32, action="all"), dict(actions=9))


def case(name):
    return build_case(**CASES[name][0])


def history_batch(k):
    """Batch and taus of step k = 1.. of the Adam history (case d), rewards not yet settled: that needs the networks the step starts from (settle_case)."""
    return build_case("random", 64, seed=500 + k, settle=False)


def settle_case(c, local, target):
    """`c` with these networks (any device) instead of its own, its batch moved to their device and its rewards settled against them."""
    dev = next(local.parameters()).device
    exp = [x.to(dev) for x in c.exp]
    tt, tl = c.tt.to(dev), c.tl.to(dev)
    exp[2] = settle_rewards(local, target, exp, tt, tl, c.gamma_n)
    return SimpleNamespace(local=local, target=target, exp=tuple(exp), tt=tt, tl=tl, gamma_n=c.gamma_n, n_step=c.n_step, B=c.B)


def assert_conditions(name, c, r):
    """What the GPU case `name` relies on, from the float64 result `r` of its input `c` alone."""
    cond = CASES[name][1]
    w = kink_window(r)
    assert r.min_abs_td >= w and r.min_kink >= w, (name, r.min_abs_td, r.min_kink, w)
    assert abs(r.norm - MAX_NORM) > 0.01, (name, r.norm)
    if cond.get("clipped") is True:
        assert r.norm > 0.52, (name, r.norm)
    if cond.get("clipped") is False:
        assert r.norm < 0.45, (name, r.norm)
    if "norm" in cond:
        assert cond["norm"][0] <= r.norm <= cond["norm"][1], (name, r.norm)
    if "lin_share" in cond:
        assert r.lin_share == cond["lin_share"], (name, r.lin_share)
    if "actions" in cond:
        assert c.exp[1].unique().numel() == cond["actions"] and int(c.exp[1].min()) >= 0 and int(c.exp[1].max()) <= 8
    kw = CASES[name][0]
    if kw.get("dones") is not None:
        assert bool((c.exp[4] == float(kw["dones"])).all())
    if kw.get("zero_sonar"):
        x = c.exp[0] if kw["zero_sonar"] == "states" else c.exp[3]
        assert bool((x[:, 4:] == 0).all()) and float(x[:, :4].abs().min()) > 0


# flat layout (named_parameters() order): velocity 32 + 16, goal 32 + 16, sensor 176 x 22 + 176, ..., output 9 x 64 + 9 at the end
P_TOTAL = 35785
SENSOR_W = slice(96, 96 + 176 * 22)


def output_rows(action):
    """Flat positions of output_layer.weight[action] (start, stop) and of output_layer.bias[action]."""
    w0 = P_TOTAL - 9 - 9 * 64
    return (w0 + 64 * action, w0 + 64 * action + 64), P_TOTAL - 9 + action


def _untouched(res, p0, sel, what):
    p0_32 = np.asarray(p0, dtype=np.float32).astype(np.float64)
    for k in ("grad", "m", "v"):
        assert not np.any(np.asarray(getattr(res, k))[sel] != 0.0), f"{what}: {k} not exactly zero"
    assert np.array_equal(np.asarray(res.params)[sel], p0_32[sel]), f"{what}: parameters moved"


def assert_untaken_actions_untouched(res, p0, taken):
    """Every row took action `taken`: gradient and moments (from zero moments) of the other eight output rows exactly 0.0, their parameters bit for bit where they were."""
    for a in range(9):
        if a != taken:
            (lo, hi), b = output_rows(a)
            _untouched(res, p0, slice(lo, hi), f"output_layer.weight[{a}]")
            _untouched(res, p0, slice(b, b + 1), f"output_layer.bias[{a}]")
    (lo, hi), b = output_rows(taken)
    assert np.abs(np.asarray(res.grad)[lo:hi]).max() > 0 and np.asarray(res.grad)[b] != 0


def assert_sensor_weight_untouched(res, p0):
    """No sonar return in any state: sensor_encoder.weight has an exactly zero gradient and Adam (0 / (0 + eps) from zero moments) leaves it alone."""
    _untouched(res, p0, SENSOR_W, "sensor_encoder.weight")
    assert np.abs(np.asarray(res.grad)[SENSOR_W.stop:SENSOR_W.stop + 176]).max() > 0      # its bias still learns


# ---- the bars ------------------------------------------------------------------------------------------------------------------------------------
MAX_FACTOR, RMS_FACTOR, FLOOR = 1.5, 1.25, 1e-6      # tests/test_dqn_train_fused_gpu.py::_compare_step; tests/test_act_split_gpu.py; the IQN tolerance so far


def _errs(x, ref):
    d = np.abs(np.asarray(x, dtype=np.float64) - ref)
    return float(d.max()), float(np.sqrt(np.mean(d * d)))


def compare_step(ref, fused, eager, label="", rows=None, max_norm=MAX_NORM, lr=LR):
    """A float32 step `fused` and the float32 yardstick `eager` (namespaces: loss, grad, m, v, params, t) against the float64 step `ref` -- the bars of a
    case; raises AssertionError.  Eager PyTorch says how large float32 error is on this input; `fused` is never its own yardstick.  Appends one table line per
    quantity to `rows` (fused error, eager error, ratio) and returns the bars of the loss and of the gradient's largest error.  `max_norm`, `lr`: the clip norm and
    learning rate of the step (the IQN step's by default; tests/dqn_train_f64.py passes the DQN step's)."""
    rows = [] if rows is None else rows
    fails = []

    def line(what, ef, ee, bar):
        rows.append(f"{label:34s} {what:14s} fused {ef:10.3e}  eager {ee:10.3e}  ratio {ef / ee if ee > 0 else float('inf') if ef > 0 else 1.0:7.2f}  bar {bar:10.3e}")
        if not ef <= bar:
            fails.append(rows[-1])

    lbar = MAX_FACTOR * abs(eager.loss - ref.loss) + FLOOR * abs(ref.loss)
    line("loss", abs(fused.loss - ref.loss), abs(eager.loss - ref.loss), lbar)
    gbar = None
    for what, xf, xe, x64 in (("grad", fused.grad, eager.grad, ref.grad), ("exp_avg", fused.m, eager.m, ref.m), ("exp_avg_sq", fused.v, eager.v, ref.v)):
        floor = FLOOR * float(np.abs(x64).max())
        (mf, rf), (me, re) = _errs(xf, x64), _errs(xe, x64)
        line(what + " max", mf, me, MAX_FACTOR * me + floor)
        line(what + " rms", rf, re, RMS_FACTOR * re + floor)
        if what == "grad":
            gbar = MAX_FACTOR * me + floor
    # (not asserted, for the reader of the table: where both float32 steps sit ~1e-4 from float64 with a ratio of 1.00 -- sweep_B384, sweep_B1024 -- they took the same
    # side of a ReLU that float64 takes the other side of; a single (row, tau) flip is worth ~1 / (8 B) of an activation.  Their own distance shows they agree)
    rows.append(f"{label:34s} {'fused-eager':14s} grad max {_errs(fused.grad, np.asarray(eager.grad))[0]:10.3e}  of max |g64| {float(np.abs(ref.grad).max()):10.3e}  (not asserted)")
    # the clip: the branch float64 dictates.  Unclipped: p.grad IS the raw gradient, its norm the norm before the clip; clipped: ||p.grad|| = 0.5 norm / (norm + 1e-6)
    want = ref.norm * min(1.0, max_norm / (ref.norm + 1e-6))
    nf, ne = float(np.linalg.norm(fused.grad)), float(np.linalg.norm(eager.grad))
    line("||grad||", abs(nf - want), abs(ne - want), MAX_FACTOR * abs(ne - want) + FLOOR * want)
    # parameters: where the gradient is well above its own error the update is well conditioned: fused within 2e-6 of eager (the tolerance of
    # test_fused_train_step_equals_pytorch); elsewhere Adam turns rounding into updates of the size of the update itself: bounded by both yardsticks' moves
    pf, pe = np.asarray(fused.params), np.asarray(eager.params)
    big = np.abs(ref.grad) > 100 * gbar
    d = np.abs(pf - pe)
    line("param big", float(d[big].max(initial=0.0)), float(np.abs(pe - ref.params)[big].max(initial=0.0)), 2e-6)
    # (first step: m = v = 0, |update| <= lr; with history |update| can reach lr (1 - b1) / sqrt(1 - b2) ~ 3.2 lr: the moves of the two yardsticks instead)
    rest_bar = np.full_like(d, 2 * lr) if ref.t == 1 else np.abs(ref.params - ref.p0) + np.abs(pe - ref.p0)
    rest = ~big
    rel = lambda x: float((x[rest] / np.maximum(rest_bar[rest], 1e-300)).max(initial=0.0))
    line("param rest", rel(d), rel(np.abs(pe - ref.params)), 1.0)
    if fused.t != ref.t:
        fails.append(f"{label}: Adam step {fused.t}, expected {ref.t}")
    assert not fails, "\n".join(fails)
    return SimpleNamespace(loss=lbar, grad=gbar)
