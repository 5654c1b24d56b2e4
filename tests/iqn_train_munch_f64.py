"""tests/iqn_train_f64.py's float64 statement of one IQN gradient step with the Munchausen target (include/marinenav_hip.h, "Munchausen target") in place
of the hard max:

    q'[a]   = mean_j Z_target(s', tt_j)[a]        d' = q' - max_a q'        E' = sum_a exp(d'[a] / te)
    tlp'[a] = d'[a] - te log E'                   pi'[a] = exp(d'[a] / te) / E'
    V[j]    = sum_a pi'[a] (Z'[j][a] - tlp'[a])
    q, d, E, tlp likewise from Z_target(s, tm_j)  -- the TARGET weights on the CURRENT state, a tau set of its own
    x[b]    = tlp[a_b]                            bonus = alpha * min(max(x, lo), 0)
    y[b,j]  = r + bonus + gamma_n (1 - done) V[j]

followed by the same loss, clip and Adam.  The rule has no bit-exact host twin (expf / logf), so a float32 evaluation is held to this one by eager float32's own
error: `compare_targets` for y, `H.compare_step` for the step.  Inputs as in that module (CPU generators); `mid_clip` gives the clip bound that clamps exactly half
of a batch's rows, so that one case runs both branches of the clamp.  Plain helper module, no fixtures."""
import copy
import math
from types import SimpleNamespace

import numpy as np
import torch

import iqn_train_f64 as H

ALPHA, TE, LO = 0.9, 0.03, -1.0      # the defaults (Vieillard et al. 2020)
DEFECTS = ("no_clamp", "policy_from_s", "plain_max", "no_entropy", "bonus_without_alpha")


def _policy(z, te):
    """(tlp [B, A], pi [B, A]) of the quantiles z [B, N, A], operation by operation as the header states them."""
    q = z.mean(dim=1)
    d = q - q.max(dim=1, keepdim=True)[0]
    e = (d / te).exp()
    E = e.sum(dim=1, keepdim=True)
    return d - te * E.log(), e / E


def targets(target64, exp, tt, tm, gamma_n, alpha, te, lo, defect=None):
    """(y [B, N], x [B]) in float64 (no graph).  `defect`: None or one of DEFECTS -- one deliberate mistake each (tests of the tests)."""
    states, actions, rewards, next_states, dones = exp
    B = states.shape[0]
    with torch.no_grad():
        zn = H._quantiles(target64, next_states, tt)                      # [B, N, A] over j
        zs = H._quantiles(target64, states, tm)
        tlp, _ = _policy(zs, te)
        tlpn, pin = _policy(zs if defect == "policy_from_s" else zn, te)
        x = tlp.gather(1, actions.view(B, 1))                             # [B, 1]
        clamped = x if defect == "no_clamp" else x.clamp(min=lo, max=0.0)
        bonus = clamped if defect == "bonus_without_alpha" else alpha * clamped
        if defect == "plain_max":
            V, bonus = zn.max(dim=2)[0], torch.zeros_like(bonus)
        elif defect == "no_entropy":
            V = (pin.unsqueeze(1) * zn).sum(dim=2)
        else:
            V = (pin.unsqueeze(1) * (zn - tlpn.unsqueeze(1))).sum(dim=2)  # [B, N]
        y = rewards.double().view(B, 1) + bonus + gamma_n * V * (1.0 - dones.double().view(B, 1))
    return y, x.view(B)


def _td(local64, target64, exp, tt, tm, tl, gamma_n, alpha, te, lo, defect=None):
    states, actions = exp[0], exp[1]
    B = states.shape[0]
    y, x = targets(target64, exp, tt, tm, gamma_n, alpha, te, lo, defect)
    z = H._quantiles(local64, states, tl).gather(2, actions.view(B, 1, 1).expand(B, tl.shape[1], 1)).squeeze(2)      # [B, N] over i
    return y.unsqueeze(1) - z.unsqueeze(2), y, x


def f64_step_munch(local, target, exp, taus_target, taus_munch, taus_local, gamma_n, alpha=ALPHA, te=TE, lo=LO, m=None, v=None, t=0, lr=H.LR, defect=None):
    """H.f64_step with the Munchausen target: the same namespace plus y [B, N] and x [B] = tlp[a_b] (float64 numpy)."""
    local64, target64 = copy.deepcopy(local).double(), copy.deepcopy(target).double()
    params = list(local64.parameters())
    td, y, x = _td(local64, target64, exp, taus_target, taus_munch, taus_local, gamma_n, alpha, te, lo, defect)
    a = td.abs()
    huber = torch.where(a <= 1.0, 0.5 * td * td, a - 0.5)
    weight = (taus_local.double().unsqueeze(2) - (td.detach() < 0).double()).abs()
    loss = (weight * huber).sum(dim=1).mean(dim=1).mean()
    grads = torch.autograd.grad(loss, params)
    g = torch.cat([p.reshape(-1) for p in grads])
    norm = float(torch.linalg.vector_norm(g))
    g = g * min(1.0, H.MAX_NORM / (norm + 1e-6))
    p0 = torch.cat([p.detach().reshape(-1) for p in params])
    dev = p0.device
    m0 = torch.zeros_like(p0) if m is None else torch.as_tensor(m, dtype=torch.float64, device=dev).reshape(-1)
    v0 = torch.zeros_like(p0) if v is None else torch.as_tensor(v, dtype=torch.float64, device=dev).reshape(-1)
    t1 = int(t) + 1
    m1 = H.B1 * m0 + (1 - H.B1) * g
    v1 = H.B2 * v0 + (1 - H.B2) * g * g
    p1 = p0 - lr / (1 - H.B1 ** t1) * m1 / (v1.sqrt() / math.sqrt(1 - H.B2 ** t1) + H.EPS)
    tdd = td.detach()
    n = lambda z: z.cpu().numpy()
    return SimpleNamespace(loss=float(loss.detach()), norm=norm, grad=n(g), params=n(p1), m=n(m1), v=n(v1), t=t1, p0=n(p0), y=n(y), x=n(x),
                           lin_share=float((tdd.abs() > 1.0).double().mean()), min_abs_td=float(tdd.abs().min()),
                           min_kink=float((tdd.abs() - 1.0).abs().min()), max_abs_y=float(y.abs().max()))


def mid_clip(x):
    """The midpoint of the two middle order statistics of x [B] (float64): the clip bound that clamps exactly half the rows.  Returns (bound, half-gap)."""
    xs = np.sort(np.asarray(x, dtype=np.float64).reshape(-1))
    k = xs.size // 2
    return float((xs[k - 1] + xs[k]) / 2), float((xs[k] - xs[k - 1]) / 2)


def settle_rewards(local, target, exp, tt, tm, tl, gamma_n, alpha, te, lo):
    """H.settle_rewards against THIS td: the 64 entries of a row still move together with its reward (x does not depend on it), so the construction carries over."""
    td, y, _ = _td(copy.deepcopy(local).double(), copy.deepcopy(target).double(), exp, tt, tm, tl, gamma_n, alpha, te, lo)
    td = td.detach().reshape(td.shape[0], -1).cpu().numpy()
    w = H.KINK * max(1.0, float(y.abs().max())) * 1.03
    ks = np.zeros(801)
    ks[1::2], ks[2::2] = np.arange(1, 401), -np.arange(1, 401)
    shifts = ks * (w / 2)
    r = exp[2].double().cpu().clone()
    for b in range(td.shape[0]):
        z = td[b][None, :] + shifts[:, None]
        clear = np.minimum(np.abs(z), np.abs(np.abs(z) - 1.0)).min(axis=1) >= 1.5 * w
        k = int(np.argmax(clear))
        assert clear[k], f"row {b}: no reward shift clears the kinks"
        r[b, 0] += shifts[k]
    return r.float().to(exp[2].device)


def small_td_rewards(local, target, exp, tt, tm, tl, gamma_n, alpha, te, lo, delta, g):
    """H.small_td_rewards against this td: r[b] = -mean_ij td0[b] + delta * randn, td0 the td of zero rewards."""
    exp0 = list(exp)
    exp0[2] = torch.zeros_like(exp[2])
    td, _, _ = _td(copy.deepcopy(local).double(), copy.deepcopy(target).double(), exp0, tt, tm, tl, gamma_n, alpha, te, lo)
    B = exp[0].shape[0]
    return (-td.detach().mean(dim=(1, 2)).view(B, 1) + delta * torch.randn(B, 1, generator=g).double()).float()


def munch_case(c, te=TE, lo=LO, alpha=ALPHA, small_td=None, settle=True):
    """`c` (H.build_case(..., settle=False)) with a third tau set, the option's scalars and rewards settled against the Munchausen td.  lo = "mid": mid_clip of the
    case's float64 x.  `small_td` = delta: rewards that make td small (an unclipped gradient norm)."""
    g = torch.Generator().manual_seed(77 + c.B)
    tm = torch.rand(c.B, H.N, generator=g)
    exp = list(c.exp)
    half_gap = None
    if lo == "mid":
        _, x = targets(copy.deepcopy(c.target).double(), c.exp, c.tt, tm, c.gamma_n, alpha, te, 0.0)
        lo, half_gap = mid_clip(x.numpy())
    if small_td is not None:
        exp[2] = small_td_rewards(c.local, c.target, exp, c.tt, tm, c.tl, c.gamma_n, alpha, te, lo, small_td, g)
    if settle:
        exp[2] = settle_rewards(c.local, c.target, exp, c.tt, tm, c.tl, c.gamma_n, alpha, te, lo)
    return SimpleNamespace(local=c.local, target=c.target, exp=tuple(exp), tt=c.tt, tm=tm, tl=c.tl, gamma_n=c.gamma_n, n_step=c.n_step, B=c.B, alpha=alpha, te=te, lo=lo,
                           half_gap=half_gap)


def build(B, te=TE, lo=LO, alpha=ALPHA, small_td=None, settle=True, **kw):
    kw.setdefault("kind", "random")
    return munch_case(H.build_case(B=B, settle=False, **kw), te=te, lo=lo, alpha=alpha, small_td=small_td, settle=settle)


def case_f64(c, **kw):
    return f64_step_munch(c.local, c.target, c.exp, c.tt, c.tm, c.tl, c.gamma_n, c.alpha, c.te, c.lo, **kw)


BATCHES = (2, 16, 18, 32, 256)
# the step cases of tests/test_munchausen_gpu.py beside the batch sweep: name -> (build keywords, conditions as in H.CASES)
STEP_CASES = {name: (dict(H.CASES[name][0], lo="mid"), dict(H.CASES[name][1])) for name in ("all_done_B32", "none_done_B32", "one_action0_B32", "one_action8_B32", "n_step3_B64")}
STEP_CASES["clipped_B32"] = (dict(kind="random", B=32, lo="mid"), dict(clipped=True))
STEP_CASES["unclipped_B32"] = (dict(kind="random", B=32, lo="mid", small_td=0.0), dict(clipped=False))
for _B in BATCHES:
    STEP_CASES[f"sweep_B{_B}"] = (dict(kind="random", B=_B, lo="mid"), dict())


def step_case(name):
    return build(**STEP_CASES[name][0])


def assert_conditions(name, c, r):
    """What the step case `name` relies on, from its float64 result alone: the kink distances and the norm side of H.assert_conditions, and the clamp's split."""
    cond = STEP_CASES[name][1]
    w = H.kink_window(r)
    assert r.min_abs_td >= w and r.min_kink >= w, (name, r.min_abs_td, r.min_kink, w)
    assert abs(r.norm - H.MAX_NORM) > 0.01, (name, r.norm)
    if cond.get("clipped") is True:
        assert r.norm > 0.52, (name, r.norm)
    if cond.get("clipped") is False:
        assert r.norm < 0.45, (name, r.norm)
    if "actions" in cond:
        assert c.exp[1].unique().numel() == cond["actions"]
    kw = STEP_CASES[name][0]
    if kw.get("dones") is not None:
        assert bool((c.exp[4] == float(kw["dones"])).all())
    assert int((r.x < c.lo).sum()) == c.B // 2, (name, int((r.x < c.lo).sum()))


def compare_targets(ref_y, fused_y, eager_y, label="", rows=None):
    """y of a float32 evaluation `fused_y` against float64 under compare_step's bar for a vector: MAX_FACTOR x eager float32's largest error + FLOOR x max |y|.
    The evaluation under test is never its own yardstick.  Returns (error, eager's error, bar)."""
    ref = np.asarray(ref_y, dtype=np.float64)
    assert np.isfinite(ref).all()
    ef = float(np.abs(np.asarray(fused_y, dtype=np.float64) - ref).max())
    ee = float(np.abs(np.asarray(eager_y, dtype=np.float64) - ref).max())
    bar = H.MAX_FACTOR * ee + H.FLOOR * float(np.abs(ref).max())
    line = f"{label:34s} {'y max':14s} fused {ef:10.3e}  eager {ee:10.3e}  bar {bar:10.3e}  max |y| {float(np.abs(ref).max()):8.3f}"
    if rows is not None:
        rows.append(line)
    assert ef <= bar, line
    return ef, ee, bar
