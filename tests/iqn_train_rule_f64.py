"""tests/iqn_train_f64.py's float64 statement of one IQN gradient step with a greedy-on-mean target (include/marinenav_hip.h, "Target rules") in place of the
per-sample max:

    Zs[j][a] = Z_target(s', tt_j)[a]   ("mean")      or   Z_local(s', ts_j)[a]   ("double": the LOCAL weights on the NEXT state, a tau set of its own)
    q[a]     = mean_j Zs[j][a]         a* = the first argmax_a q[a]
    y[b,j]   = r + gamma_n (1 - done) Z_target(s', tt_j)[a*]

followed by the same loss, clip and Adam.  A float32 evaluation is held to this one by eager float32's own error: `HM.compare_targets` for y, `H.compare_step` for
the step; a* is compared exactly.

Admission.  A hard argmax makes y discontinuous in q: an element whose two best means lie within rounding of each other may pick either action in float32, and
the two y are far apart.  The cases are therefore BUILT for a clear decision: `build` draws 4 B candidate transitions and keeps the first B whose float64 gap
between the best and the second-best selecting mean -- under BOTH rules, a case serves both -- is at least ADMIT x the largest |eager float32 mean - float64 mean|
over all candidates, measured there on the CPU.  It fails loudly if fewer than B qualify: no element is ever left out of a comparison.  The two networks are
seeded independently (the local network is no perturbation of the target), so that the two rules choose different actions on a good share of the elements.
Plain helper module, no fixtures."""
import copy
import math
from types import SimpleNamespace

import numpy as np
import torch

import iqn_train_f64 as H
from distributional_rl_navigation_amd.iqn.model import ObsEncoder

RULES = ("mean", "double")
ADMIT = 1000.0
CANDIDATES = 4      # x B
NET_NOISE = 0.1
# one deliberate mistake each (tests of the tests) -> the rules it can be made under
DEFECTS = {"per_sample_max": RULES, "selector_from_target": ("double",), "selector_on_s": RULES, "last_index_ties": RULES, "mean_over_actions": RULES}


def make_nets(seed=H.NET_SEED):
    """Two independently seeded networks, float32 on the CPU, each parameter moved by NET_NOISE x randn: a freshly initialised network prefers one action on
    nearly every state (one distinct a* in a batch of 256), which would leave the choice untested; moved so, a batch of 32 chooses five different actions and
    most elements choose another action on s than on s'."""
    g = torch.Generator().manual_seed(17)
    nets = []
    for k in range(2):
        net = ObsEncoder(26, 9, seed + k)
        with torch.no_grad():
            for p in net.parameters():
                p.add_(NET_NOISE * torch.randn(p.shape, generator=g))
        nets.append(net)
    return tuple(nets)


def select_means(local64, target64, exp, tt, ts, rule, defect=None):
    """q [B, A] in float64: the mean over the samples of the selecting quantiles."""
    states, next_states = exp[0], exp[3]
    obs = states if defect == "selector_on_s" else next_states
    with torch.no_grad():
        if rule == "double" and defect != "selector_from_target":
            zs = H._quantiles(local64, obs, ts)
        else:
            zs = H._quantiles(target64, obs, ts if rule == "double" else tt)
    return zs.mean(dim=1)


def first_argmax(q, last=False):
    """The first (or, `last`, the last) index that attains each row's maximum."""
    A = q.shape[1]
    hit = q == q.max(dim=1, keepdim=True)[0]
    idx = torch.arange(A, device=q.device).expand_as(q)
    return torch.where(hit, idx, torch.full_like(idx, -1)).max(dim=1)[0] if last else torch.where(hit, idx, torch.full_like(idx, A)).min(dim=1)[0]


def targets(local64, target64, exp, tt, ts, gamma_n, rule, defect=None):
    """(y [B, N], a* [B]) in float64 (no graph)."""
    assert rule in RULES and (defect is None or rule in DEFECTS[defect])
    states, actions, rewards, next_states, dones = exp
    B = states.shape[0]
    with torch.no_grad():
        zn = H._quantiles(target64, next_states, tt)                      # [B, N, A] over j
        if defect == "mean_over_actions":      # the mean taken over the wrong axis: an index of a SAMPLE, used as an action
            zsel = H._quantiles(local64 if rule == "double" else target64, next_states, ts if rule == "double" else tt)
            a_star = first_argmax(zsel.mean(dim=2))
        else:
            a_star = first_argmax(select_means(local64, target64, exp, tt, ts, rule, defect), last=defect == "last_index_ties")
        v = zn.max(dim=2)[0] if defect == "per_sample_max" else zn.gather(2, a_star.view(B, 1, 1).expand(B, zn.shape[1], 1)).squeeze(2)
        y = rewards.double().view(B, 1) + gamma_n * v * (1.0 - dones.double().view(B, 1))
    return y, a_star


def _td(local64, target64, exp, tt, ts, tl, gamma_n, rule, defect=None):
    states, actions = exp[0], exp[1]
    B = states.shape[0]
    y, a_star = targets(local64, target64, exp, tt, ts, gamma_n, rule, defect)
    z = H._quantiles(local64, states, tl).gather(2, actions.view(B, 1, 1).expand(B, tl.shape[1], 1)).squeeze(2)      # [B, N] over i
    return y.unsqueeze(1) - z.unsqueeze(2), y, a_star


def f64_step_rule(local, target, exp, taus_target, taus_select, taus_local, gamma_n, rule, m=None, v=None, t=0, lr=H.LR, defect=None):
    """H.f64_step under `rule`: the same namespace plus y [B, N] (float64 numpy) and a_star [B] (int64 numpy)."""
    local64, target64 = copy.deepcopy(local).double(), copy.deepcopy(target).double()
    params = list(local64.parameters())
    td, y, a_star = _td(local64, target64, exp, taus_target, taus_select, taus_local, gamma_n, rule, defect)
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
    return SimpleNamespace(loss=float(loss.detach()), norm=norm, grad=n(g), params=n(p1), m=n(m1), v=n(v1), t=t1, p0=n(p0), y=n(y), a_star=n(a_star),
                           lin_share=float((tdd.abs() > 1.0).double().mean()), min_abs_td=float(tdd.abs().min()),
                           min_kink=float((tdd.abs() - 1.0).abs().min()), max_abs_y=float(y.abs().max()))


def settle_rewards(local, target, exp, tt, ts, tl, gamma_n, rule):
    """H.settle_rewards against THIS td: the 64 entries of a row still move together with its reward (a* does not depend on it)."""
    td, y, _ = _td(copy.deepcopy(local).double(), copy.deepcopy(target).double(), exp, tt, ts, tl, gamma_n, rule)
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


# ---- admission ----------------------------------------------------------------------------------------------------------------------------------------
def eager_means(local, target, next_states, tt, ts, rule):
    """The selecting means in eager float32 on the CPU, summed as the header states it."""
    with torch.no_grad():
        zs = local(next_states, tt.shape[1], 1.0, taus=ts)[0] if rule == "double" else target(next_states, tt.shape[1], 1.0, taus=tt)[0]
        s = zs[:, 0]
        for j in range(1, zs.shape[1]):
            s = s + zs[:, j]
    return 0.125 * s


def admit(local, target, exp, tt, ts, B):
    """The first B of the candidate rows of `exp` whose float64 top-two gap of the selecting means is at least ADMIT x the largest eager-float32 error of those
    means over ALL candidates, under both rules.  Returns (indices [B], report); raises if fewer than B qualify.  CPU tensors and CPU networks."""
    local64, target64 = copy.deepcopy(local).double(), copy.deepcopy(target).double()
    ok = torch.ones(exp[0].shape[0], dtype=torch.bool)
    report = {}
    for rule in RULES:
        q64 = select_means(local64, target64, exp, tt, ts, rule)
        err = float((eager_means(local, target, exp[3], tt, ts, rule).double() - q64).abs().max())
        top = q64.topk(2, dim=1)[0]
        gap = top[:, 0] - top[:, 1]
        ok &= gap >= ADMIT * err
        report[rule] = dict(err=err, need=ADMIT * err, admitted=int((gap >= ADMIT * err).sum()))
    keep = torch.nonzero(ok).view(-1)
    assert keep.numel() >= B, f"admission: {keep.numel()} of {ok.numel()} candidates have a clear greedy action, {B} are needed ({report})"
    report["candidates"], report["qualified"] = int(ok.numel()), int(keep.numel())
    return keep[:B], report


def candidates(B, seed):
    """CANDIDATES x B transitions and three tau sets, drawn on a CPU generator.  The next states are observations drawn on their own, not H.random_batch's
    perturbed states: close to its state, a next state nearly always has the state's greedy action, and a selector evaluated on s would pass for one on s'."""
    g = torch.Generator().manual_seed(seed)
    n = CANDIDATES * B
    exp = H.random_batch(n, g)
    exp[3] = H.random_batch(n, g)[0]
    return exp, torch.rand(n, H.N, generator=g), torch.rand(n, H.N, generator=g), torch.rand(n, H.N, generator=g)


def take(exp, tt, ts, tl, keep):
    return [x[keep].contiguous() for x in exp], tt[keep].contiguous(), ts[keep].contiguous(), tl[keep].contiguous()


def build(B, rule, seed=None, n_step=1, action=None, dones=None, settle=True, nets=None):
    """One input under `rule`: networks, an admitted batch, three tau sets.  action: every row takes this action; dones: 0 / 1 for every row; `settle`: keep
    the rewards clear of the loss kinks (against this rule's td).  The batch and the taus do not depend on `rule`: the admission is under both."""
    local, target = make_nets() if nets is None else nets
    exp, tt, ts, tl = candidates(B, 3000 + B if seed is None else seed)
    keep, report = admit(local, target, exp, tt, ts, B)
    exp, tt, ts, tl = take(exp, tt, ts, tl, keep)
    gamma_n = H.GAMMA ** n_step
    if action is not None:
        exp[1] = torch.full((B, 1), int(action), dtype=torch.int64)
    if dones is not None:
        exp[4] = torch.full((B, 1), float(dones))
    if settle:
        exp[2] = settle_rewards(local, target, exp, tt, ts, tl, gamma_n, rule)
    return SimpleNamespace(local=local, target=target, exp=tuple(exp), tt=tt, ts=ts, tl=tl, gamma_n=gamma_n, n_step=n_step, B=B, rule=rule, report=report)


def case_f64(c, **kw):
    return f64_step_rule(c.local, c.target, c.exp, c.tt, c.ts, c.tl, c.gamma_n, c.rule, **kw)


def tie_case(B, rule):
    """Identical output-layer rows for actions 2 and 5 in the SELECTING network, their bias raised so that the two tie for the maximum of every mean (one
    instruction sequence on equal operands: equal words, in any precision).  "double": the selector is the local network, and the target's biases of 2 and 5 are set
    far apart (+10 and -10), so the choice shows in y.  "mean": the selector is the target itself, so Z'[j][2] == Z'[j][5] and the choice shows in a* alone."""
    c = build(B, rule, settle=False)
    local, target = copy.deepcopy(c.local), copy.deepcopy(c.target)
    with torch.no_grad():
        sel = local if rule == "double" else target
        sel.output_layer.weight[5] = sel.output_layer.weight[2]
        sel.output_layer.bias[2] = 1e3
        sel.output_layer.bias[5] = 1e3
        if rule == "double":
            target.output_layer.bias[2] = 10.0
            target.output_layer.bias[5] = -10.0
    c.local, c.target = local, target
    return c


BATCHES = (2, 16, 18, 32, 256)
# the step cases of tests/test_target_rule_gpu.py: name -> build keywords
STEP_CASES = {"all_done_B32": dict(B=32, dones=1), "none_done_B32": dict(B=32, dones=0), "one_action0_B32": dict(B=32, action=0), "one_action8_B32": dict(B=32, action=8),
              "n_step3_B64": dict(B=64, n_step=3)}
HISTORY_B, HISTORY_STEPS = 64, 12


def step_case(name, rule):
    return build(rule=rule, **STEP_CASES[name])


def assert_conditions(name, c, r):
    """What the step case `name` relies on, from its float64 result alone: the kink distances and the norm side of H.assert_conditions."""
    w = H.kink_window(r)
    assert r.min_abs_td >= w and r.min_kink >= w, (name, r.min_abs_td, r.min_kink, w)
    assert abs(r.norm - H.MAX_NORM) > 0.01, (name, r.norm)
    kw = STEP_CASES[name]
    if kw.get("action") is not None:
        assert bool((c.exp[1] == kw["action"]).all())
    if kw.get("dones") is not None:
        assert bool((c.exp[4] == float(kw["dones"])).all())


def history_candidates(k):
    """The candidates of step k = 1.. of the Adam history; admitted and settled at the networks the step starts from (`history_case`)."""
    return candidates(HISTORY_B, 5000 + k)


def history_case(k, local, target, rule):
    """Step k's batch admitted against CPU copies of these networks (any device) and settled against them."""
    lc, tc = copy.deepcopy(local).cpu().float(), copy.deepcopy(target).cpu().float()
    exp, tt, ts, tl = history_candidates(k)
    keep, report = admit(lc, tc, exp, tt, ts, HISTORY_B)
    exp, tt, ts, tl = take(exp, tt, ts, tl, keep)
    exp[2] = settle_rewards(lc, tc, exp, tt, ts, tl, H.GAMMA, rule)
    return SimpleNamespace(local=lc, target=tc, exp=tuple(exp), tt=tt, ts=ts, tl=tl, gamma_n=H.GAMMA, n_step=1, B=HISTORY_B, rule=rule, report=report)


def non_degenerate(c):
    """(share of elements whose a* differs between the two rules, share with some sample whose per-sample max is not Z'[j][a*] under c.rule, share whose a* under
    c.rule is another with the selector on s instead of s'), float64."""
    local64, target64 = copy.deepcopy(c.local).double(), copy.deepcopy(c.target).double()
    _, am = targets(local64, target64, c.exp, c.tt, c.ts, c.gamma_n, "mean")
    _, ad = targets(local64, target64, c.exp, c.tt, c.ts, c.gamma_n, "double")
    a_star = am if c.rule == "mean" else ad
    with torch.no_grad():
        zn = H._quantiles(target64, c.exp[3], c.tt)
    chosen = zn.gather(2, a_star.view(-1, 1, 1).expand(-1, zn.shape[1], 1)).squeeze(2)
    _, on_s = targets(local64, target64, c.exp, c.tt, c.ts, c.gamma_n, c.rule, defect="selector_on_s")
    return float((am != ad).double().mean()), float((chosen != zn.max(dim=2)[0]).any(dim=1).double().mean()), float((on_s != a_star).double().mean())
