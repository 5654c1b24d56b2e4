"""A float64 statement of ONE gradient step of the DQN baseline (sb3 DQN.train, dqn/dqn.py:188-230: target max, smooth-L1, clip_grad_norm_(10), torch.optim.Adam),
the inputs of the cases tests/test_dqn_train_f64_{cpu,gpu}.py run, and the bars a float32 step is held to against it (iqn_train_f64.compare_step, shared with the
IQN step).  Plain helper module, no fixtures.

    y[b]  = r[b] + (1 - done[b]) * gamma * max_a Q_target(next[b])[a]
    d[b]  = Q_local(s[b])[a_b] - y[b]
    loss  = mean_b( 0.5 d^2 if |d| < 1 else |d| - 0.5 )
    norm  = ||grad||_2 ; coef = min(1, 10 / (norm + 1e-6)) ; g = coef * grad
    m' = 0.9 m + 0.1 g ; v' = 0.999 v + 0.001 g^2 ; t' = t + 1
    p' = p - lr / (1 - 0.9^t') * m' / (sqrt(v') / sqrt(1 - 0.999^t') + 1e-8)

The networks are deep copies cast to double; nothing goes through F.smooth_l1_loss, clip_grad_norm_ or torch.optim.  All inputs are built with CPU generators, so
the CPU file (which asserts the condition a case relies on: norm side of 10, Huber branch share, distance from |d| = 1) and the GPU file (which moves them to the
device) see the same numbers.

Kinks.  The smooth-L1 gradient is continuous at |d| = 1, so a float32 evaluation on the other side of it differs by rounding only; the cases that CLAIM a branch
(all_linear, all_quadratic) keep every |d| at least KINK * max(1, max |y|) away from 1 all the same (`clear_of_the_kink` constructs it where a random batch does
not deliver it).  The ReLUs are kinks that cannot be excluded; they are the reason the bar is eager's own error and not a number."""
import copy
import math
import os
import sys
from types import SimpleNamespace

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(__file__))
from iqn_train_f64 import MAX_FACTOR, RMS_FACTOR, FLOOR, _untouched, compare_step as _compare_step, flat      # noqa: F401  (the bars are the IQN step's)

GAMMA, LR, MAX_NORM, B1, B2, EPS = 0.99, 1e-4, 10.0, 0.9, 0.999, 1e-8
KINK = 1e-3
NET_SEED = 3
TILE = 16
GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
DEFECTS = ("always_clip", "mse_everywhere", "t_stuck", "done_ignored", "target_is_local", "mean_over_tiles", "eps_inside_sqrt")


def _td(local64, target64, exp, gamma, defect=None):
    """d[b] = Q_local(s_b)[a_b] - y[b] and y, float64."""
    states, actions, rewards, next_states, dones = exp
    B = states.shape[0]
    with torch.no_grad():
        q_next = (local64 if defect == "target_is_local" else target64)(next_states.double()).max(dim=1)[0].view(B, 1)
        live = torch.ones(B, 1, dtype=torch.float64, device=states.device) if defect == "done_ignored" else 1.0 - dones.double().view(B, 1)
        y = rewards.double().view(B, 1) + live * gamma * q_next
    q = local64(states.double()).gather(1, actions.view(B, 1).long())
    return q - y, y


def dqn_f64_step(local, target, exp, gamma=GAMMA, m=None, v=None, t=0, lr=LR, max_norm=MAX_NORM, defect=None):
    """One step in float64 from `local` / `target` (a DQNPolicy.q_net, any device, not modified).  Returns a namespace: loss, norm (before the clip), grad (clipped,
    flat, dqn/fused_train.py::PARAM_NAMES order), params, m, v (flat, after the step), t (after), p0 (flat, before) and facts about the INPUT: lin_share (share of
    rows with |d| >= 1), min_kink (= min ||d| - 1|), max_abs_y, n_done, max_abs_act (the largest |output| of any linear layer of either forward).
    `defect`: None, or one deliberate mistake of DEFECTS, with which the CPU file shows that the bars reject a wrong step (tests of the tests)."""
    assert defect is None or defect in DEFECTS, defect
    local64, target64 = copy.deepcopy(local).double(), copy.deepcopy(target).double()
    params = list(local64.parameters())
    d, y = _td(local64, target64, exp, gamma, defect)
    B = d.shape[0]
    a = d.abs()
    terms = 0.5 * d * d if defect == "mse_everywhere" else torch.where(a < 1.0, 0.5 * d * d, a - 0.5)
    loss = terms.sum() / (TILE * ((B + TILE - 1) // TILE) if defect == "mean_over_tiles" else B)
    grads = torch.autograd.grad(loss, params)
    g = torch.cat([x.reshape(-1) for x in grads])
    norm = float(torch.linalg.vector_norm(g))
    coef = max_norm / (norm + 1e-6)
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
    bc1, bc2 = 1 - B1 ** tb, 1 - B2 ** tb
    denom = (v1 / bc2 + EPS).sqrt() if defect == "eps_inside_sqrt" else v1.sqrt() / math.sqrt(bc2) + EPS
    p1 = p0 - lr / bc1 * m1 / denom
    dd = d.detach()
    n = lambda x: x.cpu().numpy()
    return SimpleNamespace(loss=float(loss.detach()), norm=norm, grad=n(g), params=n(p1), m=n(m1), v=n(v1), t=t1, p0=n(p0),
                           lin_share=float((dd.abs() >= 1.0).double().mean()), min_kink=float((dd.abs() - 1.0).abs().min()),
                           max_abs_y=float(y.abs().max()), n_done=int((exp[4] != 0).sum()),
                           max_abs_act=max(_max_abs_act(local64, exp[0]), _max_abs_act(target64, exp[3])))


def _max_abs_act(net64, obs):
    """The largest |output| of any linear layer of the network on these observations: the scale float32 rounds the forward at."""
    top = [0.0]
    hooks = [mod.register_forward_hook(lambda _m, _i, out: top.__setitem__(0, max(top[0], float(out.detach().abs().max()))))
             for mod in net64.modules() if isinstance(mod, torch.nn.Linear)]
    try:
        with torch.no_grad():
            net64(obs.double())
    finally:
        for h in hooks:
            h.remove()
    return top[0]


def kink_window(r):
    return KINK * max(1.0, r.max_abs_y)


# ---- inputs (CPU generators) ------------------------------------------------------------------------------------------------------------------------
def make_nets(kind, gen, factor=1.0):
    """(local, target), float32 `_QNet`s on the CPU.  "seeded": DQNAgent(seed=3)'s network, target = local + 0.05 randn; "pretrained": the golden q_net.npz,
    target = local + 0.01 randn; "steep": the seeded pair with the LOCAL q_net.4.weight multiplied by `factor` (the gradient norm grows with it)."""
    from distributional_rl_navigation_amd.dqn import DQNAgent
    ag = DQNAgent(device="cpu", seed=NET_SEED, buffer_size=4, batch_size=1)
    if kind == "pretrained":
        ag.load(os.path.join(GOLDEN, "pretrained_DQN_seed3", "q_net.npz"))
    else:
        assert kind in ("seeded", "steep"), kind
    local = ag.q_net
    target = copy.deepcopy(local)
    with torch.no_grad():
        for p in target.parameters():
            p.add_((0.01 if kind == "pretrained" else 0.05) * torch.randn(p.shape, generator=gen))
        if kind == "steep":
            local.q_net[4].weight.mul_(float(factor))
    return local, target


def random_batch(B, g):
    """tests/iqn_train_f64.py::random_batch: observations randn * 5 with half of the sonar columns exactly zero, actions uniform in 0..8, rewards randn * 3,
    next = obs + 0.3 randn, dones 1 with probability 0.1."""
    obs = torch.randn(B, 26, generator=g) * 5
    obs[:, 4:] = torch.where(torch.rand(B, 22, generator=g) < 0.5, torch.zeros(()), obs[:, 4:])
    return [obs, torch.randint(0, 9, (B, 1), generator=g), torch.randn(B, 1, generator=g) * 3,
            obs + 0.3 * torch.randn(B, 26, generator=g), (torch.rand(B, 1, generator=g) < 0.1).float()]


def small_td_rewards(local, target, exp, gamma, delta, g):
    """r[b] = Q_local(s_b)[a_b] - gamma (1 - done_b) max_a Q_target(next_b) - delta * randn (float64 forward): d = delta * randn."""
    exp0 = list(exp)
    exp0[2] = torch.zeros_like(exp[2])
    d, _ = _td(copy.deepcopy(local).double(), copy.deepcopy(target).double(), exp0, gamma)
    noise = torch.randn(exp[0].shape[0], 1, generator=g).double()
    return (d.detach() - delta * noise).float()


def clear_of_the_kink(local, target, exp, gamma, td_floor=0.0):
    """Rewards with every row's |d| at least 2 windows above 1: a row nearer to |d| = 1 than that, or below it, gets the reward that puts its |d| at 1 + 4 windows
    (a case that claims the LINEAR branch for every row).  `td_floor`: and no |d| below this -- a row below it keeps its sign and gets |d| = td_floor.  Returns
    the float32 rewards."""
    d, y = _td(copy.deepcopy(local).double(), copy.deepcopy(target).double(), exp, gamma)
    d = d.detach()
    w = KINK * max(1.0, float(y.abs().max()), td_floor) * 1.03      # (the shifts may raise max |y| a little)
    sign = torch.where(d < 0, -torch.ones_like(d), torch.ones_like(d))
    low = max(1.0 + 4 * w, float(td_floor))
    want = torch.where(d.abs() < max(1.0 + 2 * w, float(td_floor)), sign * low, d)
    return (exp[2].double() + (d - want)).float()      # d = Q - r - ...: lowering r by x raises d by x


def build_case(kind="seeded", B=32, seed=None, reward_scale=1.0, action=None, dones=None, zero_sonar=None, small_td=None, steep=None, last_tile=False, td_floor=0.0):
    """One input: networks and batch.  kind: make_nets' ("steep" is chosen by `steep` = the factor).  reward_scale multiplies the rewards (above 1: and the rows
    are then put clear of |d| = 1 on the linear side, and at |d| >= td_floor); action: every row takes this action, or "all" = every action at least once; dones: 0 / 1 for every row;
    zero_sonar: "states" / "next_states" with columns 4..25 zero; small_td = delta: rewards from a float64 forward so that d = delta * randn; last_tile: case f,
    the rows of the last (partial) tile terminal with action 8, all others not terminal with actions 0..7."""
    g = torch.Generator().manual_seed(1000 + B if seed is None else seed)
    local, target = make_nets("steep" if steep is not None else kind, g, 1.0 if steep is None else steep)
    exp = random_batch(B, g)
    if action == "all":
        exp[1] = (torch.arange(B) % 9)[torch.randperm(B, generator=g)].view(B, 1)
    elif action is not None:
        exp[1] = torch.full((B, 1), int(action), dtype=torch.int64)
    if dones is not None:
        exp[4] = torch.full((B, 1), float(dones))
    if last_tile:
        n0 = (B - 1) // TILE * TILE
        exp[1] = torch.cat([torch.arange(n0) % 8, torch.full((B - n0,), 8)]).view(B, 1)
        exp[4] = torch.cat([torch.zeros(n0), torch.ones(B - n0)]).view(B, 1)
    if zero_sonar == "states":
        exp[0][:, 4:] = 0.0
    elif zero_sonar == "next_states":
        exp[3][:, 4:] = 0.0
    if small_td is not None:
        exp[2] = small_td_rewards(local, target, exp, GAMMA, small_td, g)
    exp[2] = exp[2] * reward_scale
    if reward_scale > 1.0:
        exp[2] = clear_of_the_kink(local, target, exp, GAMMA, td_floor)
    return SimpleNamespace(local=local, target=target, exp=tuple(exp), B=B)


def case_f64(c, **kw):
    return dqn_f64_step(c.local, c.target, c.exp, GAMMA, **kw)


# ---- the cases ------------------------------------------------------------------------------------------------------------------------------------
SWEEP = (1, 2, 15, 16, 17, 31, 32, 33, 100, 255, 256)
# factor of "steep" for which the float64 norm lands in 8.0-9.6 / 10.4-12.0 (bisection on dqn_f64_step, on the CPU)
THRESHOLD_STEEP = {2: (16.3, 17.9), 32: (50.6, 62.1), 256: (72.2, 83.7)}
HISTORY_STEPS, HISTORY_B, LATE_T = 12, 64, 99_999

# name -> (build_case keywords, conditions): clipped True / False = norm above 12 / below 8; norm = (lo, hi); lin_share = exact share of rows on the linear branch
# (and then every |d| a kink window from 1); actions = number of distinct actions
CASES = {}
# a. The seeded network never clips on these batches, the pretrained one always does (norms in the hundreds).  On these out-of-distribution observations the
# pretrained network's activations reach 2e3 and its Q values the hundreds: float32 resolves 3e-5 of such a Q, and d = Q - y carries a few of those steps as
# absolute error in ANY float32 step.  With random rewards that breaks both yardsticks.  On a quadratic row (|d| < 1) the gradient is proportional to d: two correct
# float32 steps differ from float64 by whichever neighbouring float their Q landed on (measured at B = 15: the fused step and eager on the CPU are both 8.27e-5 off
# in the gradient, eager on the GPU 1.3e-5).  And the loss, a few units, is the difference of numbers a hundred times larger: its floor of 1e-6 |loss| is below one
# float32 step of Q, and at B = 1, 2 no mean averages the rows' errors (measured: fused 5.5e-5 and 1.7e-4 off, eager 6e-6 and 1.8e-5; over the whole table the
# fused / eager ratio of the loss has median 1.00).  So the pretrained rows are put on the linear branch, dL/dQ = +-1 / B exactly, at |d| >= PRETRAINED_TD, which
# makes the loss of the size of the largest activation: its floor is then worth at least 4 float32 steps of that (`loss_floor`, asserted on the CPU).  Quadratic
# rows under a clipped step: threshold_hi_*, where Q is of order 10.
PRETRAINED_TD = 1024.0
for _B in SWEEP:
    CASES[f"sweep_B{_B}"] = (dict(B=_B), dict(clipped=False))
    CASES[f"sweep_pretrained_B{_B}"] = (dict(kind="pretrained", B=_B, reward_scale=30.0, td_floor=PRETRAINED_TD), dict(clipped=True, lin_share=1.0, loss_floor=True))
for _B, (_lo, _hi) in THRESHOLD_STEEP.items():      # b.
    CASES[f"threshold_lo_B{_B}"] = (dict(B=_B, steep=_lo), dict(norm=(8.0, 9.6)))
    CASES[f"threshold_hi_B{_B}"] = (dict(B=_B, steep=_hi), dict(norm=(10.4, 12.0)))
for _B in (17, 32, 100, 256):      # c. (17 and 100: the learner-group launches run three different cases of one batch size)
    CASES[f"all_done_B{_B}"] = (dict(B=_B, dones=1), dict())
    CASES[f"all_linear_B{_B}"] = (dict(B=_B, reward_scale=30.0), dict(lin_share=1.0))
for _B in (32, 256):
    CASES[f"none_done_B{_B}"] = (dict(B=_B, dones=0), dict())
    CASES[f"all_quadratic_B{_B}"] = (dict(B=_B, small_td=0.05), dict(lin_share=0.0, clipped=False))
    CASES[f"one_action0_B{_B}"] = (dict(B=_B, action=0), dict(actions=1))
    CASES[f"one_action8_B{_B}"] = (dict(B=_B, action=8), dict(actions=1))
    CASES[f"no_sonar_states_B{_B}"] = (dict(B=_B, zero_sonar="states"), dict())
    CASES[f"no_sonar_next_B{_B}"] = (dict(B=_B, zero_sonar="next_states"), dict())
CASES["every_action_B32"] = (dict(B=32, action="all"), dict(actions=9))
# (d., e. the batches of the 12-step history and of the late step: history_batch, conditions asserted at the states an eager run meets)
CASES["last_tile_B17"] = (dict(B=17, last_tile=True), dict(clipped=False))      # f.
EDGES = tuple(n for n in CASES if not n.startswith(("sweep_", "threshold_", "last_tile")))


def case(name):
    return build_case(**CASES[name][0])


def history_batch(k):
    """Networks (k = 1: the history starts from them) and batch of step k = 1..HISTORY_STEPS of the Adam history (case d); k = HISTORY_STEPS + 1: the late step (e)."""
    return build_case(B=HISTORY_B, seed=500 + k)


def assert_margin(name, r, max_norm=MAX_NORM):
    """No case sits where float32 and float64 could disagree about the clip: the norm is outside 0.8 .. 1.2 max_norm unless the case names its own range."""
    assert r.norm < 0.8 * max_norm or r.norm > 1.2 * max_norm, (name, r.norm)


def assert_conditions(name, c, r):
    """What the GPU case `name` relies on, from the float64 result `r` of its input `c` alone."""
    kw, cond = CASES[name]
    if "norm" in cond:
        assert cond["norm"][0] <= r.norm <= cond["norm"][1], (name, r.norm)
    else:
        assert_margin(name, r)
    if cond.get("clipped") is True:
        assert r.norm > 12.0, (name, r.norm)
    if cond.get("clipped") is False:
        assert r.norm < 8.0, (name, r.norm)
    if "lin_share" in cond:
        assert r.lin_share == cond["lin_share"] and r.min_kink >= kink_window(r), (name, r.lin_share, r.min_kink, kink_window(r))
    if cond.get("loss_floor"):      # 1e-6 |loss| is at least 4 float32 steps (2^-24 relative, rounding to nearest) of the largest number either forward handles
        assert FLOOR * r.loss >= 4 * 2.0 ** -24 * r.max_abs_act, (name, r.loss, r.max_abs_act)
    if "actions" in cond:
        assert c.exp[1].unique().numel() == cond["actions"] and int(c.exp[1].min()) >= 0 and int(c.exp[1].max()) <= 8
    if kw.get("action") not in (None, "all"):
        assert bool((c.exp[1] == kw["action"]).all())
    if kw.get("dones") is not None:
        assert bool((c.exp[4] == float(kw["dones"])).all()) and r.n_done == (c.B if kw["dones"] else 0)
    if kw.get("zero_sonar"):
        x = c.exp[0] if kw["zero_sonar"] == "states" else c.exp[3]
        assert bool((x[:, 4:] == 0).all()) and float(x[:, :4].abs().min()) > 0
    if kw.get("last_tile"):
        n0 = (c.B - 1) // TILE * TILE
        a, d = c.exp[1].view(-1), c.exp[4].view(-1)
        assert 0 < c.B - n0 < TILE and bool((a[n0:] == 8).all()) and bool((d[n0:] == 1).all()) and int(a[:n0].max()) == 7 and not bool(d[:n0].any())
        assert r.n_done == c.B - n0


# flat layout (dqn/fused_train.py::PARAM_NAMES, the offsets of csrc/dqn_train.hip): velocity 32 + 16, goal 32 + 16, sensor 176 x 22 + 176, ..., q_net.4 9 x 64 + 9 at the end
P_TOTAL = 27650
O_SW, O_SB, O_Q4W, O_Q4B = 96, 3968, 27065, 27641
SENSOR_W = slice(O_SW, O_SB)


def output_rows(action):
    """Flat positions of q_net.4.weight[action] (start, stop) and of q_net.4.bias[action]."""
    return (O_Q4W + 64 * action, O_Q4W + 64 * action + 64), O_Q4B + action


def assert_untaken_actions_untouched(res, p0, taken):
    """Every row took action `taken`: gradient and moments (from zero moments) of the other eight q_net.4 rows exactly 0.0, their parameters bit for bit where they were."""
    for a in range(9):
        if a != taken:
            (lo, hi), b = output_rows(a)
            _untouched(res, p0, slice(lo, hi), f"q_net.4.weight[{a}]")
            _untouched(res, p0, slice(b, b + 1), f"q_net.4.bias[{a}]")
    (lo, hi), b = output_rows(taken)
    assert np.abs(np.asarray(res.grad)[lo:hi]).max() > 0 and np.asarray(res.grad)[b] != 0


def assert_sensor_weight_untouched(res, p0):
    """No sonar return in any state: sensor_encoder.weight has an exactly zero gradient and Adam (0 / (0 + eps) from zero moments) leaves it alone."""
    _untouched(res, p0, SENSOR_W, "sensor_encoder.weight")
    assert np.abs(np.asarray(res.grad)[O_SB:O_SB + 176]).max() > 0      # its bias still learns


# ---- the bars ------------------------------------------------------------------------------------------------------------------------------------
def compare_step(ref, fused, eager, label="", rows=None):
    """iqn_train_f64.compare_step with the DQN step's clip norm and learning rate."""
    return _compare_step(ref, fused, eager, label, rows, max_norm=MAX_NORM, lr=LR)
