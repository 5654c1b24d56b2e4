"""Hand-built inputs for the two discrete decisions every learned policy ends in (tests/test_decision_edges_cpu.py, tests/test_decision_edges_gpu.py):
which action is greedy -- argmax, the first maximum wins, like np.argmax -- and which CVaR level an adaptive row acts with (`adjust_cvar_row`,
csrc/mn_rollout_iqn_body.h, the device restatement of `IQNAgent.adjust_cvar_batch`).

A. `bias_table()`: bias vectors for an output layer whose WEIGHT is zero.  Every IQN form then computes 0 * scale + b4[a] (act_eval's form: the mean of
   32 copies of b4[a]), the DQN network q_net[4].bias: Q is the bias whatever the observation and the taus, so ties are exact and the expected action is
   np.argmax(bias), computed, never written down.  Every magnitude is a float32 with few significant bits and at most 2^100, so 32 copies sum exactly.
   `expected_q(bias)` is float32(0) + bias: the bias bit for bit except that a bias of -0.0 comes out as +0.0, because the zero product the bias is
   added to is +0.0 and (+0) + (-0) = +0 in IEEE 754 -- in eager PyTorch as in the kernels.
   OUT OF SCOPE, nothing here asserts on them: denormal, infinite and NaN biases.  A non-finite bias also enters the range bounds of the split kernel;
   the kernels' `v > best` chains and torch.argmax differ on NaN by design of their comparisons; and a network with a NaN weight has all Q NaN, where
   every kernel returns action 0.
B. `duplicate_output_row` / `tie_lift`: a tie through the real arithmetic.  Output row a is copied over row b and both biases are lifted by the smallest
   power of two that puts column a clear of every other column in a float64 evaluation; the two columns run one instruction sequence on one set of
   inputs and must come out bit-equal.
C. `cvar_twin(rows)`: a numpy float32 restatement of the comment above `adjust_cvar_row` (not of the torch code), and `cvar_edge_rows()`: observation
   rows that sit on its three thresholds (|x| < 1e-3 and |y| < 1e-3: skip; closest < 10; no return: 1.0).  `cvar_decisions_f32 / _f64` are the
   skip and below-10 decisions of the twin's arithmetic and of the reference's rule in float64 on the same float32 values; a row on which float32
   rounding of the norm moves a decision does not belong in the table (test_decision_edges_cpu.py checks that none does).
"""
import os

import numpy as np

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
N_ROWS = 70                       # more than one wavefront's / tile's worth of rows, and a ragged last tile
N_ACTIONS, N_BEAMS, N_TAUS = 9, 11, 32
PAIRS = ((0, 8), (3, 4), (7, 8))  # part B: first and last action; across lane groups 0/1 and 1/2 of dqn_argmax
F = np.float32


# ---- A: the bias table -------------------------------------------------------------------------------------------------------------------------------
def bias_table():
    """[(name, float32 [9])]; the expected action of each is `int(np.argmax(bias))`."""
    def const(v):
        return np.full(N_ACTIONS, v, dtype=F)

    def maxima(at, hi=2.0, lo=-1.0):
        b = const(lo)
        b[list(at)] = hi
        return b
    t = [("all 0", const(0.0)), ("all 3.5", const(3.5)), ("all -7", const(-7.0))]
    t += [(f"single maximum at {k}", maxima((k,))) for k in range(N_ACTIONS)]
    t += [("ascending 1..9", np.arange(1, 10, dtype=F)), ("descending 9..1", np.arange(9, 0, -1, dtype=F)), ("ascending -9..-1", np.arange(-9, 0, dtype=F))]
    t += [(f"equal maxima at {at}", maxima(at)) for at in ((0, 8), (3, 4), (7, 8), (4, 8), (1, 2), (2, 5, 8))]
    z = const(0.0)
    z[0::2] = -0.0
    t.append(("signed zeros -0 +0 -0 ...", z))
    z = const(-1.0)
    z[1::3], z[2::3] = -0.0, 0.0
    t.append(("-1 -0 +0 -1 ...", z))
    b = const(1.0)
    b[5] = np.nextafter(F(1), F(2))
    t.append(("1 everywhere, nextafter(1, 2) at 5", b))
    b = const(1.0)
    b[0] = np.nextafter(F(1), F(0))
    t.append(("1 everywhere, nextafter(1, 0) at 0", b))
    t.append(("-2^100 everywhere, +2^100 at 6 and 8", maxima((6, 8), hi=2.0 ** 100, lo=-2.0 ** 100)))
    for name, b in t:
        assert b.dtype == F and b.shape == (N_ACTIONS,) and np.isfinite(b).all() and np.abs(b).max() <= 2.0 ** 100, name
        assert ((b == 0) | (np.abs(b) >= np.finfo(F).tiny)).all(), name      # no denormals
    return t


def expected_action(bias):
    return int(np.argmax(bias))


def expected_q(bias):
    """What a zero output weight leaves of `bias`: (+0) + bias in float32 -- the bias itself, a -0.0 as +0.0."""
    return np.zeros(N_ACTIONS, dtype=F) + np.asarray(bias, dtype=F)


def bits(x):
    """float32 array -> its int32 bit patterns."""
    x = np.ascontiguousarray(x)
    assert x.dtype == F
    return x.view(np.int32)


def random_obs(n, seed=11, scale=5.0):
    """[n, 26] float32 observations in the style of tests/test_act_split_gpu.py::_inputs: normal x scale, 40 % of the sonar entries exact zeros (misses)."""
    r = np.random.RandomState(seed)
    obs = (r.standard_normal((n, 26)) * scale).astype(F)
    miss = r.random_sample((n, 22)) < 0.4
    obs[:, 4:][miss] = 0.0
    return obs


def random_taus(shape, seed=12):
    return np.random.RandomState(seed).random_sample(shape).astype(F)


def set_output(layer, weight, bias):
    """Overwrite an nn.Linear output layer (through PyTorch: the act contexts see the version counters move).  weight None: zero."""
    import torch
    with torch.no_grad():
        if weight is None:
            layer.weight.zero_()
        else:
            layer.weight.copy_(torch.as_tensor(weight).to(layer.weight))
        layer.bias.copy_(torch.as_tensor(np.asarray(bias, dtype=F)).to(layer.bias))


# ---- B: ties through the real arithmetic ---------------------------------------------------------------------------------------------------------------
def clear_of_the_others(q64, a, b):
    """Part B's condition on a float64 [rows, 9] evaluation: columns a and b equal, and column a above every other column by at least
    1e-3 max|Q64| on every row."""
    q64 = np.asarray(q64, dtype=np.float64)
    others = np.delete(q64, [a, b], axis=1).max(axis=1)
    return bool(np.array_equal(q64[:, a], q64[:, b]) and ((q64[:, a] - others) >= 1e-3 * np.abs(q64).max()).all())


def tie_lift(layer, weight, bias, a, b, q64_of):
    """Copies output row `a` of (`weight`, `bias`: the layer's original float32 arrays) over row `b` in `layer`, then lifts both biases by the smallest
    power of two 2^k, k >= -30, for which `q64_of()` -- a float64 evaluation of the network as it then stands, [rows, 9] -- satisfies
    `clear_of_the_others`.  A small lift keeps the low bits of Q alive.  Returns (lift, that float64 evaluation)."""
    w = np.array(weight, dtype=F)
    w[b] = w[a]
    for k in range(-30, 41):
        lift = F(2.0 ** k)
        bb = np.array(bias, dtype=F)
        bb[a] = bb[b] = F(bb[a] + lift)
        set_output(layer, w, bb)
        q64 = q64_of()
        if clear_of_the_others(q64, a, b):
            return float(lift), q64
    raise AssertionError("no lift up to 2^40 separates the duplicated rows from the others")


# ---- C: adjust_cvar on its thresholds ----------------------------------------------------------------------------------------------------------------
P = F(1e-3)
P_LO, P_HI = np.nextafter(P, F(0)), np.nextafter(P, F(1))      # the float32 neighbours of float32(1e-3)
TEN = F(10.0)


def cvar_twin(rows):
    """adjust_cvar_row for float32 rows [m, 26], operation by operation in float32: per beam b in 0..10 px = row[4 + 2 b], py = row[5 + 2 b]; the two
    squares rounded separately, their sum rounded, a correctly rounded square root; the point is skipped iff |px| < 1e-3f and |py| < 1e-3f; closest =
    the minimum; closest < 10 ? closest * 0.1f : 1."""
    rows = np.asarray(rows)
    assert rows.dtype == F and rows.ndim == 2 and rows.shape[1] == 26
    px, py = rows[:, 4::2], rows[:, 5::2]
    assert px.shape[1] == N_BEAMS and py.shape[1] == N_BEAMS
    xx, yy = px * px, py * py
    d = np.sqrt(xx + yy)
    assert xx.dtype == F and d.dtype == F
    skip = (np.abs(px) < P) & (np.abs(py) < P)
    closest = np.where(skip, F(np.inf), d).min(axis=1)
    with np.errstate(invalid="ignore"):
        out = np.where(closest < TEN, closest * F(0.1), F(1.0))
    assert out.dtype == F
    return out


def cvar_decisions_f32(rows):
    """(skip [m, 11], below 10 [m]) as the twin's float32 arithmetic decides them."""
    rows = np.asarray(rows)
    assert rows.dtype == F
    px, py = rows[:, 4::2], rows[:, 5::2]
    skip = (np.abs(px) < P) & (np.abs(py) < P)
    closest = np.where(skip, F(np.inf), np.sqrt(px * px + py * py)).min(axis=1)
    return skip, closest < TEN


def cvar_decisions_f64(rows):
    """The same decisions by the reference's rule (abs(x) < 1e-3 and abs(y) < 1e-3; norm < 10.0) in float64 on the same float32 values."""
    rows = np.asarray(rows)
    assert rows.dtype == F
    px, py = rows[:, 4::2].astype(np.float64), rows[:, 5::2].astype(np.float64)
    skip = (np.abs(px) < 1e-3) & (np.abs(py) < 1e-3)
    closest = np.where(skip, np.inf, np.hypot(px, py)).min(axis=1)
    return skip, closest < 10.0


def _row(points=(), head=(0.5, -0.25, 3.0, -4.0)):
    """One observation row: `head` in row[0:4], sonar point (x, y) in beam b for every (b, x, y) of `points`, exact zeros (no return) elsewhere."""
    r = np.zeros(26, dtype=F)
    r[:4] = head
    for b, x, y in points:
        assert 0 <= b < N_BEAMS
        r[4 + 2 * b], r[5 + 2 * b] = x, y
    return r


def hand_rows():
    """[(name, row)]: the hand-made threshold rows."""
    below10, above10 = np.nextafter(TEN, F(0)), np.nextafter(TEN, F(20))
    far = [(b, 8.0, 0.0) for b in range(N_BEAMS)]
    t = [
        ("no return in any beam", _row()),
        ("one return, beam 0 only", _row([(0, 3.0, 4.0)])),
        ("one return, beam 10 only", _row([(10, 3.0, 4.0)])),
        ("(10, 0): exactly 10", _row([(4, 10.0, 0.0)])),
        ("(6, 8): exactly 10", _row([(4, 6.0, 8.0)])),
        ("(0, -10): exactly 10", _row([(4, 0.0, -10.0)])),
        ("(-6, -8): exactly 10", _row([(9, -6.0, -8.0)])),
        ("(nextafter(10, 0), 0): just below 10", _row([(4, below10, 0.0)])),
        ("(nextafter(10, 20), 0): just above 10", _row([(4, above10, 0.0)])),
        ("(60, 80): far", _row([(2, 60.0, 80.0)])),
        ("(p-, p-) alone: skipped", _row([(6, P_LO, P_LO)])),
        ("(p-, p-) beside a return at 5", _row([(3, P_LO, P_LO), (7, 3.0, 4.0)])),
        ("(p-, p-) in beam 10 beside a return at 5 in beam 0", _row([(10, P_LO, P_LO), (0, 3.0, 4.0)])),
        ("(p, 0): not skipped", _row([(1, P, 0.0)])),
        ("(0, p): not skipped", _row([(1, 0.0, P)])),
        ("(p-, p): not skipped", _row([(5, P_LO, P)])),
        ("(p, p-): not skipped", _row([(5, P, P_LO)])),
        ("(p, p): not skipped", _row([(5, P, P)])),
        ("(-p+, 0): not skipped", _row([(8, -P_HI, 0.0)])),
        ("(p-, 0) alone: skipped", _row([(8, P_LO, 0.0)])),
        ("(0, -p-) alone: skipped", _row([(8, 0.0, -P_LO)])),
        ("(-p-, p-) alone: skipped", _row([(2, -P_LO, P_LO)])),
        ("(-p-, p-) beside a return at 5", _row([(2, -P_LO, P_LO), (3, -5.0, 0.0)])),
        ("(-0.0, 0.0) alone: skipped", _row([(0, -0.0, 0.0)])),
        ("two beams at equal distance 5", _row([(2, 3.0, 4.0), (8, 4.0, 3.0)])),
        ("every beam at distance 5", _row([(b, 0.0, -5.0) for b in range(N_BEAMS)])),
        ("closest return at 9.999", _row([(4, 9.999, 0.0), (5, 12.0, 0.0)])),
        ("closest return at 3", _row([(4, 0.0, 3.0), (9, 7.0, 0.0)])),
        ("closest return at 0.5", _row([(6, -0.5, 0.0), (1, 2.0, 2.0)])),
        ("closest return at 0.0015", _row([(10, 0.0015, 0.0), (0, 1.0, 1.0)])),
        ("row[0:4] = 1e-4, no return", _row(head=(1e-4,) * 4)),
        ("row[0:4] = 1e-4, a return at exactly 10", _row([(4, 6.0, 8.0)], head=(1e-4,) * 4)),
        ("row[0:4] = 50, a return at 5", _row([(4, 3.0, 4.0)], head=(50.0,) * 4)),
        ("beam 10 closest (2), beams 0..9 at 8", _row(far[:10] + [(10, 0.0, 2.0)])),
        ("beam 0 closest (2), beams 1..10 at 8", _row([(0, 2.0, 0.0)] + far[1:])),
        ("every beam at 10 or beyond", _row([(b, 10.0 + b, 0.0) for b in range(N_BEAMS)])),
        ("exactly 10 beside 12", _row([(3, 0.0, 10.0), (4, 12.0, 0.0)])),
        ("exactly 10 beside just below 10", _row([(3, 0.0, 10.0), (4, 0.0, below10)])),
    ]
    return t


def cvar_edge_rows():
    """([70, 26] float32, names): the hand-made rows followed by the `cvar_states` rows of tests/golden/g7_iqn.npz cast to float32 (the rows the
    reference's own adjust_cvar was recorded on), tiled to N_ROWS."""
    hand = hand_rows()
    g7 = np.load(os.path.join(GOLD, "g7_iqn.npz"))["cvar_states"].astype(F)
    rows = np.concatenate([np.stack([r for _, r in hand]), g7])
    names = [n for n, _ in hand] + [f"g7 cvar_states[{i}]" for i in range(len(g7))]
    assert len(rows) <= N_ROWS, "more edge rows than the launches carry: raise N_ROWS"
    idx = np.arange(N_ROWS) % len(rows)
    return np.ascontiguousarray(rows[idx]), [names[i] for i in idx]
