"""The hand-built decision fixtures of tests/decision_edges.py on the CPU: the bias table is what it says it is, the CVaR twin decides as the reference's
rule does in float64 on every edge row, and the eager PyTorch paths (IQNAgent.act_batch / act_eval_batch / adjust_cvar_batch, DQNPolicy.q_values /
act_batch) make the same choices.  The kernels are held to the same fixtures in tests/test_decision_edges_gpu.py."""
import copy
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import decision_edges as E      # noqa: E402

F = np.float32


@pytest.fixture(scope="module")
def torch():
    import torch as t
    return t


# ---- A ---------------------------------------------------------------------------------------------------------------------------------------------
def test_bias_table_holds_the_patterns_it_names():
    table = E.bias_table()
    assert 20 <= len(table) <= 64 and len({n for n, _ in table}) == len(table)
    want = {"all 0": 0, "all 3.5": 0, "all -7": 0, "ascending 1..9": 8, "descending 9..1": 0, "ascending -9..-1": 8, "equal maxima at (0, 8)": 0,
            "equal maxima at (3, 4)": 3, "equal maxima at (7, 8)": 7, "equal maxima at (4, 8)": 4, "equal maxima at (1, 2)": 1,
            "equal maxima at (2, 5, 8)": 2, "signed zeros -0 +0 -0 ...": 0, "-1 -0 +0 -1 ...": 1, "1 everywhere, nextafter(1, 2) at 5": 5,
            "1 everywhere, nextafter(1, 0) at 0": 1, "-2^100 everywhere, +2^100 at 6 and 8": 6}
    want.update({f"single maximum at {k}": k for k in range(9)})
    got = {n: E.expected_action(b) for n, b in table}
    assert got == want
    ties = [n for n, b in table if (b == b.max()).sum() > 1]
    assert len(ties) >= 12      # most of the table is exact ties, which no other test holds
    zeros = dict(table)["signed zeros -0 +0 -0 ..."]
    assert np.signbit(zeros).tolist() == [True, False] * 4 + [True] and not zeros.any()
    # what a zero output weight leaves of a bias: the bias bit for bit, a -0.0 as +0.0; and 32 copies of it sum and average exactly
    for name, b in table:
        q = E.expected_q(b)
        same = E.bits(q) == E.bits(b)
        assert (same | ((b == 0) & np.signbit(b) & (E.bits(q) == 0))).all(), name
        s = q
        for _ in range(5):      # 32 copies, summed pairwise: every partial sum is a power of two times q
            s = s + s
        assert np.array_equal(E.bits(s * F(1 / 32)), E.bits(q)), name


def test_eager_iqn_paths_on_the_bias_table(torch):
    from distributional_rl_navigation_amd.iqn.agent import IQNAgent
    agent = IQNAgent(26, 9, device="cpu", seed=5)
    net = agent.qnetwork_local
    obs = torch.from_numpy(E.random_obs(E.N_ROWS))
    taus = torch.from_numpy(E.random_taus((E.N_ROWS, 32)))
    for name, b in E.bias_table():
        E.set_output(net.output_layer, None, b)
        a_want = E.expected_action(b)
        q = agent.qvals_batch(obs, 1.0, taus=taus).numpy()
        assert np.array_equal(E.bits(q), np.broadcast_to(E.bits(E.expected_q(b)), q.shape)), name
        assert (agent.act_batch(obs, 0.0).numpy() == a_want).all(), name
        acts, quant, t = agent.act_eval_batch(obs, 0.0, 1.0, taus=taus)
        assert np.array_equal(E.bits(quant.numpy()), np.broadcast_to(E.bits(E.expected_q(b)), quant.shape)), name
        assert (acts.numpy() == a_want).all(), name


def test_eager_dqn_paths_on_the_bias_table(torch):
    from distributional_rl_navigation_amd.dqn import DQNPolicy
    pol = DQNPolicy.load(os.path.join(E.GOLD, "pretrained_DQN_seed3", "q_net.npz"), device="cpu")
    for n in (E.N_ROWS, 37):
        obs = torch.from_numpy(E.random_obs(n, seed=3))
        for name, b in E.bias_table():
            E.set_output(pol.q_net.q_net[4], None, b)
            q = pol.q_values(obs).numpy()
            assert np.array_equal(E.bits(q), np.broadcast_to(E.bits(E.expected_q(b)), q.shape)), name
            assert (pol.act_batch(obs).numpy() == E.expected_action(b)).all(), name
            a, _ = pol.predict(obs.numpy(), deterministic=True)
            assert (a == E.expected_action(b)).all(), name


# ---- B ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("a,b", E.PAIRS)
def test_duplicated_output_rows_tie_in_eager_pytorch(torch, a, b):
    from distributional_rl_navigation_amd.iqn.model import ObsEncoder
    net = ObsEncoder(26, 9, seed=5, device="cpu")
    obs = torch.from_numpy(E.random_obs(E.N_ROWS))
    taus = torch.from_numpy(E.random_taus((E.N_ROWS, 32)))
    w0, b0 = net.output_layer.weight.detach().numpy().copy(), net.output_layer.bias.detach().numpy().copy()

    def q64_of():
        with torch.no_grad():
            return copy.deepcopy(net).double().get_qvals(obs.double(), 1.0, taus=taus.double()).numpy()
    lift, q64 = E.tie_lift(net.output_layer, w0, b0, a, b, q64_of)
    assert E.clear_of_the_others(q64, a, b) and (q64.argmax(axis=1) == a).all()
    assert lift <= 4.0 * np.abs(q64).max()      # a small power of two: the low bits of Q stay alive
    with torch.no_grad():
        q = net.get_qvals(obs, 1.0, taus=taus).numpy()
    assert np.array_equal(E.bits(q[:, a].copy()), E.bits(q[:, b].copy()))
    assert (q.argmax(axis=1) == a).all() and (torch.from_numpy(q).argmax(dim=1).numpy() == a).all()


# ---- C ---------------------------------------------------------------------------------------------------------------------------------------------
def test_edge_rows_cover_the_three_thresholds():
    rows, names = E.cvar_edge_rows()
    assert rows.shape == (E.N_ROWS, 26) and rows.dtype == F and len(names) == E.N_ROWS
    hand = E.hand_rows()
    assert 35 <= len(hand) <= 45 and len({n for n, _ in hand}) == len(hand)
    cv = dict(zip(names, E.cvar_twin(rows)))
    one = [n for n, v in cv.items() if v == 1.0]
    for n in ("no return in any beam", "(10, 0): exactly 10", "(6, 8): exactly 10", "(0, -10): exactly 10", "(-6, -8): exactly 10", "(p-, p-) alone: skipped",
              "(-p-, p-) alone: skipped", "(-0.0, 0.0) alone: skipped", "(p-, 0) alone: skipped", "(0, -p-) alone: skipped", "row[0:4] = 1e-4, no return",
              "row[0:4] = 1e-4, a return at exactly 10", "(nextafter(10, 20), 0): just above 10", "every beam at 10 or beyond", "exactly 10 beside 12"):
        assert n in one, n
    for n in ("(nextafter(10, 0), 0): just below 10", "exactly 10 beside just below 10"):
        assert cv[n] < 1.0 and cv[n] >= np.nextafter(F(1), F(0)) - F(2e-7), (n, cv[n])
    for n in ("one return, beam 0 only", "one return, beam 10 only", "(p-, p-) beside a return at 5", "(p-, p-) in beam 10 beside a return at 5 in beam 0",
              "(-p-, p-) beside a return at 5", "two beams at equal distance 5", "every beam at distance 5", "row[0:4] = 50, a return at 5"):
        assert cv[n] == F(0.5), (n, cv[n])
    for n in ("(p, 0): not skipped", "(0, p): not skipped", "(p-, p): not skipped", "(p, p-): not skipped", "(p, p): not skipped", "(-p+, 0): not skipped"):
        assert 0.9e-4 < cv[n] < 1.5e-4, (n, cv[n])
    assert cv["beam 10 closest (2), beams 0..9 at 8"] == cv["beam 0 closest (2), beams 1..10 at 8"] == F(2.0) * F(0.1)
    assert cv["closest return at 3"] == F(3.0) * F(0.1) and cv["closest return at 0.5"] == F(0.5) * F(0.1)
    assert abs(cv["closest return at 9.999"] - 0.9999) < 1e-6 and abs(cv["closest return at 0.0015"] - 1.5e-4) < 1e-9
    # the rows the reference's own adjust_cvar was recorded on: the twin reproduces its float64 results to float32 rounding
    z = np.load(os.path.join(E.GOLD, "g7_iqn.npz"))
    got = E.cvar_twin(z["cvar_states"].astype(F))
    assert np.abs(got - z["cvar_values"]).max() < 1e-6 and (got < 1.0).sum() >= 4 and (got == 1.0).sum() >= 4


def test_twin_decides_as_the_reference_rule_does_in_float64():
    rows, names = E.cvar_edge_rows()
    skip32, below32 = E.cvar_decisions_f32(rows)
    skip64, below64 = E.cvar_decisions_f64(rows)
    bad = [names[i] for i in range(len(rows)) if not (np.array_equal(skip32[i], skip64[i]) and below32[i] == below64[i])]
    assert not bad, bad      # a row on which float32 rounding of the norm moves a decision does not belong in the table
    assert skip32.any() and (~skip32).any() and below32.any() and (~below32).any()
    # float32(1e-3) lies above 1e-3: it is not skipped in either arithmetic, its lower neighbour is in both
    assert float(E.P) >= 1e-3 > float(E.P_LO)


def _cvar_variant(rows, skip_any=False, at_ten=False, beams=E.N_BEAMS, one_rounding=False, divide=False):
    """cvar_twin with one deliberate departure from the kernel comment's recipe."""
    px, py = rows[:, 4:4 + 2 * beams:2], rows[:, 5:5 + 2 * beams:2]
    d = np.hypot(px.astype(np.float64), py.astype(np.float64)).astype(F) if one_rounding else np.sqrt(px * px + py * py)
    small_x, small_y = np.abs(px) < E.P, np.abs(py) < E.P
    skip = (small_x | small_y) if skip_any else (small_x & small_y)
    closest = np.where(skip, F(np.inf), d).min(axis=1)
    below = closest <= E.TEN if at_ten else closest < E.TEN
    with np.errstate(invalid="ignore"):
        return np.where(below, closest / E.TEN if divide else closest * F(0.1), F(1.0))


@pytest.mark.parametrize("bug", [dict(skip_any=True), dict(beams=10), dict(one_rounding=True), dict(divide=True)],
                         ids=["|x| or |y| small skips", "beam loop stops at 10", "one rounding for the norm", "a division for * 0.1f"])
def test_edge_rows_tell_the_recipe_from_its_near_misses(bug):
    """The edge rows have the power the GPU tests rely on: a kernel with one of these departures would leave another cvar bit pattern on some row."""
    rows, names = E.cvar_edge_rows()
    assert np.array_equal(E.bits(_cvar_variant(rows)), E.bits(E.cvar_twin(rows)))
    moved = np.nonzero(E.bits(_cvar_variant(rows, **bug)) != E.bits(E.cvar_twin(rows)))[0]
    assert len(moved) >= 1, bug
    print(bug, "moves", sorted({names[i] for i in moved}))


def test_at_exactly_ten_both_branches_give_one():
    """`closest <= 10` for `closest < 10` is NOT a departure any row can show: float32(10 * 0.1f) is 1.0, the other branch's value.  The rows at exactly 10
    therefore pin the value 1.0, not the comparison."""
    assert F(10.0) * F(0.1) == F(1.0) and np.nextafter(E.TEN, F(0)) * F(0.1) < F(1.0)
    rows, _ = E.cvar_edge_rows()
    assert np.array_equal(E.bits(_cvar_variant(rows, at_ten=True)), E.bits(E.cvar_twin(rows)))


def _eager_cvar(torch):
    from distributional_rl_navigation_amd.iqn.agent import IQNAgent
    agent = IQNAgent(26, 9, device="cpu", seed=5)
    rows, names = E.cvar_edge_rows()
    got = agent.adjust_cvar_batch(torch.from_numpy(rows)).numpy()
    assert got.dtype == F and got.shape == (E.N_ROWS,)
    return rows, names, got, E.cvar_twin(rows)


def _ulps(x, y):
    return np.abs(E.bits(x).astype(np.int64) - E.bits(y).astype(np.int64))


def test_eager_adjust_cvar_batch_decides_as_the_twin(torch):
    """The same decisions on every edge row: 1.0 exactly where the twin says 1.0 (no return, skipped points, nothing closer than 10), below 1 elsewhere.
    On CPU tensors adjust_cvar_batch writes the device's norm out (torch's CPU `linalg.vector_norm` rounds x^2 + y^2 once and lands one ulp from it
    on some points), so up to the last step it IS the twin: the result is `closest < 10 ? closest / 10 : 1` of the twin's own closest norm bit for
    bit -- a true division, where the device multiplies by 0.1f."""
    rows, names, got, twin = _eager_cvar(torch)
    assert np.array_equal(got == 1.0, twin == 1.0), [names[i] for i in np.nonzero((got == 1.0) != (twin == 1.0))[0]]
    px, py = rows[:, 4::2], rows[:, 5::2]
    norm = np.sqrt(px * px + py * py)
    p = torch.from_numpy(rows)[:, 4:].view(len(rows), -1, 2)
    assert _ulps(torch.linalg.vector_norm(p, dim=2).numpy(), norm).max() == 1      # (why the norm is written out)
    skip, _ = E.cvar_decisions_f32(rows)
    closest = np.where(skip, F(np.inf), norm).min(axis=1)
    with np.errstate(invalid="ignore"):
        own = np.where(closest < E.TEN, closest / E.TEN, F(1.0))
    assert np.array_equal(E.bits(got), E.bits(own))


def test_eager_adjust_cvar_batch_values_within_one_ulp_of_the_twin(torch):
    """The CPU values against the twin: equal or one float32 ulp apart.  What is left between them is the last step, `/ 10.0` on the CPU against
    `* 0.1f` on the device; the number of rows it moves is printed."""
    rows, names, got, twin = _eager_cvar(torch)
    ulps = _ulps(got, twin)
    print(f"adjust_cvar_batch on the CPU: {int((ulps != 0).sum())} of {len(rows)} rows differ from the twin, at most {int(ulps.max())} ulp")
    assert ulps.max() <= 1, [(names[i], got[i], twin[i]) for i in np.nonzero(ulps > 1)[0]]
