"""The greedy-on-mean and Double-IQN targets (include/marinenav_hip.h, "Target rules") on the CPU: the admission and the non-degeneracy of every case
tests/test_target_rule_gpu.py runs, the eager float32 definition (`IQNAgent.td_targets` / `compute_loss`) against a literal per-element restatement of the header's
rule and against the float64 statement of tests/iqn_train_rule_f64.py, tests of the tests, the option's refusals, its draws, and a CPU agent stopped and resumed."""
import copy
import math
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import iqn_train_f64 as H              # noqa: E402
import iqn_train_munch_f64 as HM       # noqa: E402
import iqn_train_rule_f64 as HR        # noqa: E402

from distributional_rl_navigation_amd.iqn.agent import IQNAgent      # noqa: E402

TARGET_CASES = [(B, rule) for B in HR.BATCHES for rule in HR.RULES]
STEP_CASES = [(name, rule) for name in HR.STEP_CASES for rule in HR.RULES]


def _agent(c, **kw):
    ag = IQNAgent(26, 9, BATCH_SIZE=c.B, n_step=c.n_step, seed=H.NET_SEED, BUFFER_SIZE=64, device="cpu", target_rule=c.rule, **kw)
    ag.qnetwork_local.load_state_dict(c.local.state_dict())
    ag.qnetwork_target.load_state_dict(c.target.state_dict())
    return ag


def _all_cases():
    for B, rule in TARGET_CASES:
        yield f"B{B}_{rule}", HR.build(B, rule, settle=False)
    for name, rule in STEP_CASES:
        yield f"{name}_{rule}", HR.step_case(name, rule)


# ---- the cases ----------------------------------------------------------------------------------------------------------------------------------------
def test_every_gpu_case_is_admitted_in_full_and_eager_float32_picks_float64s_action():
    for label, c in _all_cases():
        assert c.report["qualified"] >= c.B and c.exp[0].shape[0] == c.B == c.tt.shape[0] == c.ts.shape[0], label
        ref = HR.case_f64(c)
        with torch.no_grad():
            _, a32 = _agent(c).td_targets(c.exp, c.tt, taus_select=c.ts, want_select=True)
        assert np.array_equal(a32.numpy(), ref.a_star), label
        print(f"{label:28s} {c.report}")


def test_every_target_case_tells_the_three_rules_apart():
    """In float64: at least a quarter of the elements choose another action under the other rule, and at least a quarter have a sample whose per-sample max is
    not the chosen action's quantile, and at least a quarter would choose another action from s than from s'.  The two networks have different weights."""
    for label, c in _all_cases():
        assert any(not torch.equal(p, q) for p, q in zip(c.local.parameters(), c.target.parameters()))
        differ, not_max, on_s = HR.non_degenerate(c)
        print(f"{label:28s} a*(mean) != a*(double) on {differ:.3f}, some sample's max is not Z'[j][a*] on {not_max:.3f}, a* from s is another on {on_s:.3f}")
        assert differ >= 0.25 and not_max >= 0.25 and on_s >= 0.25, (label, differ, not_max, on_s)


def test_the_history_steps_are_admitted_along_the_eager_trajectory():
    for rule in HR.RULES:
        ag = _agent(HR.build(HR.HISTORY_B, rule, settle=False))
        for k in range(1, HR.HISTORY_STEPS + 1):
            c = HR.history_case(k, ag.qnetwork_local, ag.qnetwork_target, rule)
            assert c.report["qualified"] >= HR.HISTORY_B
            ag.train(c.exp, c.tt, c.tl, taus_select=c.ts)


# ---- the eager definition ---------------------------------------------------------------------------------------------------------------------------------
def _literal(c):
    """The header's rule, element by element, in float32 scalars on the float32 quantiles of the two networks."""
    f = np.float32
    s, a, r, ns, d = c.exp
    with torch.no_grad():
        zt = c.target(ns, H.N, 1.0, taus=c.tt)[0].numpy()
        zs = c.local(ns, H.N, 1.0, taus=c.ts)[0].numpy() if c.rule == "double" else zt
    y, sel = np.zeros((c.B, H.N), dtype=np.float32), np.zeros(c.B, dtype=np.int64)
    gamma = f(c.gamma_n)
    for b in range(c.B):
        q = []
        for act in range(9):
            acc = f(zs[b, 0, act])
            for j in range(1, 8):
                acc = f(acc + f(zs[b, j, act]))
            q.append(f(f(0.125) * acc))
        best = 0
        for act in range(1, 9):
            if q[act] > q[best]:
                best = act
        sel[b] = best
        rew, done = f(r[b, 0].item()), f(d[b, 0].item())
        for j in range(8):
            # fmaf(gamma * Z, 1 - done, r): one rounding of the sum of the exact product and r -- evaluated in float64, where the product of two float32 is exact
            prod = f(gamma * f(zt[b, j, best]))
            y[b, j] = f(np.float64(prod) * np.float64(f(f(1.0) - done)) + np.float64(rew))
    return y, sel


@pytest.mark.parametrize("B,rule", TARGET_CASES)
def test_eager_equals_the_literal_statement(B, rule):
    c = HR.build(B, rule, settle=False)
    y, sel = _literal(c)
    with torch.no_grad():
        y32, a32 = _agent(c).td_targets(c.exp, c.tt, taus_select=c.ts, want_select=True)
    assert np.array_equal(a32.numpy(), sel)
    assert np.array_equal(y32.view(B, H.N).numpy().view(np.uint32), y.view(np.uint32))


def _eager(ag, c):
    """IQNAgent.train's PyTorch step with the option: compute_loss, clip, torch Adam -> compare_step's namespace plus y."""
    ag.optimizer.zero_grad(set_to_none=False)
    loss, y = ag.compute_loss(c.exp, c.tt, c.tl, taus_select=c.ts, want_targets=True)
    loss.backward()
    torch.nn.utils.clip_grad_norm_(ag.qnetwork_local.parameters(), H.MAX_NORM)
    ag.optimizer.step()
    ps, st = list(ag.qnetwork_local.parameters()), ag.optimizer.state
    return SimpleNamespace(loss=float(loss.detach()), y=y.detach().double().numpy(), grad=H.flat([p.grad for p in ps]), params=H.flat(ps),
                           m=H.flat([st[p]["exp_avg"] for p in ps]), v=H.flat([st[p]["exp_avg_sq"] for p in ps]), t=int(float(st[ps[0]]["step"])))


@pytest.mark.parametrize("B,rule", TARGET_CASES)
def test_compute_loss_against_float64(B, rule):
    """Eager float32 -- loss, y, gradient, moments, parameters -- against the helper under `compare_targets` / `H.compare_step`, with itself as the yardstick: the
    table's eager column is printed, the bars are not degenerate, the float64 side is finite."""
    c = HR.build(B, rule)
    ref = HR.case_f64(c)
    eager = _eager(_agent(c), c)
    assert np.isfinite(ref.y).all() and math.isfinite(ref.loss) and all(np.isfinite(getattr(ref, k)).all() for k in ("grad", "m", "v", "params"))
    w = H.kink_window(ref)
    assert ref.min_abs_td >= w and ref.min_kink >= w
    rows = []
    try:
        ef, ee, bar = HM.compare_targets(ref.y, eager.y, eager.y, f"eager_B{B}_{rule}", rows)
        bars = H.compare_step(ref, eager, eager, f"eager_B{B}_{rule}", rows)
    finally:
        print("\n".join(rows))
    assert 0 < ee and ef == ee < bar
    ge = float(np.abs(eager.grad - ref.grad).max())
    assert 0 < ge < bars.grad and 0 < abs(eager.loss - ref.loss) < bars.loss


@pytest.mark.parametrize("name,rule", STEP_CASES)
def test_conditions_of_the_step_cases(name, rule):
    c = HR.step_case(name, rule)
    HR.assert_conditions(name, c, HR.case_f64(c))


# ---- tests of the tests -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("defect", [d for d in HR.DEFECTS if d != "last_index_ties"])
def test_the_bar_rejects_a_wrong_target(defect):
    """The float64 reference with one defect at a time exceeds compare_targets's bar on every target case of the GPU file."""
    for B in HR.BATCHES:
        for rule in HR.DEFECTS[defect]:
            c = HR.build(B, rule, settle=False)
            ref = HR.case_f64(c)
            with torch.no_grad():
                y = _agent(c).td_targets(c.exp, c.tt, taus_select=c.ts).view(B, H.N).double().numpy()
            HM.compare_targets(ref.y, y, y)
            wrong = HR.case_f64(c, defect=defect)
            with pytest.raises(AssertionError):
                HM.compare_targets(ref.y, wrong.y, y)


@pytest.mark.parametrize("B", HR.BATCHES)
def test_ties_take_the_first_index_and_the_bar_rejects_the_last(B):
    for rule in HR.RULES:
        c = HR.tie_case(B, rule)
        ref = HR.case_f64(c)
        with torch.no_grad():
            y32, a32 = _agent(c).td_targets(c.exp, c.tt, taus_select=c.ts, want_select=True)
        y = y32.view(B, H.N).double().numpy()
        assert (ref.a_star == 2).all() and (a32.numpy() == 2).all(), rule
        wrong = HR.case_f64(c, defect="last_index_ties")
        assert (wrong.a_star == 5).all(), rule      # (the tie is exact in float64 too)
        HM.compare_targets(ref.y, y, y)
        if rule == "double":      # (under "mean" the tied rows are the valued ones: the choice shows in a* alone)
            with pytest.raises(AssertionError):
                HM.compare_targets(ref.y, wrong.y, y)
        else:
            assert np.array_equal(ref.y, wrong.y)


# ---- the agent ------------------------------------------------------------------------------------------------------------------------------------
def _filled_agent(rule, seed=5, **kw):
    ag = IQNAgent(26, 9, BATCH_SIZE=16, seed=seed, BUFFER_SIZE=256, device="cpu", target_rule=rule, **kw)
    g = torch.Generator().manual_seed(11)
    s, a, r, ns, d = H.random_batch(200, g)
    ag.memory.add_batch(s, a.view(-1), r.view(-1), ns, d.view(-1))
    with torch.no_grad():
        for p in ag.qnetwork_target.parameters():
            p.add_(0.05 * torch.randn(p.shape, generator=g))
    return ag


def _bits(ag):
    return [p.detach().clone() for p in ag.qnetwork_local.parameters()]


@pytest.mark.parametrize("rule", HR.RULES)
def test_cpu_agent_stopped_and_resumed_bit_for_bit(rule):
    torch.manual_seed(4)
    ag = _filled_agent(rule)
    saved, losses = None, []
    for k in range(12):
        if k == 5:
            saved = copy.deepcopy(dict(agent=ag.state_dict(), ring=ag.memory.state_dict(), rng=torch.get_rng_state()))
        losses.append(float(ag.train_from_memory()))
    straight = _bits(ag)
    other = _filled_agent(rule, seed=99)
    other.memory.load_state_dict(saved["ring"])
    other.load_state_dict(saved["agent"])
    torch.set_rng_state(saved["rng"])
    resumed = [float(other.train_from_memory()) for _ in range(7)]
    assert resumed == losses[5:]
    for a, b in zip(straight, _bits(other)):
        assert torch.equal(a, b)
    plain = IQNAgent(26, 9, BATCH_SIZE=16, seed=5, BUFFER_SIZE=256, device="cpu")      # the option changes the step
    plain.memory.load_state_dict(saved["ring"])
    plain.load_state_dict(saved["agent"])
    torch.set_rng_state(saved["rng"])
    assert float(plain.train_from_memory()) != losses[5]


def test_taus_consumed():
    """"max" and "mean" draw two tau sets from the global generator per compute_loss, "double" three, in the order of the network calls -- target(s'),
    local(s') (double), local(s)."""
    c = HR.build(16, "double", settle=False)
    for rule, sets in (("max", 2), ("mean", 2), ("double", 3)):
        ag = _agent(c)
        ag.target_rule = rule
        torch.manual_seed(7)
        loss = ag.compute_loss(c.exp)
        after = torch.rand(1)
        torch.manual_seed(7)
        taus = [torch.rand(16, H.N) for _ in range(sets)]
        assert torch.equal(after, torch.rand(1)), rule
        again = ag.compute_loss(c.exp, taus[0], taus[-1], taus_select=taus[1] if sets == 3 else None)
        assert torch.equal(loss, again), rule


def test_max_is_the_default_and_the_code_path_of_before():
    c = HR.build(16, "mean", settle=False)
    ag = IQNAgent(26, 9, BATCH_SIZE=16, seed=H.NET_SEED, BUFFER_SIZE=64, device="cpu")
    assert ag.target_rule == "max"
    with torch.no_grad():
        y = ag.td_targets(c.exp, c.tt)
        z = ag.qnetwork_target(c.exp[3], H.N, taus=c.tt)[0].max(2)[0].unsqueeze(1)
    assert torch.equal(y, c.exp[2].unsqueeze(-1) + (H.GAMMA * z * (1. - c.exp[4].unsqueeze(-1))))


def test_refusals_name_the_option():
    from distributional_rl_navigation_amd import train_iqn as TI
    assert set(TI.TARGET_RULE_REFUSALS) == {"together", "shared", "per", "munchausen"} and all("--target-rule" in v for v in TI.TARGET_RULE_REFUSALS.values())
    with pytest.raises(ValueError, match="target_rule must be"):
        IQNAgent(26, 9, device="cpu", target_rule="softmax", BUFFER_SIZE=64)
    for rule in HR.RULES:
        with pytest.raises(ValueError, match=f"target_rule='{rule}' with munchausen=True"):
            IQNAgent(26, 9, device="cpu", target_rule=rule, munchausen=True, BUFFER_SIZE=64)
        with pytest.raises(ValueError, match=f"target_rule='{rule}' with per=True"):
            IQNAgent(26, 9, device="cpu", target_rule=rule, per=True, BUFFER_SIZE=64)
        with pytest.raises(ValueError, match=f"target_rule='{rule}'.*distributed=True"):
            IQNAgent(26, 9, device="cpu", target_rule=rule, distributed=True, BUFFER_SIZE=64)
        ag = _filled_agent(rule)
        ag.use_fused_graph = True
        with pytest.raises(ValueError, match="target_rule.*use_fused_graph"):
            ag.train_steps_from_memory(2)
        ag.use_fused_graph, ag.use_train_graph = False, True
        with pytest.raises(ValueError, match="target_rule.*use_train_graph"):
            ag.train(ag.memory.sample())
        with pytest.raises(ValueError, match="--target-rule"):
            TI.run_trials_together("cpu", [dict(seed=1, total_timesteps=100, eval_freq=50, save_dir="x")], 4, target_rule=rule)
        # step_sampled, the draw inside the launch (the refusal comes before anything touches a device)
        from distributional_rl_navigation_amd.iqn.fused_train import FusedTrainer
        with pytest.raises(ValueError, match="target_rule.*step_sampled"):
            FusedTrainer.step_sampled(SimpleNamespace(agent=SimpleNamespace(target_rule=rule, munchausen=False, per=False)), None, 0, 0)
        for extra in (["--together"], ["--shared-learner"], ["--per"], ["--munchausen"]):
            with pytest.raises(SystemExit, match="--target-rule"):
                TI.main(["-C", os.devnull, "--target-rule", rule, *extra])
    from distributional_rl_navigation_amd.iqn.group_train import check_agents
    fake = lambda **kw: SimpleNamespace(BATCH_SIZE=32, memory=SimpleNamespace(capacity=1000, size=640), GAMMA=0.99, n_step=1, LR=1e-4, N=8, device="cuda:0",
                                        use_fused_train=True, distributed=False, **kw)      # what check_agents reads of an IQNAgent
    assert len(check_agents([fake(), fake(target_rule="max")])) == 2
    with pytest.raises(ValueError, match="agent 1 uses target_rule='double'"):
        check_agents([fake(), fake(target_rule="double")])
    # the trainer's checkpoint comparison; a run under "max" records no key
    args = TI.run_shaping_args(target_rule="mean")
    assert args["target_rule"] == "mean" and "target_rule" not in TI.run_shaping_args() and "target_rule" not in TI.run_shaping_args(target_rule="max")
    for saved, now in ((args, TI.run_shaping_args()), (TI.run_shaping_args(), args), (args, TI.run_shaping_args(target_rule="double"))):
        with pytest.raises(ValueError, match="other arguments: target_rule was"):
            TI.check_resumable(dict(plan={}, args=saved), {}, now)
    TI.check_resumable(dict(plan={}, args=args), {}, dict(args))
    TI.check_resumable(dict(plan={}, args=TI.run_shaping_args()), {}, TI.run_shaping_args(target_rule="max"))
