"""The DQN baseline's fused gradient step (csrc/dqn_train.hip, dqn/fused_train.py, dqn/group_train.py) against a float64 statement of the same step
(tests/dqn_train_f64.py), with eager float32 PyTorch as the yardstick of how large float32 error is on each input: fused and eager start from the SAME training
state and are both measured against float64 -- loss, gradient, exp_avg, exp_avg_sq, ||grad|| and parameters; the kernel is never its own yardstick.  Every batch
size around the 16-row tiles, unclipped and clipped, both sides of the clip threshold, the edges of the loss phase with their exact-zero consequences, Adam with
history one step at a time and at step 100 000, the multi-step and the grouped launch forms on the same inputs, and the in-launch draw.  The inputs and the
conditions they meet are asserted without a GPU in tests/test_dqn_train_f64_cpu.py.
MN_DQN_F64_TABLE=<file>: the error table of the run (profiles/dqn_train_f64_errors.txt)."""
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import dqn_train_f64 as H      # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_ROWS = []
_AGENTS = {}


@pytest.fixture(scope="module")
def torch():
    import torch as t
    if not t.cuda.is_available():
        pytest.skip("no GPU")
    yield t
    _AGENTS.clear()
    path = os.environ.get("MN_DQN_F64_TABLE")
    if path and _ROWS:
        import ctypes as C
        from distributional_rl_navigation_amd import _capi
        out = (C.c_double * 5)()
        rc = _capi.lib().mn_probe_mfma_clock(C.c_double(50.0), out, C.c_void_p(t.cuda.current_stream(t.device(DEV)).cuda_stream))
        with open(path, "w") as f:
            f.write("# tests/test_dqn_train_f64_gpu.py: |fused - float64| and |eager float32 - float64| of one DQN gradient step from the same state, per case and quantity\n"
                    "# (max = largest entry, rms over all 27 650; 'param big' = |fused - eager| where |g64| > 100 x the gradient bar, 'param rest' = the same elsewhere as a share of its bar)\n"
                    f"# device: {t.cuda.get_device_name(0)}, clock under f16 matrix load (mn_probe_mfma_clock) {out[1] if rc == 0 else float('nan'):.3f} GHz\n")
            f.write("\n".join(_ROWS) + "\n")


# ---- agents, rings, states ----------------------------------------------------------------------------------------------------------------------------
def _ring(ag):
    m = ag.memory
    return (m.states, m.actions, m.rewards, m.next_states, m.dones)


def _rows(ag, idx):
    return tuple(t[idx] for t in _ring(ag))


def _load_nets(torch, ag, c):
    """The case's networks into the agent's flat buffers (the parameters stay views of them); zero moments, step 0."""
    ft = ag._fused_trainer()
    ag.q_net.load_state_dict(c.local.state_dict())
    ag.q_net_target.load_state_dict(c.target.state_dict())
    assert ft.owns(ag) and torch.equal(ft.local.cpu(), torch.cat([p.detach().reshape(-1) for p in c.local.parameters()]))
    assert torch.equal(ft.target.cpu(), torch.cat([p.detach().reshape(-1) for p in c.target.parameters()]))
    ft.exp_avg.zero_(); ft.exp_avg_sq.zero_(); ft.step_dev.zero_()
    ag._train_path = "hip"      # the device counter is authoritative
    ag.policy.weights_changed()


def _load_ring(torch, ag, c, seed, decoys=True):
    """The case's rows into the ring among as many decoy rows, all at shuffled positions; returns the positions of the case's rows in batch order (`idx` of the
    step: a gather, not arange).  decoys False: the ring is exactly the case's rows."""
    B, m = c.B, ag.memory
    g = torch.Generator().manual_seed(seed)
    decoy = H.random_batch(B, g)
    perm = torch.randperm(2 * B if decoys else B, generator=g).to(DEV)
    pos, dpos = perm[:B], perm[B:]
    assert m.capacity >= perm.numel()
    for dst, x, dx in zip(_ring(ag), c.exp, decoy):
        dst.zero_()
        dst[pos] = x.to(DEV)
        if decoys:
            dst[dpos] = dx.to(DEV)
    m.size, m.ptr = perm.numel(), perm.numel() % m.capacity
    m.version += 1
    for got, want in zip(_rows(ag, pos), c.exp):
        assert torch.equal(got.cpu(), want)
    return pos


def _agent(torch, c, slot=0, decoys=True):
    """The fused agent of this batch size (built once per size and learner slot) with the case's networks and rows; returns (agent, idx)."""
    from distributional_rl_navigation_amd.dqn import DQNAgent
    ag = _AGENTS.get((c.B, slot))
    if ag is None:
        ag = _AGENTS[(c.B, slot)] = DQNAgent(device=DEV, fused_train=True, batch_size=c.B, buffer_size=max(64, 2 * c.B), seed=H.NET_SEED)
        assert ag._uses_fused() and ag.gamma == H.GAMMA and ag.learning_rate == H.LR and ag.max_grad_norm == H.MAX_NORM
    _load_nets(torch, ag, c)
    return ag, _load_ring(torch, ag, c, 7000 + 10 * c.B + slot, decoys)


class _State:
    """Snapshot / restore of a fused agent's whole training state (parameters, target, Adam moments, step and draw counters) -- tests/test_dqn_train_multi_gpu.py's."""

    def __init__(self, ag):
        ft = ag._fused_trainer()
        self.ag, self.t = ag, [x.clone() for x in self._tensors(ft)]

    @staticmethod
    def _tensors(ft):
        return (ft.local, ft.target, ft.exp_avg, ft.exp_avg_sq, ft.step_dev, ft.rng_state)

    def restore(self):
        for d, s in zip(self._tensors(self.ag._fused), self.t):
            d.copy_(s)
        self.ag._train_path = "hip"      # the device counter is authoritative: the next eager step takes it over
        self.ag.policy.weights_changed()


def _f64(ag, rows):
    """The float64 step from the agent's current state: networks, both moments and the step counter read from the trainer."""
    ft = ag._fused
    return H.dqn_f64_step(ag.q_net, ag.q_net_target, rows, ag.gamma, m=ft.exp_avg, v=ft.exp_avg_sq, t=int(ft.step_dev.item()), lr=ag.learning_rate,
                          max_norm=ag.max_grad_norm)


def _fused_result(ag, loss):
    """What a fused launch left, read from the trainer's own buffers (not through p.grad, which an eager step re-points)."""
    ft = ag._fused
    return SimpleNamespace(loss=float(loss), grad=H.flat([ft.grad]), params=H.flat([ft.local]), m=H.flat([ft.exp_avg]), v=H.flat([ft.exp_avg_sq]),
                           t=int(ft.step_dev.item()))


def _eager_step(ag, rows):
    ag.fused_train = False
    try:
        loss = ag.train(rows)
    finally:
        ag.fused_train = True
    grad = H.flat([p.grad for p in ag.q_net.parameters()])
    ag._enter_train_path("hip")      # the optimizer's step count back into the device counter
    ft = ag._fused
    return SimpleNamespace(loss=float(loss), grad=grad, params=H.flat(list(ag.q_net.parameters())), m=H.flat([ft.exp_avg]), v=H.flat([ft.exp_avg_sq]),
                           t=int(ft.step_dev.item()))


def _compare(ag, state, idx, label, fused=None):
    """Float64, the fused step (`train_fused(idx)`) and the eager step (`train(rows)`) from `state`, the two float32 steps against float64 (H.compare_step);
    `fused`: a fused result taken from `state` already, by whichever launch form.  Leaves the agent at the eager result.  Returns (float64, fused, eager, bars)."""
    state.restore()
    rows = _rows(ag, idx)
    ref = _f64(ag, rows)
    if fused is None:
        fused = _fused_result(ag, ag.train_fused(idx))
        state.restore()
    eager = _eager_step(ag, rows)
    n0 = len(_ROWS)
    try:
        bars = H.compare_step(ref, fused, eager, label, _ROWS)
    finally:
        print("\n".join(_ROWS[n0:]))
    return ref, fused, eager, bars


def _run_case(torch, name, label=None, slot=0):
    c = H.case(name)
    ag, idx = _agent(torch, c, slot)
    state = _State(ag)
    ref, fused, eager, bars = _compare(ag, state, idx, label or name)
    cond = H.CASES[name][1]
    if cond.get("clipped") is not None:      # the input is on the side of the threshold the CPU file asserts
        assert (ref.norm > 12.0) if cond["clipped"] else (ref.norm < 8.0), (name, ref.norm)
    if "norm" in cond:
        assert cond["norm"][0] <= ref.norm <= cond["norm"][1], (name, ref.norm)
    if "lin_share" in cond:
        assert ref.lin_share == cond["lin_share"], (name, ref.lin_share)
    return SimpleNamespace(c=c, ag=ag, idx=idx, state=state, ref=ref, fused=fused, eager=eager, bars=bars)


def _same_bits(a, b):
    return a.loss == b.loss and all(np.array_equal(getattr(a, k), getattr(b, k)) for k in ("grad", "params", "m", "v"))


# ---- 1. every batch size around the tiles, unclipped and clipped ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("net", ["seeded", "pretrained"])
@pytest.mark.parametrize("B", H.SWEEP)
def test_batch_sweep(torch, B, net):
    """15, 31, 255: the last live slot of a tile; 17, 33: one live row in the last workgroup; 16, 32, 256: whole tiles.  The seeded network never clips on these
    batches, the pretrained one always does (norms in the hundreds; its rows are on the linear branch, tests/dqn_train_f64.py says why)."""
    r = _run_case(torch, f"sweep_B{B}" if net == "seeded" else f"sweep_pretrained_B{B}")
    assert r.fused.t == 1 and np.abs(r.fused.params - r.ref.p0).max() > 0.5 * H.LR


# ---- 2. both sides of the clip threshold ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", list(H.THRESHOLD_STEEP))
def test_both_sides_of_the_clip_threshold(torch, B):
    """One batch under two output layers, float64 norm 8.0-9.6 and 10.4-12.0: the fused step takes the branch float64 dictates (the ||grad|| line of compare_step;
    and here, coarsely -- float32 resolves 1e-7 of the norm, the wrong branch is 4e-2 of it away)."""
    for side in ("hi", "lo"):
        r = _run_case(torch, f"threshold_{side}_B{B}")
        n = float(np.linalg.norm(r.fused.grad))
        if side == "lo":
            assert 8.0 <= r.ref.norm <= 9.6 and abs(n - r.ref.norm) <= 1e-3 * r.ref.norm
        else:
            assert 10.4 <= r.ref.norm <= 12.0 and abs(n - H.MAX_NORM) <= 1e-3 * H.MAX_NORM


# ---- 3. edges of the loss phase ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", H.EDGES)
def test_loss_phase_edges(torch, name):
    r = _run_case(torch, name)
    kw = H.CASES[name][0]
    if kw.get("action") in (0, 8):
        H.assert_untaken_actions_untouched(r.fused, r.ref.p0, kw["action"])
        H.assert_untaken_actions_untouched(r.eager, r.ref.p0, kw["action"])
    if kw.get("action") == "all":
        for a in range(9):
            (lo, hi), b = H.output_rows(a)
            assert np.abs(r.fused.grad[lo:hi]).max() > 0 and r.fused.grad[b] != 0
    if kw.get("zero_sonar") == "states":
        H.assert_sensor_weight_untouched(r.fused, r.ref.p0)
        H.assert_sensor_weight_untouched(r.eager, r.ref.p0)
    if kw.get("dones") == 1:
        # y = reward exactly, whatever the (finite) target network and the next states hold -- bit for bit
        ag, ft = r.ag, r.ag._fused
        r.state.restore()
        g = torch.Generator().manual_seed(77)
        with torch.no_grad():
            ft.target.add_((0.3 * torch.randn(ft.target.shape, generator=g)).to(DEV))
        ag.memory.next_states[r.idx] = (torch.randn(r.c.B, 26, generator=g) * 7).to(DEV)
        assert not torch.equal(ft.target, r.state.t[1]) and bool(torch.isfinite(ft.target).all())
        again = _fused_result(ag, ag.train_fused(r.idx))
        assert _same_bits(again, r.fused)


# ---- 4. Adam with history, one step at a time; the late step ------------------------------------------------------------------------------------------------
def test_adam_with_history_and_the_late_step(torch):
    """12 consecutive steps on fresh batches, each taken float64 / fused / eager from the state in front of it (moments and step count go into the float64 step: no
    trajectory divergence enters), continued from the FUSED result: bias correction at t > 1, exp_avg and exp_avg_sq against something other than the kernel.  Then
    step 100 000 from that state: both bias corrections are 1 and pow(b, t) underflows towards 0."""
    ag, _ = _agent(torch, H.history_batch(1))
    start = ag._fused.local.clone()
    for k in range(1, H.HISTORY_STEPS + 2):
        idx = _load_ring(torch, ag, H.history_batch(k), 8000 + k)
        if k == H.HISTORY_STEPS + 1:
            assert float((ag._fused.local - start).abs().max()) > 5 * H.LR      # the run moved the weights: it proves something
            ag._fused.step_dev.fill_(H.LATE_T)
        t0 = int(ag._fused.step_dev.item())
        assert t0 == (k - 1 if k <= H.HISTORY_STEPS else H.LATE_T)
        state = _State(ag)
        ref, fused, eager, _ = _compare(ag, state, idx, f"history_B{H.HISTORY_B} step {t0 + 1}")
        H.assert_margin(f"history step {k}", ref)
        assert ref.t == fused.t == eager.t == t0 + 1
        if k > 1:
            assert float(state.t[2].abs().max()) > 0 and float(state.t[3].max()) > 0
        state.restore()
        again = _fused_result(ag, ag.train_fused(idx))      # continue from the fused result
        assert _same_bits(again, fused)
    assert int(ag._fused.step_dev.item()) == H.LATE_T + 1


# ---- 5. the other launch forms on the same inputs -----------------------------------------------------------------------------------------------------------
def _mixed_rows(torch, ag, n, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.stack([torch.randperm(ag.memory.size, generator=g)[:ag.batch_size] for _ in range(n)]).to(DEV)


@pytest.mark.parametrize("B", [1, 15, 16, 17, 32])
def test_multi_step_call_against_float64(torch, B):
    """`FusedTrainer.steps`: a call of one step, and the last step of a 3-step call with float64 taken from the state after step 2 (non-zero moments, t = 3)."""
    ag, idx = _agent(torch, H.case(f"sweep_B{B}"))
    ft, m = ag._fused, ag.memory
    state = _State(ag)
    losses = ft.steps(_ring(ag), m.size, B, 1, idx[None])
    fused = _fused_result(ag, losses[0])
    assert torch.equal(ft.last_idx, idx[None])
    _compare(ag, state, idx, f"sweep_B{B} (steps, n = 1)", fused=fused)
    idx3 = torch.cat([_mixed_rows(torch, ag, 2, 40 + B), idx[None]])
    state.restore()
    ft.steps(_ring(ag), m.size, B, 2, idx3[:2])
    after2 = _State(ag)
    state.restore()
    losses = ft.steps(_ring(ag), m.size, B, 3, idx3)
    fused = _fused_result(ag, losses[2])
    ref, _, _, _ = _compare(ag, after2, idx, f"sweep_B{B} (steps, 3 of 3)", fused=fused)
    assert ref.t == fused.t == 3 and float(after2.t[2].abs().max()) > 0


def _group(torch, B):
    from distributional_rl_navigation_amd.dqn.group_train import LearnerGroup
    names = (f"all_done_B{B}", f"all_linear_B{B}", f"sweep_B{B}")
    pairs = [_agent(torch, H.case(n), slot) for slot, n in enumerate(names)]
    ags, idxs = [a for a, _ in pairs], [i for _, i in pairs]
    return names, ags, idxs, LearnerGroup(ags)


@pytest.mark.parametrize("B", [17, 100, 256])
def test_grouped_launch_against_float64(torch, B):
    """Three different cases of one batch size in ONE launch (all rows terminal, all rows on the linear branch, the sweep case): each learner against its own float64."""
    names, ags, idxs, grp = _group(torch, B)
    try:
        states = [_State(a) for a in ags]
        losses = grp.train(torch.stack(idxs))
        assert torch.equal(grp.last_idx, torch.stack(idxs))
        fused = [_fused_result(a, l) for a, l in zip(ags, losses)]
        for name, a, i, s, f in zip(names, ags, idxs, states, fused):
            ref, _, _, _ = _compare(a, s, i, f"{name} (group of 3)", fused=f)
            assert ref.t == f.t == 1
        assert fused[0].loss != fused[1].loss != fused[2].loss
    finally:
        grp.close()


def test_grouped_multi_step_call_against_float64(torch):
    """`LearnerGroup.train_many(3, idx)` at B = 17: every learner's last step against float64 from its state after step 2."""
    names, ags, idxs, grp = _group(torch, 17)
    try:
        states = [_State(a) for a in ags]
        idx3 = torch.stack([torch.cat([_mixed_rows(torch, a, 2, 60 + g), i[None]]) for g, (a, i) in enumerate(zip(ags, idxs))])      # [G][3][B]
        grp.train_many(2, idx3[:, :2].contiguous())
        after2 = [_State(a) for a in ags]
        for s in states:
            s.restore()
        losses = grp.train_many(3, idx3)
        fused = [_fused_result(a, l[2]) for a, l in zip(ags, losses)]
        for name, a, i, s, f in zip(names, ags, idxs, after2, fused):
            ref, _, _, _ = _compare(a, s, i, f"{name} (group of 3, 3 of 3)", fused=f)
            assert ref.t == f.t == 3 and float(s.t[2].abs().max()) > 0
    finally:
        grp.close()


# ---- 6. drawn in the launch -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ring", ["exact", "double"])
@pytest.mark.parametrize("B", [17, 100])
def test_step_drawn_in_the_launch(torch, B, ring):
    """`train_fused()` without rows: the batch the launch drew for itself (`last_idx`), gathered here, through the float64 and the eager step.  A ring of exactly B
    rows is drawn whole, in some order; of 2 B rows, B distinct ones."""
    c = H.case(f"sweep_B{B}")
    ag, _ = _agent(torch, c, decoys=ring == "double")
    ft = ag._fused
    assert ag.memory.size == (B if ring == "exact" else 2 * B)
    state = _State(ag)
    fused = _fused_result(ag, ag.train_fused())
    drawn = ft.last_idx.clone()
    assert drawn.shape == (B,) and drawn.unique().numel() == B and int(drawn.min()) >= 0 and int(drawn.max()) < ag.memory.size
    if ring == "exact":
        assert sorted(drawn.tolist()) == list(range(B)) and drawn.tolist() != list(range(B))
    assert int(ft.rng_state[1]) == int(state.t[5][1]) + 1 and int(ft.rng_state[0]) == int(state.t[5][0])
    _compare(ag, state, drawn, f"drawn_B{B} (ring of {ag.memory.size})", fused=fused)


# ---- 7. a partial last tile with structure ------------------------------------------------------------------------------------------------------------------
def test_partial_last_tile_with_structure(torch):
    """B = 17: the one live row of the second workgroup is terminal and alone takes action 8, the 16 rows of the first are not terminal and take actions 0..7: the
    gradient of q_net.4's row 8 comes from the second workgroup alone, the other rows' from the first alone."""
    r = _run_case(torch, "last_tile_B17")
    (lo, hi), b = H.output_rows(8)
    want = r.ref.grad[lo:hi]
    assert np.abs(want).max() > 100 * r.bars.grad and np.abs(r.fused.grad[lo:hi] - want).max() <= r.bars.grad
    assert abs(r.fused.grad[b] - r.ref.grad[b]) <= r.bars.grad and abs(r.ref.grad[b]) > 100 * r.bars.grad
    for a in range(8):      # (two rows each: their bias gradients +-1 / 17 may cancel exactly, their weight gradients do not)
        (lo, hi), b = H.output_rows(a)
        assert np.abs(r.fused.grad[lo:hi]).max() > 0
