"""Prioritized replay on the device (csrc/per.hip, the weighted step of csrc/iqn_train.hip) against its host twin (tests/per_twin.py) and a float64
statement of the weighted gradient step (tests/iqn_train_per_f64.py): a ring of 2 053 rows -- two full blocks of 1 024 and a partial one.  The sampler's
rows are the twin's exactly, from the masses read back from the device; appends and updates leave exact integer sums; the weighted step is held to float64
by eager float32 PyTorch's own error (tests/iqn_train_f64.py `compare_step`)."""
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import iqn_train_f64 as H          # noqa: E402
import iqn_train_per_f64 as HP     # noqa: E402
import per_twin as T               # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CAP = 2053
SEED = 0x1234ABCD5678
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def torch():
    import torch as t
    if not t.cuda.is_available():
        pytest.skip("no GPU")
    return t


def _store(torch, twin=None, seed=SEED):
    from distributional_rl_navigation_amd.iqn.priority import PriorityStore
    ps = PriorityStore(CAP, DEV, seed)
    if twin is not None:
        ps.mass.copy_(torch.from_numpy(twin.mass.view(np.int32).copy()))
        ps.bsum.copy_(torch.from_numpy(twin.bsum.view(np.int64).copy()))
        ps.mmax.fill_(int(twin.mmax))
    return ps


def _read_back(ps):
    """The device's words as a twin store."""
    st = T.Store(ps.capacity)
    st.mass[:] = ps.mass.cpu().numpy().view(np.uint32)
    st.bsum[:] = ps.bsum.cpu().numpy().view(np.uint64)
    st.mmax = int(ps.mmax.cpu()[0])
    return st


def _sums_are_exact(st):
    assert np.array_equal(st.bsum, T.block_sums(st.mass)), "block sums are not the sums of the read-back masses"


# ---- the sampler ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [700, 1024, 1025, 2053])
@pytest.mark.parametrize("name", ["equal", "one_heavy", "holes", "random"])
def test_sampler_rows_equal_the_twin(torch, name, size):
    ps = _store(torch, T.hand_made(name, size, CAP))
    st = _read_back(ps)
    ctr = 0
    for batch in (2, 16, 32, 256):
        for beta in (0.4, 1.0):
            idx, w, taus = (x.cpu().numpy() for x in ps.sample(size, batch, beta))
            ti, tw, tt = T.sample(st, size, batch, beta, SEED, ctr)
            ctr += 1
            assert idx.tolist() == ti.tolist(), (name, size, batch)
            assert int(idx.max()) < size and (st.mass[idx] > 0).all()
            w64 = T.weights_f64(st.mass[ti], size, st.total, beta)
            rel = np.abs(w - w64) / w64
            print(f"{name} size {size} batch {batch} beta {beta}: weights max rel err {rel.max():.3e}")
            assert rel.max() <= 1e-5 and w.max() == 1.0
            assert np.array_equal(taus, tt)
    assert ps.rng_state.cpu().tolist() == [SEED, ctr]
    if name == "one_heavy":
        assert len(set(idx.tolist())) < 256
    _sums_are_exact(_read_back(ps))      # the sampler writes nothing


def test_sampler_refusals_launch_nothing(torch):
    import ctypes as C
    from distributional_rl_navigation_amd import _capi
    ps = _store(torch, T.hand_made("equal", 700, CAP))
    idx, w, taus = ps._buffers(32)
    p = lambda t: C.c_void_p(t.data_ptr())
    L, s = _capi.lib(), _capi.stream_ptr(ps.device)
    call = lambda size, cap, batch, beta: L.mn_per_sample(p(ps.mass), p(ps.bsum), size, cap, batch, C.c_float(beta), p(ps.rng_state), p(idx), p(w), p(taus), s)
    assert call(700, CAP, 32, 0.4) == 0
    for bad in ((31, CAP, 32, 0.4), (CAP + 1, CAP, 32, 0.4), (700, (1 << 20) + 1, 32, 0.4), (700, CAP, 0, 0.4), (700, CAP, 1025, 0.4), (700, CAP, 32, -1.0)):
        assert call(*bad) != 0, bad
    assert L.mn_per_append(p(ps.mass), p(ps.bsum), p(ps.mmax), CAP, 1, CAP, s) != 0 and L.mn_per_append(p(ps.mass), p(ps.bsum), p(ps.mmax), 0, CAP + 1, CAP, s) != 0
    assert L.mn_per_update(p(ps.mass), p(ps.bsum), p(ps.mmax), p(idx), p(w), 1025, C.c_float(0.6), C.c_float(1e-6), CAP, s) != 0
    torch.cuda.synchronize()
    assert ps.rng_state.cpu().tolist() == [SEED, 1]
    with pytest.raises(ValueError, match="2\\^20"):
        from distributional_rl_navigation_amd.iqn.replay_buffer import ReplayBuffer
        ReplayBuffer((1 << 20) + 1, 32, "cpu", 0, 0.99, prioritized=True)


# ---- append ------------------------------------------------------------------------------------------------------------------------------------
def _vector_step(torch, k, g):
    return (torch.randn(k, 26, generator=g).to(DEV), torch.randint(0, 9, (k,), generator=g).to(torch.int32).to(DEV), torch.randn(k, generator=g).to(DEV),
            torch.randn(k, 26, generator=g).to(DEV), (torch.rand(k, generator=g) < 0.1).to(torch.uint8).to(DEV))


@pytest.mark.parametrize("n_step", [1, 3])
def test_append_across_the_wrap(torch, n_step):
    """add_vector_step (n_step 1: mn_replay_append; 3: the window append, which emits nothing for its first two calls), with the largest mass moving in between."""
    from distributional_rl_navigation_amd.iqn.replay_buffer import ReplayBuffer
    rb = ReplayBuffer(CAP, 32, DEV, 3, 0.99, n_step=n_step, prioritized=True)
    st = T.Store(CAP)
    g = torch.Generator().manual_seed(1)
    ptr, emitted = 0, 0
    for call in range(6 + n_step):      # 500 rows a call: past the wrap
        rb.add_vector_step(*_vector_step(torch, 500, g))
        if call + 1 >= n_step:
            T.append(st, ptr, 500)
            ptr, emitted = (ptr + 500) % CAP, emitted + 500
        got = _read_back(rb.priority)
        assert np.array_equal(got.mass, st.mass) and np.array_equal(got.bsum, st.bsum) and got.mmax == st.mmax, call
        if call == 3:      # a new largest mass: later rows enter with it
            rows = torch.tensor([5, 1030], dtype=torch.int64, device=DEV)
            rb.priority.update(rows, torch.tensor([3.0, 0.5], device=DEV), 1.0, 0.0)
            T.update(st, [5, 1030], [3 * T.MASS_ONE, T.MASS_ONE // 2])
    assert emitted > CAP and rb.size == CAP and rb.ptr == ptr and st.mmax == 3 * T.MASS_ONE
    assert (st.mass == 3 * T.MASS_ONE).sum() > 500


def test_append_behind_mn_step_append(torch):
    from distributional_rl_navigation_amd.iqn.replay_buffer import ReplayBuffer
    from distributional_rl_navigation_amd.marinenav_env.vec_env import VecMarineNavEnv
    n = 600
    env = VecMarineNavEnv(n, seed=3, device=DEV, precision="f64")
    try:
        rb = ReplayBuffer(CAP, 32, DEV, 3, 0.99, prioritized=True)
        st = T.Store(CAP)
        obs = env.reset()
        g = torch.Generator().manual_seed(2)
        ptr = 0
        for _ in range(4):      # 2 400 rows: across the wrap
            a = torch.randint(0, 9, (n,), generator=g).to(torch.int32).to(DEV)
            nxt, _, _, _ = env.step_append(a, obs, rb)
            T.append(st, ptr, n)
            ptr = (ptr + n) % CAP
            obs = env.reset_done()
            got = _read_back(rb.priority)
            assert np.array_equal(got.mass, st.mass) and np.array_equal(got.bsum, st.bsum)
        assert rb.ptr == ptr and rb.size == CAP
    finally:
        env.close()


# ---- update ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch", [2, 16, 32, 256])
def test_update(torch, batch):
    ps = _store(torch, T.hand_made("random", CAP, CAP))
    st = _read_back(ps)
    g = np.random.default_rng(batch)
    idx = g.permutation(np.setdiff1d(np.arange(CAP), [1023, 1500]))[:batch]      # distinct rows, then the repeats
    if batch >= 16:
        idx[[1, 7, 12]] = 1500      # one row three times: slot 12 wins
        idx[[3, 4]] = 1023
    d = (g.random(batch) * 10 ** g.uniform(-5, 3, batch)).astype(np.float32)
    if batch >= 16:
        d[0], d[2] = 0.0, 1e30      # the clamps: mass 1 and 2^31 - 1
    ps.update(torch.from_numpy(idx).to(DEV), torch.from_numpy(d).to(DEV), 0.6, 1e-6)
    got = _read_back(ps)
    _sums_are_exact(got)
    m64 = T.new_mass_f64(d, 0.6, 1e-6)
    winners = {int(r): k for k, r in enumerate(idx)}      # the highest slot of every row
    for r, k in winners.items():
        assert abs(int(got.mass[r]) - int(m64[k])) <= 1 + 1e-5 * int(m64[k]), (r, k, int(got.mass[r]), int(m64[k]))
    untouched = np.setdiff1d(np.arange(CAP), idx)
    assert np.array_equal(got.mass[untouched], st.mass[untouched])
    assert got.mmax == max(st.mmax, max(int(got.mass[r]) for r in winners))
    if batch >= 16:
        assert winners[1500] == 12 and got.mass[idx[0]] == 16 and got.mass[idx[2]] == T.MASS_MAX and got.mmax == T.MASS_MAX      # (1e-6 ** 0.6 * 65536 = 16.46)
        ps.update(torch.from_numpy(idx[:2].copy()).to(DEV), torch.tensor([0.0, float("nan")], device=DEV), 1.0, 0.0)      # the lower clamp, and a NaN
        low = _read_back(ps)
        _sums_are_exact(low)
        assert low.mass[idx[0]] == 1 and low.mass[idx[1]] == 1 and low.mmax == T.MASS_MAX


# ---- the weighted step -------------------------------------------------------------------------------------------------------------------------
def _agent(torch, c, **attrs):
    from distributional_rl_navigation_amd.iqn.agent import IQNAgent
    ag = IQNAgent(26, 9, BATCH_SIZE=c.B, n_step=c.n_step, seed=H.NET_SEED, BUFFER_SIZE=64, device=DEV)
    ag.qnetwork_local.load_state_dict(c.local.state_dict())
    ag.qnetwork_target.load_state_dict(c.target.state_dict())
    for k, v in attrs.items():
        setattr(ag, k, v)
    ag._fused_trainer()
    return ag


class _State:
    def __init__(self, ag):
        ft = ag._fused_trainer()
        self.ag, self.t = ag, [x.clone() for x in (ft.local, ft.target, ft.exp_avg, ft.exp_avg_sq, ft.step_dev)]

    def restore(self):
        from distributional_rl_navigation_amd.iqn.fused_act import weights_changed
        ft = self.ag._fused
        for d, s in zip((ft.local, ft.target, ft.exp_avg, ft.exp_avg_sq, ft.step_dev), self.t):
            d.copy_(s)
        self.ag._train_path = "hip"
        weights_changed(self.ag.qnetwork_local)


def _result(ag, loss, abs_td):
    ft = ag._fused
    ag._enter_train_path("hip")
    ps = list(ag.qnetwork_local.parameters())
    return SimpleNamespace(loss=float(loss), grad=H.flat([p.grad for p in ps]), params=H.flat(ps), m=H.flat([ft.exp_avg]), v=H.flat([ft.exp_avg_sq]),
                           t=int(ft.step_dev.item()), abs_td=abs_td.detach().double().cpu().numpy())


def _fused_weighted(torch, ag, exp, tt, tl, w):
    ft = ag._fused_trainer()
    ag._enter_train_path("hip")
    idx = torch.arange(exp[0].shape[0], dtype=torch.int64, device=DEV)
    loss, abs_td = ft.step_per(tuple(t.contiguous() for t in exp), idx, tt.contiguous(), tl.contiguous(), w.contiguous())
    return _result(ag, loss, abs_td)


def _eager_weighted(torch, ag, exp, tt, tl, w):
    """IQNAgent.train's PyTorch step with the weighted loss."""
    from distributional_rl_navigation_amd.iqn.fused_act import weights_changed
    ag._enter_train_path("torch")
    ag.optimizer.zero_grad(set_to_none=False)
    loss, abs_td = ag.compute_loss(exp, tt, tl, weights=w, want_abs_td=True)
    loss.backward()
    torch.nn.utils.clip_grad_norm_(ag.qnetwork_local.parameters(), 0.5)
    ag.optimizer.step()
    weights_changed(ag.qnetwork_local)
    return _result(ag, loss.detach(), abs_td)


def _f64_weighted(ag, exp, tt, tl, w):
    ft = ag._fused
    return HP.f64_step_weighted(ag.qnetwork_local, ag.qnetwork_target, exp, tt, tl, H.GAMMA ** ag.n_step, w, m=ft.exp_avg, v=ft.exp_avg_sq, t=int(ft.step_dev.item()))


def _compare_weighted(torch, ag, state, exp, tt, tl, w, label, order=("fused", "eager")):
    """Float64, fused and eager from `state`; leaves the agent at the result of the step named last in `order`."""
    state.restore()
    ref = _f64_weighted(ag, exp, tt, tl, w)
    out = {}
    for which in order:
        state.restore()
        out[which] = (_fused_weighted if which == "fused" else _eager_weighted)(torch, ag, exp, tt, tl, w)
    rows = []
    try:
        H.compare_step(ref, out["fused"], out["eager"], label, rows)
        HP.compare_abs_td(ref.abs_td, out["fused"].abs_td, out["eager"].abs_td, label, rows)
    finally:
        print("\n".join(rows))
    return ref, out["fused"], out["eager"]


@pytest.mark.parametrize("B", [2, 32, 256])
def test_weighted_step_against_float64(torch, B):
    c = H.build_case("random", B)
    ag = _agent(torch, c)
    exp, tt, tl = tuple(x.to(DEV) for x in c.exp), c.tt.to(DEV), c.tl.to(DEV)
    w = HP.case_weights(B).to(DEV)
    state = _State(ag)
    ref, fused, eager = _compare_weighted(torch, ag, state, exp, tt, tl, w, f"weighted_B{B}")
    kw = H.kink_window(ref)
    assert ref.min_abs_td >= kw and ref.min_kink >= kw
    # the weights matter: the unweighted float64 step is elsewhere
    plain = H.f64_step(c.local, c.target, c.exp, c.tt, c.tl, c.gamma_n)
    assert abs(plain.loss - ref.loss) > 1e-3 * abs(plain.loss)


@pytest.mark.parametrize("B", [2, 32, 256])
def test_weights_of_one_equal_the_unweighted_kernel_bit_for_bit(torch, B):
    c = H.build_case("random", B)
    ag = _agent(torch, c, two_launch_step=False)      # the separate launches: mn_iqn_train_grad + mn_iqn_train_adam
    exp, tt, tl = tuple(x.to(DEV) for x in c.exp), c.tt.to(DEV), c.tl.to(DEV)
    state = _State(ag)
    ag.use_fused_train = True
    plain = _result(ag, ag.train(exp, tt, tl), torch.zeros(B))
    state.restore()
    ones = _fused_weighted(torch, ag, exp, tt, tl, torch.ones(B, device=DEV))
    for k in ("grad", "params", "m", "v"):
        assert np.array_equal(getattr(plain, k), getattr(ones, k)), k
    assert plain.loss == ones.loss and plain.t == ones.t == 1
    assert (ones.abs_td > 0).all()


def test_a_zero_weight_element_contributes_no_gradient(torch):
    B = 32
    c = H.build_case("random", B)
    ag = _agent(torch, c)
    exp, tt, tl = [x.to(DEV) for x in c.exp], c.tt.to(DEV), c.tl.to(DEV)
    w = HP.case_weights(B).to(DEV)
    w[5] = 0.0
    state = _State(ag)
    a = _fused_weighted(torch, ag, tuple(exp), tt, tl, w)
    exp2 = [x.clone() for x in exp]      # another transition in slot 5: another state, action, reward, next state
    exp2[0][5] = exp[0][6]; exp2[1][5] = (exp[1][5] + 1) % 9; exp2[2][5] = exp[2][5] + 7.0; exp2[3][5] = exp[3][7]
    state.restore()
    b = _fused_weighted(torch, ag, tuple(exp2), tt, tl, w)
    assert np.array_equal(a.grad, b.grad) and a.loss == b.loss and np.array_equal(a.params, b.params)
    assert a.abs_td[5] != b.abs_td[5] and np.array_equal(np.delete(a.abs_td, 5), np.delete(b.abs_td, 5))      # its priority is still reported
    w[5] = 0.5
    state.restore()
    assert not np.array_equal(_fused_weighted(torch, ag, tuple(exp2), tt, tl, w).grad, a.grad)


# ---- twenty prioritized gradient steps -----------------------------------------------------------------------------------------------------------
N_ROWS, PER_BATCH, PER_STEPS = 1500, 32, 20


def _per_agent(torch, fill=True):
    from distributional_rl_navigation_amd.iqn.agent import IQNAgent
    ag = IQNAgent(26, 9, BATCH_SIZE=PER_BATCH, seed=H.NET_SEED, BUFFER_SIZE=CAP, device=DEV, per=True)
    ag.per_beta_steps = PER_STEPS
    if fill:
        g = torch.Generator().manual_seed(77)
        s, a, r, ns, d = H.random_batch(N_ROWS, g)
        ag.memory.add_batch(s.to(DEV), a.view(-1).to(DEV), r.view(-1).to(DEV), ns.to(DEV), d.view(-1).to(DEV))
        with torch.no_grad():
            for p in ag.qnetwork_target.parameters():
                p.add_(0.05 * torch.randn(p.shape, generator=g).to(DEV))
    ag._fused_trainer()
    return ag


class _PerState(_State):
    """The trainer's state plus the priority store's and beta's position."""

    def __init__(self, ag):
        super().__init__(ag)
        pr = ag.memory.priority
        self.p = [x.clone() for x in (pr.mass, pr.bsum, pr.mmax, pr.rng_state)]
        self.counters = (ag._per_step, ag.grad_steps)

    def restore(self):
        super().restore()
        pr = self.ag.memory.priority
        for d, s in zip((pr.mass, pr.bsum, pr.mmax, pr.rng_state), self.p):
            d.copy_(s)
        self.ag._per_step, self.ag.grad_steps = self.counters


def _per_bits(ag, loss):
    pr = ag.memory.priority
    ft = ag._fused
    return dict(local=ft.local.cpu(), exp_avg=ft.exp_avg.cpu(), exp_avg_sq=ft.exp_avg_sq.cpu(), step=ft.step_dev.cpu(), loss=loss.detach().cpu().reshape(1).clone(),
                mass=pr.mass.cpu(), bsum=pr.bsum.cpu(), mmax=pr.mmax.cpu(), rng=pr.rng_state.cpu())


def test_twenty_prioritized_steps_fused_and_eager_against_float64(torch):
    ag = _per_agent(torch)
    m = ag.memory
    ring = (m.states, m.actions, m.rewards, m.next_states, m.dones)
    repeats = 0
    for k in range(PER_STEPS):
        s0 = _PerState(ag)
        beta = ag.per_beta()
        assert abs(beta - (0.4 + 0.6 * k / PER_STEPS)) < 1e-12
        idx, w, taus = (x.clone() for x in m.priority.sample(m.size, PER_BATCH, beta))      # the batch all three steps take
        st = _read_back(m.priority)
        ti, tw, _ = T.sample(st, m.size, PER_BATCH, beta, int(s0.p[3][0]), int(s0.p[3][1]))
        assert idx.cpu().tolist() == ti.tolist()
        repeats += PER_BATCH - len(set(ti.tolist()))
        exp = tuple(t[idx] for t in ring)
        s0.restore()
        ref = _f64_weighted(ag, exp, taus[0], taus[1], w)
        res = {}
        for which in ("eager", "fused"):      # fused last: the run continues from its result
            s0.restore()
            ag.use_fused_train = which == "fused"
            loss = ag.train_from_memory()
            after = _read_back(m.priority)
            _sums_are_exact(after)
            res[which] = _result(ag, loss, torch.zeros(1))
        ag.use_fused_train = True
        rows = []
        try:
            H.compare_step(ref, res["fused"], res["eager"], f"per_step_{k}", rows)
        finally:
            print("\n".join(rows))
        d = ag._fused._absdelta[PER_BATCH].cpu().numpy()      # the fused step's priorities: its rows' new masses are their float64 masses, the update's bar
        m64 = T.new_mass_f64(d, 0.6, 1e-6)
        for r, j in {int(r): j for j, r in enumerate(ti)}.items():      # (the highest slot of every row)
            assert abs(int(after.mass[r]) - int(m64[j])) <= 1 + 1e-5 * int(m64[j]), (k, r, int(after.mass[r]), int(m64[j]))
        assert ag._per_step == k + 1 and ag.grad_steps == k + 1 and int(m.priority.rng_state[1]) == k + 1
    assert ag.per_beta() == 1.0 and int(m.priority.mmax[0]) > T.MASS_ONE
    print(f"repeated rows over {PER_STEPS} batches: {repeats}")


def test_a_fresh_process_resumes_prioritized_steps_bit_for_bit(torch, tmp_path):
    ag = _per_agent(torch)
    loss = None
    for k in range(PER_STEPS):
        if k == 8:
            torch.save(dict(agent=ag.state_dict(), ring=ag.memory.state_dict()), tmp_path / "state.pt")
        loss = ag.train_from_memory()
    straight = _per_bits(ag, loss)
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "per_resume_child.py"), str(tmp_path / "state.pt"), str(PER_STEPS - 8), str(tmp_path / "out.pt")],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-3000:]
    resumed = torch.load(tmp_path / "out.pt")
    for k, v in straight.items():
        assert torch.equal(v, resumed[k]), k


# ---- the whole trainer with --per: stop, resume in a fresh process, compare with the uninterrupted run ---------------------------------------------
import test_resume_gpu as RG      # noqa: E402  (its toy runs, its child-process launcher and its byte-for-byte file comparison)

PER_ARGS = ["--per", "--per-alpha", "0.5", "--per-beta0", "0.3"]      # (away from the defaults: the values must travel)
TRAINER_CASES = {
    # learner budget: 60 vector steps of 64 envs, one batch-32 gradient step behind each -> beta runs over 60 steps
    "learner": (dict(RG.LEARNER, args=RG.LEARNER["args"] + PER_ARGS), 60),
    # reference budget at toy size: learning from vector step 10 on, 4 gradient steps behind each of the 50 that learn -> beta runs over 200 steps
    "reference": (dict(RG.REFERENCE, args=RG.REFERENCE["args"] + ["--reference", "learning_starts=160", "target_update_interval=160", "exploration_fraction=0.8",
                                                                  "replay=4096"] + PER_ARGS), 200),
}


@pytest.mark.parametrize("name", list(TRAINER_CASES))
def test_trainer_with_per_stopped_and_resumed_writes_the_files_of_the_straight_run(torch, tmp_path, name):
    case, beta_steps = TRAINER_CASES[name]
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    seed_a, seed_b = (os.path.join(d, "runs", "training_toy", "seed_3") for d in (a, b))
    RG._train(a, case, "--dump-final-state", "final.pt")                                  # A: straight through
    out = RG._train(b, case, "--stop-after", str(RG.STOP))                                # B: stopped behind step 30
    assert f"stopped after vector step {RG.STOP} of {case['vector_steps']}" in out
    ck = torch.load(os.path.join(seed_b, "checkpoint.pt"), map_location="cpu", weights_only=False)
    assert ck["args"]["per"] == dict(alpha=0.5, beta0=0.3)
    pr, ag = ck["ring"]["priority"], ck["agent"]["per"]
    size = int(ck["ring"]["size"])
    assert pr["mass"].shape == (size,) and bool((pr["mass"] > 0).all()) and int(pr["mmax"]) >= T.MASS_ONE
    assert ag["beta_steps"] == beta_steps and ag["step"] == int(ck["agent"]["counters"]["grad_steps"]) > 0 and int(pr["rng_state"][1]) == ag["step"]
    assert bool((pr["mass"] != T.MASS_ONE).any())      # priorities moved before the stop
    # a resume that leaves --per out is another run: refused, and the key is named
    cmd = [sys.executable, "-m", "distributional_rl_navigation_amd.train_iqn", "-C", "config.json", "-D", DEV, "--run-name", "toy",
           *[x for x in case["args"] if x not in PER_ARGS], *RG.COMMON, "--resume", os.path.join("runs", "training_toy")]
    r = subprocess.run(cmd, cwd=b, env=dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", "")), capture_output=True, text=True, timeout=240)
    assert r.returncode != 0 and "other arguments: per was" in r.stderr, r.stderr[-1500:]
    out = RG._train(b, case, "--resume", os.path.join("runs", "training_toy"), "--dump-final-state", "final.pt")      # C: a fresh process continues B's directory
    assert f"continuing from vector step {RG.STOP} (checkpoint.pt)" in out
    files_a = sorted(os.listdir(seed_a))
    assert {"completed.json", "network_params.pth", "greedy_evaluations.npz", "trial_config.json"} <= set(files_a)
    assert sorted(set(os.listdir(seed_b)) - {"checkpoint.pt", "checkpoint.prev.pt"}) == files_a
    for f in files_a:
        RG._same_file(os.path.join(seed_a, f), os.path.join(seed_b, f), f)
    RG._same_file(os.path.join(a, "final.pt"), os.path.join(b, "final.pt"), "final.pt")      # agent, ring (masses, mmax, generator state) and env behind the last step
    final = torch.load(os.path.join(a, "final.pt"), map_location="cpu", weights_only=False)
    assert final["agent"]["per"]["step"] == beta_steps == int(final["agent"]["counters"]["grad_steps"])      # beta reached 1 with the last gradient step
