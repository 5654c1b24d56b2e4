"""Prioritized replay without a GPU: the symbols, the twin of the priority store (tests/per_twin.py) against a brute-force restatement -- one plain
cumulative sum over all rows in Python ints --, the empirical frequencies of its draws, the CPU path of iqn/priority.py against the twin, the weighted
loss of IQNAgent.compute_loss, and an agent that trains with priorities on the CPU, stopped and resumed.  At the ring sizes training uses (64 to 1 024
blocks) the brute force is one uint64 cumulative sum (per_twin.rows_by_cumsum), and the draws are shown to reach the far blocks.  (The kernels against the
twin: tests/test_per_gpu.py, and tests/test_per_scale_gpu.py at these sizes.)"""
import ctypes
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import per_twin as T      # noqa: E402
import rng_twin as R      # noqa: E402

SEED = 0x1234ABCD5678


# ---- symbols -----------------------------------------------------------------------------------------------------------------------------------
def test_symbols_are_declared_and_bound():
    from distributional_rl_navigation_amd import _capi
    bound = {s[0]: s for s in _capi.SIGNATURES}
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "marinenav_hip.h")).read()
    assert "Prioritized replay" in header
    for name, n_args in (("mn_per_append", 7), ("mn_per_sample", 11), ("mn_per_update", 10), ("mn_iqn_train_grad_per", 19)):
        assert name + "(" in header, name
        assert name in bound and len(bound[name][2]) == n_args, name
    if not os.path.exists(_capi.LIB_PATH):
        _capi.build()
    lib = ctypes.CDLL(_capi.LIB_PATH)
    for name in ("mn_per_append", "mn_per_sample", "mn_per_update", "mn_iqn_train_grad_per"):
        assert hasattr(lib, name), name
    assert (_capi.PER_MASS_ONE, _capi.PER_BLOCK, _capi.PER_MAX_CAPACITY, _capi.PER_MAX_BATCH) == (T.MASS_ONE, T.BLOCK, T.MAX_CAPACITY, 1024)


# ---- the twin against brute force ------------------------------------------------------------------------------------------------------------
def brute_rows(mass, batch, seed, ctr):
    """The rule restated without blocks: one cumulative sum over all rows, Python ints."""
    mass = [int(m) for m in mass]
    total = sum(mass)
    q = total // batch
    base = int(R.sample_base(seed, ctr))
    rows = []
    for k in range(batch):
        x = int(R.mix64(base ^ ((0x8CB92BA72F3D8DD7 * (k + 1)) & ((1 << 64) - 1))))
        u = x >> 40
        target = k * q + (((u << 40) * q) >> 64)
        assert k * q <= target < (k + 1) * q
        run = 0
        for i, m in enumerate(mass):
            run += m
            if run > target:
                rows.append(i)
                break
    return rows


hand_made = T.hand_made


CASES = [("equal", 2053, 16), ("equal", 1024, 32), ("equal", 1024, 256), ("one_heavy", 2053, 32), ("one_heavy", 700, 16), ("holes", 2053, 32), ("holes", 700, 2),
         ("random", 700, 32), ("random", 1025, 256), ("random", 2053, 256),
         ("equal", 700, 16), ("random", 256, 256), ("equal", 32, 32)]      # a single partial block; size = B


@pytest.mark.parametrize("name,size,batch", CASES)
def test_twin_equals_brute_force(name, size, batch):
    st = hand_made(name, size)
    assert [int(b) for b in st.bsum] == [sum(int(x) for x in st.mass[i:i + 1024]) for i in range(0, st.capacity, 1024)]
    for ctr in range(3):
        idx, w, taus = T.sample(st, size, batch, 0.4, SEED, ctr)
        want = brute_rows(st.mass, batch, SEED, ctr)
        assert idx.tolist() == want, (name, size, batch, ctr)
        assert (st.mass[idx] > 0).all() and int(idx.max()) < size
        assert w.dtype == np.float32 and w.max() == 1.0 and (w > 0).all()
        np.testing.assert_allclose(w, T.weights_f64(st.mass[idx], size, st.total, 0.4), rtol=1e-5)
        assert np.array_equal(taus.reshape(-1), R.sample_taus(R.sample_base(SEED, ctr), 2 * batch * 8))
    if name == "one_heavy":
        assert len(set(idx.tolist())) < batch      # the heavy row spans several strata
    if name == "equal" and (size * T.MASS_ONE) % batch == 0:      # stratum k starts exactly at a row boundary
        q = size * T.MASS_ONE // batch
        assert all(i >= (k * q) // T.MASS_ONE for k, i in enumerate(idx.tolist()))


def test_target_on_a_row_boundary_takes_the_next_row():
    st = T.Store(8)
    st.set_masses([5, 0, 7, 0, 0, 2])
    assert [T.find_row(st, t) for t in (0, 4, 5, 11, 12, 13)] == [0, 0, 2, 2, 5, 5]


def test_frequencies_follow_the_masses():
    g = np.random.default_rng(11)
    mass = g.integers(1, 40, 50).astype(np.uint32) * 1000
    st = T.Store(50)
    st.set_masses(mass)
    batch, calls = 20, 10_000      # 200 000 draws
    counts = np.zeros(50)
    for ctr in range(calls):
        for i in T.sample(st, 50, batch, 0.4, 99, ctr)[0]:
            counts[i] += 1
    n = batch * calls
    p = mass / mass.sum()
    sigma = np.sqrt(n * p * (1 - p))      # (stratification only lowers the variance of a row's count below the multinomial's)
    assert (np.abs(counts - n * p) <= 4 * sigma).all(), np.abs(counts - n * p) / sigma


# ---- the CPU store against the twin ----------------------------------------------------------------------------------------------------------
def _same_store(ps, st):
    assert np.array_equal(ps.mass.numpy().view(np.uint32), st.mass)
    assert np.array_equal(ps.bsum.numpy().view(np.uint64), st.bsum)
    assert int(ps.mmax[0]) == st.mmax


def test_cpu_store_equals_the_twin_interleaved():
    from distributional_rl_navigation_amd.iqn.priority import PriorityStore
    cap, batch = 2053, 16
    ps, st = PriorityStore(cap, "cpu", SEED), T.Store(cap)
    g = np.random.default_rng(3)
    ptr = size = ctr = 0
    for it in range(40):
        n = int(g.integers(1, 300))
        ps.append(ptr, n); T.append(st, ptr, n)
        ptr, size = (ptr + n) % cap, min(cap, size + n)
        _same_store(ps, st)
        if size >= batch:
            idx, w, taus = ps.sample(size, batch, 0.5)
            ti, tw, tt = T.sample(st, size, batch, 0.5, SEED, ctr)
            ctr += 1
            assert idx.tolist() == ti.tolist() and np.array_equal(w.numpy(), tw) and np.array_equal(taus.numpy(), tt)
            np.testing.assert_allclose(w.numpy(), T.weights_f64(st.mass[ti], size, st.total, 0.5), rtol=1e-5)      # (the twin's float32 weights are the same numpy expression: float64 is the independent yardstick)
            d = torch.from_numpy((g.random(batch) * 10 ** g.uniform(-4, 2, batch)).astype(np.float32))
            ps.update(idx, d, 0.6, 1e-6)
            T.update(st, ti, T.new_mass_f32(d.numpy(), 0.6, 1e-6))
            _same_store(ps, st)
    assert size == cap and it * 150 > cap      # the ring wrapped
    assert st.mmax > T.MASS_ONE and int(ps.rng_state[1]) == ctr


# ---- rings of the sizes training uses: 64 to 1 024 blocks -----------------------------------------------------------------------------------
LARGE_BATCHES = (2, 256, 1024)
_large_samples = {}


def _twin_large(name, capacity, size):
    """The twin's draws of one vector at one place of the grid -- {(batch, ctr): (idx, w, taus)} --, drawn once for the tests below."""
    key = (name, capacity, size)
    if key not in _large_samples:
        out = {}
        for batch in LARGE_BATCHES:
            st, n = T.large_case(name, capacity, size, batch)
            for ctr in range(3):
                out[batch, ctr] = T.sample(st, n, batch, 0.4, SEED, ctr)
        _large_samples[key] = out
    return _large_samples[key]


def _inputs_exercise_the_code(name, capacity, size, batch, idx):
    """What a case is there for, asserted on the twin's rows: a case that stops reaching the code it was made for fails here."""
    blocks = idx // T.BLOCK
    full = name != "young" and size == capacity
    # holes_wide keeps blocks 64..127 empty and gives the last row mass 3: up to 131 072 rows it has three units of mass beyond row 65 535, no seed changes that
    if full and capacity > 65_536 and batch >= 256 and not (name == "holes_wide" and size <= 128 * T.BLOCK):
        assert int(idx.max()) >= 65_536, (name, capacity, batch)      # beyond the first wavefront's 64 block sums
    if capacity == T.MAX_CAPACITY and batch == 1024 and name in ("random", "saturated", "holes_wide"):
        assert int(blocks.max()) == 1023, (name, int(blocks.max()))
    if name == "holes_wide":
        assert not ((blocks >= 64) & (blocks < 128)).any() and int(idx.min()) >= 1024
        if size > 128 * T.BLOCK and batch >= 256:
            assert (blocks < 64).any() and (blocks >= 128).any()      # rows on both sides of the empty wavefront
    if name == "heavy_far" and batch >= 256:
        assert len(set(idx.tolist())) < batch
        if size > 65_536:
            heavy = np.bincount(idx).argmax()
            assert heavy >= 65_536 and (idx == heavy).sum() > 1      # the repeats lie beyond block 63
    if name == "young":
        assert sorted(idx.tolist()) == list(range(batch))      # every stratum is one row


@pytest.mark.parametrize("name", T.LARGE_VECTORS)
@pytest.mark.parametrize("capacity,size", T.LARGE_GRID)
def test_twin_equals_one_cumulative_sum_at_scale(capacity, size, name):
    draws = _twin_large(name, capacity, size)
    for batch in LARGE_BATCHES:
        st, n = T.large_case(name, capacity, size, batch)
        assert np.array_equal(st.bsum, T.block_sums(st.mass)) and st.total == int(st.mass.sum(dtype=np.uint64)) < 1 << 51
        for ctr in range(3):
            idx, w, taus = draws[batch, ctr]
            tg = T.targets(st.total, SEED, ctr, batch)
            q = st.total // batch
            assert all(k * q <= t < (k + 1) * q for k, t in enumerate(tg))
            assert idx.tolist() == T.rows_by_cumsum(st.mass, tg).tolist(), (name, capacity, size, batch, ctr)
            assert (st.mass[idx] > 0).all() and int(idx.max()) < n
            assert w.dtype == np.float32 and w.max() == 1.0 and (w > 0).all()
            np.testing.assert_allclose(w, T.weights_f64(st.mass[idx], n, st.total, 0.4), rtol=1e-5)
            assert np.array_equal(taus.reshape(-1), R.sample_taus(R.sample_base(SEED, ctr), 2 * batch * 8))
            _inputs_exercise_the_code(name, capacity, size, batch, idx)
        blocks = np.unique(np.concatenate([draws[batch, c][0] for c in range(3)]) // T.BLOCK)
        print(f"capacity {capacity} size {n} {name} batch {batch}: rows in {len(blocks)} distinct blocks, highest {int(blocks.max())}")


@pytest.mark.parametrize("name", T.LARGE_VECTORS)
@pytest.mark.parametrize("capacity,size", T.LARGE_GRID)
def test_cpu_store_equals_the_twin_at_scale(capacity, size, name):
    from distributional_rl_navigation_amd.iqn.priority import PriorityStore
    draws = _twin_large(name, capacity, size)
    ps = PriorityStore(capacity, "cpu", SEED)
    for batch in LARGE_BATCHES:
        st, n = T.large_case(name, capacity, size, batch)
        ps.mass.copy_(torch.from_numpy(st.mass.view(np.int32).copy()))
        ps.bsum.copy_(torch.from_numpy(st.bsum.view(np.int64).copy()))
        ps.rng_state[1] = 0
        for ctr in range(3):
            idx, w, taus = ps.sample(n, batch, 0.4)
            ti, tw, tt = draws[batch, ctr]
            assert idx.tolist() == ti.tolist(), (name, capacity, size, batch, ctr)
            assert np.array_equal(w.numpy(), tw) and np.array_equal(taus.numpy(), tt)
            assert ps.rng_state.tolist() == [SEED, ctr + 1]
        _same_store(ps, st)      # the sampler writes nothing


def test_cpu_store_equals_the_twin_interleaved_at_scale():
    """train_iqn --per's default ring: 98 blocks, 4 096 rows a vector step, batch 256."""
    from distributional_rl_navigation_amd.iqn.priority import PriorityStore
    cap, batch, n = 100_000, 256, 4096
    ps, st = PriorityStore(cap, "cpu", SEED), T.Store(cap)
    g = np.random.default_rng(3)
    ptr = size = ctr = 0
    beyond = 0
    for it in range(40):
        ps.append(ptr, n); T.append(st, ptr, n)
        ptr, size = (ptr + n) % cap, min(cap, size + n)
        _same_store(ps, st)
        idx, w, taus = ps.sample(size, batch, 0.5)
        ti, tw, tt = T.sample(st, size, batch, 0.5, SEED, ctr)
        ctr += 1
        assert idx.tolist() == ti.tolist() and np.array_equal(w.numpy(), tw) and np.array_equal(taus.numpy(), tt)
        assert ti.tolist() == T.rows_by_cumsum(st.mass, T.targets(st.total, SEED, ctr - 1, batch)).tolist()
        np.testing.assert_allclose(w.numpy(), T.weights_f64(st.mass[ti], size, st.total, 0.5), rtol=1e-5)
        beyond += int((ti >= 65_536).sum())
        d = torch.from_numpy((g.random(batch) * 10 ** g.uniform(-4, 2, batch)).astype(np.float32))
        ps.update(idx, d, 0.6, 1e-6)
        T.update(st, ti, T.new_mass_f32(d.numpy(), 0.6, 1e-6))
        _same_store(ps, st)
    assert size == cap and 40 * n > cap and ptr == 40 * n % cap      # the ring wrapped
    assert st.mmax > T.MASS_ONE and int(ps.rng_state[1]) == ctr and beyond > 0


def test_update_highest_slot_wins_and_clamps():
    from distributional_rl_navigation_amd.iqn.priority import PriorityStore
    ps = PriorityStore(10, "cpu", 0)
    ps.append(0, 10)
    idx = torch.tensor([4, 2, 4, 7, 4, 9], dtype=torch.int64)
    d = torch.tensor([1.0, 0.0, 2.0, 1e30, 0.25, float("nan")], dtype=torch.float32)
    ps.update(idx, d, 1.0, 0.0)
    m = ps.mass.tolist()
    assert m[4] == 16384 and m[2] == 1 and m[7] == T.MASS_MAX and m[9] == 1 and m[0] == T.MASS_ONE
    assert int(ps.bsum[0]) == sum(m) and int(ps.mmax[0]) == T.MASS_MAX
    assert T.new_mass_f32(d.numpy(), 1.0, 0.0).tolist() == [65536, 1, 131072, T.MASS_MAX, 16384, 1]
    assert T.new_mass_f64(d.numpy(), 1.0, 0.0).tolist() == [65536, 1, 131072, T.MASS_MAX, 16384, 1]


def test_capacity_beyond_2_to_20_is_refused():
    from distributional_rl_navigation_amd.iqn.priority import PriorityStore
    with pytest.raises(ValueError, match="2\\^20"):
        PriorityStore((1 << 20) + 1, "cpu", 0)
    assert PriorityStore(1_000_000, "cpu", 0).bsum.numel() == 977


def test_ring_appends_priorities_wherever_it_writes():
    from distributional_rl_navigation_amd.iqn.replay_buffer import ReplayBuffer
    g = torch.Generator().manual_seed(0)
    rows = lambda k: (torch.randn(k, 26, generator=g), torch.randint(0, 9, (k,), generator=g), torch.randn(k, generator=g), torch.randn(k, 26, generator=g),
                      torch.zeros(k))
    rb = ReplayBuffer(40, 8, "cpu", 3, 0.99, prioritized=True)
    rb.add_batch(*rows(30))
    assert rb.priority.mass.tolist() == [T.MASS_ONE] * 30 + [0] * 10
    rb.priority.update(torch.tensor([5]), torch.tensor([4.0]), 1.0, 0.0)
    rb.add_batch(*rows(15))      # across the wrap: rows 30..39 and 0..4 get the new largest mass
    m = rb.priority.mass.tolist()
    assert m[30:] == [4 * T.MASS_ONE] * 10 and m[:5] == [4 * T.MASS_ONE] * 5 and m[5] == 4 * T.MASS_ONE and m[6:30] == [T.MASS_ONE] * 24
    assert int(rb.priority.bsum[0]) == sum(m)
    rb3 = ReplayBuffer(40, 8, "cpu", 3, 0.99, n_step=3, prioritized=True)
    rb3.add_batch(*rows(4)); rb3.add_batch(*rows(4))
    assert int(rb3.priority.bsum.sum()) == 0      # the window is still filling: nothing was emitted
    rb3.add_batch(*rows(4))
    assert rb3.priority.mass.tolist() == [T.MASS_ONE] * 4 + [0] * 36
    assert ReplayBuffer(40, 8, "cpu", 3, 0.99).priority is None and "priority" not in ReplayBuffer(40, 8, "cpu", 3, 0.99).state_dict()


# ---- the weighted loss -----------------------------------------------------------------------------------------------------------------------
def _agent(seed, **kw):
    from distributional_rl_navigation_amd.iqn.agent import IQNAgent
    return IQNAgent(26, 9, BATCH_SIZE=8, BUFFER_SIZE=64, device="cpu", seed=seed, **kw)


def _rows(k, seed=0):
    g = torch.Generator().manual_seed(seed)
    s = torch.randn(k, 26, generator=g)
    return (s, torch.randint(0, 9, (k,), generator=g), torch.randn(k, generator=g), s + 0.1 * torch.randn(k, 26, generator=g),
            (torch.rand(k, generator=g) < 0.2).float())


def _batch(k, seed=0):
    s, a, r, ns, d = _rows(k, seed)
    return (s, a.view(k, 1), r.view(k, 1), ns, d.view(k, 1))


def test_weights_of_one_give_todays_loss_bit_for_bit():
    ag = _agent(1)
    exp = _batch(8)
    g = torch.Generator().manual_seed(5)
    tt, tl = torch.rand(8, 8, generator=g), torch.rand(8, 8, generator=g)
    plain = ag.compute_loss(exp, tt, tl)
    ones, abs_td = ag.compute_loss(exp, tt, tl, weights=torch.ones(8), want_abs_td=True)
    assert torch.equal(plain, ones) and abs_td.shape == (8,) and not abs_td.requires_grad and bool((abs_td > 0).all())
    gp = torch.autograd.grad(plain, list(ag.qnetwork_local.parameters()))
    go = torch.autograd.grad(ones, list(ag.qnetwork_local.parameters()))
    assert all(torch.equal(x, y) for x, y in zip(gp, go))


def test_weighted_loss_is_the_weighted_sum_of_the_element_losses():
    ag = _agent(1)
    exp = _batch(8)
    g = torch.Generator().manual_seed(5)
    tt, tl = torch.rand(8, 8, generator=g), torch.rand(8, 8, generator=g)
    w = torch.rand(8, generator=g)
    w[3] = 0.0
    per_element = torch.stack([ag.compute_loss(tuple(t[b:b + 1] for t in exp), tt[b:b + 1], tl[b:b + 1]) for b in range(8)])      # each a mean over ONE element
    want = float((per_element.detach().double() * w.double()).sum() / 8)
    got = float(ag.compute_loss(exp, tt, tl, weights=w).detach())
    assert abs(got - want) <= 8 * 2.0 ** -24 * float((per_element.detach().double().abs() * w.double()).sum() / 8)      # 8 roundings' worth of a float32 sum of these terms


# ---- an agent with priorities, stopped and resumed -----------------------------------------------------------------------------------------
def _train(ag, k):
    loss = None
    for _ in range(k):
        loss = ag.train_from_memory()
        if ag.grad_steps % 4 == 0:
            ag._sync_target()
    return loss


def _bits(ag, loss):
    m, v, step = ag._adam_state()
    flat = lambda ps: torch.cat([p.detach().reshape(-1) for p in ps])
    pr = ag.memory.priority
    return dict(local=flat(ag.qnetwork_local.parameters()), exp_avg=m, exp_avg_sq=v, loss=loss, mass=pr.mass.clone(), bsum=pr.bsum.clone(), mmax=pr.mmax.clone(),
                rng=pr.rng_state.clone(), step=step, per_step=ag._per_step)


def test_per_agent_trains_on_the_cpu_and_resumes_bit_for_bit():
    rows = _rows(48, seed=3)
    mk = lambda seed: _agent(seed, per=True)
    a = mk(0)
    a.per_beta_steps = 12
    a.memory.add_batch(*rows)
    assert a.per_beta() == pytest.approx(0.4)
    straight = _bits(a, _train(a, 12))
    assert a.per_beta() == pytest.approx(1.0) and straight["per_step"] == 12 and int(straight["rng"][1]) == 12
    assert int(straight["mmax"]) != T.MASS_ONE or bool((straight["mass"][:48] != T.MASS_ONE).any())      # priorities moved
    assert int(straight["bsum"].sum()) == int(straight["mass"].to(torch.int64).sum())

    b = mk(0)
    b.per_beta_steps = 12
    b.memory.add_batch(*rows)
    _train(b, 5)
    agent_sd, ring_sd = b.state_dict(), b.memory.state_dict()
    c = mk(1234)
    c.memory.load_state_dict(ring_sd)
    c.load_state_dict(agent_sd)
    resumed = _bits(c, _train(c, 7))
    for k, v in straight.items():
        assert torch.equal(v, resumed[k]) if torch.is_tensor(v) else v == resumed[k], k


def test_state_saved_without_priorities_loads_as_uniform():
    rows = _rows(48, seed=3)
    u = _agent(0)
    u.memory.add_batch(*rows)
    _train(u, 2)
    p = _agent(0, per=True)
    p.memory.load_state_dict(u.memory.state_dict())
    p.load_state_dict(u.state_dict())
    assert p.memory.priority.mass.tolist() == [T.MASS_ONE] * 48 + [0] * 16 and int(p.memory.priority.bsum[0]) == 48 * T.MASS_ONE
    assert p._per_step == 0
    _train(p, 1)
    # and the other way round: a uniform agent reads a prioritized state's ring and networks
    u2 = _agent(0)
    u2.memory.load_state_dict(p.memory.state_dict())
    u2.load_state_dict(p.state_dict())


def test_refusals(tmp_path):
    from distributional_rl_navigation_amd import train_iqn
    with pytest.raises(ValueError, match="shared learner"):
        _agent(0, per=True, distributed=True)
    ag = _agent(0, per=True)
    ag.use_fused_graph = True
    with pytest.raises(ValueError, match="use_fused_graph"):
        ag.train_steps_from_memory(2)
    with pytest.raises(ValueError, match="--together"):
        train_iqn.run_trials_together("cpu", [dict(seed=0, total_timesteps=100, eval_freq=50, save_dir="x")], 4, per=dict(alpha=0.6, beta0=0.4))
    cfg = tmp_path / "config.json"
    cfg.write_text(json.dumps(dict(agent="IQN", seed=[3, 4], total_timesteps=4000, eval_freq=400, save_dir=str(tmp_path / "runs"))))
    for extra, word in ((["--together"], "--together"), (["--stack-envs", "--together"], "--together"), (["--shared-learner"], "shared learner")):
        with pytest.raises(SystemExit, match=word):
            train_iqn.main(["-C", str(cfg), "--per", "--dry-run"] + extra)
    train_iqn.main(["-C", str(cfg), "--per", "--per-alpha", "0.5", "--dry-run"])      # alone it is accepted
    assert train_iqn.run_shaping_args() == {k: v for k, v in train_iqn.run_shaping_args(per=None).items()} and "per" not in train_iqn.run_shaping_args()
    assert train_iqn.run_shaping_args(per=dict(alpha=0.6, beta0=0.4))["per"] == dict(alpha=0.6, beta0=0.4)


def test_resume_with_or_without_per_against_the_checkpoint_is_refused():
    from distributional_rl_navigation_amd.train_iqn import check_resumable, run_shaping_args
    per = dict(alpha=0.6, beta0=0.4)
    shape = dict(n_envs=16, batch=32)
    with_per, without = run_shaping_args(per=per), run_shaping_args()
    check_resumable(dict(plan=shape, args=with_per), shape, run_shaping_args(per=dict(per)))
    check_resumable(dict(plan=shape, args=without), shape, run_shaping_args())      # (a checkpoint from before there were priorities has no such key either)
    for saved, now in ((with_per, without), (without, with_per), (with_per, run_shaping_args(per=dict(per, alpha=0.5)))):
        with pytest.raises(ValueError, match="other arguments: per was"):
            check_resumable(dict(plan=shape, args=saved), shape, now)
