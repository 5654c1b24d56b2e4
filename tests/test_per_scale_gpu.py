"""Prioritized replay on the device at the ring sizes training uses (csrc/per.hip, the gather of the weighted step in csrc/iqn_train.hip): 64 to 1 024 block
sums, so that the sampler's scan crosses wavefronts and its binary search runs over whole wavefronts of empty blocks; batches up to the 1 024 the ABI admits;
appends long enough for the append kernel's grid-stride loop; totals just under 2^51.  The yardstick is the host twin (tests/per_twin.py), which
tests/test_per_cpu.py holds to one cumulative sum over all rows at these very sizes and whose draws it shows to reach the far blocks.  tests/test_per_gpu.py
has the same checks on a ring of three blocks; its helpers are used here.  Only the two tolerances of that file appear: 1e-5 relative for the weights against
float64, 1 + 1e-5 m for an updated mass; everything else is equality of integers or bits."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import iqn_train_f64 as H      # noqa: E402
import per_twin as T           # noqa: E402
import test_per_gpu as PG      # noqa: E402

pytestmark = pytest.mark.gpu
DEV, SEED = PG.DEV, PG.SEED
torch = PG.torch      # the fixture: skips without a GPU
_read_back, _sums_are_exact = PG._read_back, PG._sums_are_exact


def _load(torch, ps, twin):
    ps.mass.copy_(torch.from_numpy(twin.mass.view(np.int32).copy()))
    ps.bsum.copy_(torch.from_numpy(twin.bsum.view(np.int64).copy()))
    ps.mmax.fill_(int(twin.mmax))


def _store(torch, capacity, twin=None):
    from distributional_rl_navigation_amd.iqn.priority import PriorityStore
    ps = PriorityStore(capacity, DEV, SEED)
    if twin is not None:
        _load(torch, ps, twin)
    return ps


def _same_store(ps, st, what):
    got = _read_back(ps)
    assert np.array_equal(got.mass, st.mass), what
    assert np.array_equal(got.bsum, st.bsum), what
    assert got.mmax == st.mmax, what
    return got


# ---- the sampler ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("capacity,size", T.LARGE_GRID)
def test_sampler_rows_equal_the_twin_at_scale(torch, capacity, size):
    ps = _store(torch, capacity)
    ctr, worst = 0, 0.0
    for name in T.LARGE_VECTORS:
        for batch in (2, 256, 512, 1024):
            if name == "young" or batch == 2:
                twin, n = T.large_case(name, capacity, size, batch)
                _load(torch, ps, twin)
                st = _read_back(ps)
                assert np.array_equal(st.mass, twin.mass)
            for beta in (0.4, 1.0):
                idx, w, taus = (x.cpu().numpy() for x in ps.sample(n, batch, beta))
                ti, tw, tt = T.sample(st, n, batch, beta, SEED, ctr)
                ctr += 1
                assert idx.tolist() == ti.tolist(), (name, batch, beta)
                assert int(idx.max()) < n and (st.mass[idx] > 0).all()
                w64 = T.weights_f64(st.mass[ti], n, st.total, beta)
                rel = np.abs(w - w64) / w64
                worst = max(worst, float(rel.max()))
                blocks = np.unique(ti // T.BLOCK)
                print(f"capacity {capacity} size {n} {name} batch {batch} beta {beta}: weights max rel err {rel.max():.3e}, rows in {len(blocks)} blocks, "
                      f"highest {int(blocks.max())}")
                assert rel.max() <= 1e-5 and w.max() == 1.0
                assert np.array_equal(taus, tt)
            if name == "heavy_far" and batch >= 256:
                assert len(set(idx.tolist())) < batch
            if name == "young" or batch == 1024:
                _same_store(ps, twin, name)      # the sampler writes nothing
                _sums_are_exact(_read_back(ps))
    assert ps.rng_state.cpu().tolist() == [SEED, ctr]
    print(f"capacity {capacity} size {size}: largest weight error over the vectors {worst:.3e}")


# ---- append ------------------------------------------------------------------------------------------------------------------------------------
def test_append_at_scale_train_ring(torch):
    """train_iqn --per's default ring: a first call of 37 rows, so that every later wavefront straddles a block boundary somewhere and no `ptr` is a multiple
    of 64; then calls of 4 096 and 65 536 rows across the wrap, the largest mass moving in between."""
    cap = 100_000
    ps, st = _store(torch, cap), T.Store(cap)
    ptr = 0
    for call, n in enumerate((37, 4096, 65_536, 4096, 65_536, 4096)):
        ps.append(ptr, n)
        T.append(st, ptr, n)
        ptr = (ptr + n) % cap
        _same_store(ps, st, (call, n))
        if call == 2:      # a new largest mass: later rows enter with it, over rows that hold the old one
            rows = torch.tensor([5, 66_000], dtype=torch.int64, device=DEV)
            ps.update(rows, torch.tensor([3.0, 0.5], device=DEV), 1.0, 0.0)
            T.update(st, [5, 66_000], [3 * T.MASS_ONE, T.MASS_ONE // 2])
            _same_store(ps, st, "update")
    assert ptr == (37 + 3 * 4096 + 2 * 65_536) % cap and ptr % 64 and 37 + 3 * 4096 + 2 * 65_536 > cap
    assert st.mmax == 3 * T.MASS_ONE and (st.mass == 3 * T.MASS_ONE).sum() > 65_536 and (st.mass == T.MASS_ONE).sum() > 0


def test_append_at_scale_grid_stride_and_whole_ring(torch):
    """2^20 rows: more rows in one call than the launch has threads (1 024 x 256), across the wrap, over masses that all differ; then the whole ring in one
    call from a `ptr` inside it."""
    cap = T.MAX_CAPACITY
    st = T.hand_made_large("random", cap, cap)
    ps = _store(torch, cap, st)
    ps.append(900_001, 300_000)
    T.append(st, 900_001, 300_000)
    got = _same_store(ps, st, "300 000 rows from 900 001")
    assert 300_000 > 1024 * 256 and 900_001 + 300_000 > cap
    _sums_are_exact(got)
    rows = torch.tensor([7, 500_000], dtype=torch.int64, device=DEV)
    ps.update(rows, torch.tensor([5.0, 0.25], device=DEV), 1.0, 0.0)
    T.update(st, [7, 500_000], [5 * T.MASS_ONE, T.MASS_ONE // 4])
    _same_store(ps, st, "update")
    ptr = (900_001 + 300_000) % cap
    ps.append(ptr, cap)
    T.append(st, ptr, cap)
    got = _same_store(ps, st, "the whole ring")
    assert ptr > 0 and (got.mass == 5 * T.MASS_ONE).all() and int(got.bsum[-1]) == 1024 * 5 * T.MASS_ONE


# ---- update ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch", [512, 1024])
def test_update_at_scale(torch, batch):
    cap = 100_000
    FIVE, PAIR = 99_000, 70_001
    ps = _store(torch, cap, T.hand_made_large("random", cap, cap))
    st = _read_back(ps)
    g = np.random.default_rng(batch)
    idx = g.permutation(np.setdiff1d(np.arange(cap), [FIVE, PAIR]))[:batch]      # distinct rows of the whole ring, then the repeats
    five = np.linspace(3, batch - 2, 5).astype(np.int64)      # one row five times, its slots spread over the batch: slot batch - 2 wins
    idx[five] = FIVE
    idx[[10, 11]] = PAIR      # a pair in adjacent slots
    d = (g.random(batch) * 10 ** g.uniform(-5, 3, batch)).astype(np.float32)
    d[five] = [0.1, 0.2, 0.3, 0.4, 7.0]
    d[10], d[11] = 2.0, 0.05
    d[0], d[2], d[5] = 0.0, 1e30, float("nan")      # the clamps -- mass 1 and 2^31 - 1 -- and a NaN
    assert len(set(idx.tolist())) == batch - 5 and int(idx.max()) >= 65_536 and len(np.unique(idx // T.BLOCK)) > 64
    ps.update(torch.from_numpy(idx).to(DEV), torch.from_numpy(d).to(DEV), 0.6, 1e-6)
    got = _read_back(ps)
    _sums_are_exact(got)
    m64 = T.new_mass_f64(d, 0.6, 1e-6)
    winners = {int(r): k for k, r in enumerate(idx)}      # the highest slot of every row
    assert winners[FIVE] == batch - 2 and winners[PAIR] == 11
    for r, k in winners.items():
        assert abs(int(got.mass[r]) - int(m64[k])) <= 1 + 1e-5 * int(m64[k]), (r, k, int(got.mass[r]), int(m64[k]))
    for k in list(five[:-1]) + [10]:      # a losing slot's mass is far from its row's
        assert abs(int(m64[k]) - int(got.mass[idx[k]])) > 1000
    untouched = np.setdiff1d(np.arange(cap), idx)
    assert np.array_equal(got.mass[untouched], st.mass[untouched])
    assert got.mmax == max(st.mmax, max(int(got.mass[r]) for r in winners)) == T.MASS_MAX
    assert got.mass[idx[0]] == 16 and got.mass[idx[2]] == T.MASS_MAX and got.mass[idx[5]] == 1      # (1e-6 ** 0.6 * 65536 = 16.46)
    ps.update(torch.from_numpy(idx[:2].copy()).to(DEV), torch.tensor([0.0, float("nan")], device=DEV), 1.0, 0.0)      # the lower clamp with eps 0
    low = _read_back(ps)
    _sums_are_exact(low)
    assert low.mass[idx[0]] == 1 and low.mass[idx[1]] == 1 and low.mmax == T.MASS_MAX


# ---- a store's lifetime --------------------------------------------------------------------------------------------------------------------------
def test_forty_rounds_of_append_sample_update(torch):
    """train_iqn --per's default ring and vector step: append 4 096, sample 256, update; the store is read back behind every operation."""
    cap, batch, n, rounds = 100_000, 256, 4096, 40
    ps, st = _store(torch, cap), T.Store(cap)
    g = np.random.default_rng(5)
    ptr = size = 0
    beyond = 0
    for it in range(rounds):
        ps.append(ptr, n)
        T.append(st, ptr, n)
        ptr, size = (ptr + n) % cap, min(cap, size + n)
        _sums_are_exact(_same_store(ps, st, ("append", it)))
        beta = 0.4 + 0.6 * it / (rounds - 1)
        idx, w, taus = (x.clone() for x in ps.sample(size, batch, beta))
        got = _same_store(ps, st, ("sample", it))
        ti, tw, tt = T.sample(got, size, batch, beta, SEED, it)
        assert idx.cpu().tolist() == ti.tolist(), it
        w64 = T.weights_f64(got.mass[ti], size, got.total, beta)
        wn = w.cpu().numpy()
        assert (np.abs(wn - w64) / w64).max() <= 1e-5 and wn.max() == 1.0 and np.array_equal(taus.cpu().numpy(), tt)
        beyond += int((ti >= 65_536).sum())
        d = (g.random(batch) * 10 ** g.uniform(-4, 2, batch)).astype(np.float32)
        ps.update(idx, torch.from_numpy(d).to(DEV), 0.6, 1e-6)
        after = _read_back(ps)
        _sums_are_exact(after)
        m64 = T.new_mass_f64(d, 0.6, 1e-6)
        winners = {int(r): k for k, r in enumerate(ti)}
        for r, k in winners.items():
            assert abs(int(after.mass[r]) - int(m64[k])) <= 1 + 1e-5 * int(m64[k]), (it, r, k, int(after.mass[r]), int(m64[k]))
        untouched = np.setdiff1d(np.arange(cap), ti)
        assert np.array_equal(after.mass[untouched], st.mass[untouched])
        assert after.mmax == max(st.mmax, max(int(after.mass[r]) for r in winners))
        st = after      # powf is not pinned to bits: the twin goes on from the device's masses
    assert ps.rng_state.cpu().tolist() == [SEED, rounds] and beta == 1.0
    assert size == cap and rounds * n > cap and ptr == rounds * n % cap      # the ring wrapped
    assert st.mmax > T.MASS_ONE and beyond > 0


# ---- the weighted step gathers from a large ring -------------------------------------------------------------------------------------------------
def test_weighted_step_from_a_large_ring_equals_the_gathered_batch_bit_for_bit(torch):
    cap, B = 100_000, 256
    c = H.build_case("random", B)
    ag = PG._agent(torch, c)
    ring = tuple(t.to(DEV).contiguous() for t in H.random_batch(cap, torch.Generator().manual_seed(21)))
    ps = _store(torch, cap, T.hand_made_large("random", cap, cap))
    idx, w, taus = (x.clone() for x in ps.sample(cap, B, 0.7))
    rows = idx.cpu().numpy()
    assert int(rows.max()) >= 65_536 and int(rows.max()) < cap and not np.array_equal(rows, np.arange(B))
    tt, tl = taus[0].contiguous(), taus[1].contiguous()
    state = PG._State(ag)
    ft = ag._fused_trainer()
    ag._enter_train_path("hip")
    loss, abs_td = ft.step_per(ring, idx, tt, tl, w)
    far = PG._result(ag, loss, abs_td)
    state.restore()
    near = PG._fused_weighted(torch, ag, tuple(t[idx].contiguous() for t in ring), tt, tl, w)
    for k in ("grad", "params", "m", "v", "abs_td"):
        assert np.array_equal(getattr(far, k), getattr(near, k)), k
    assert far.loss == near.loss and far.t == near.t == 1
    assert np.isfinite(far.loss) and (far.abs_td > 0).all() and np.abs(far.grad).max() > 0
