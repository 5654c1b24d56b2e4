"""What the streams of tests/rng_twin.py -- the host twin of the kernels' four counter-based generators -- must satisfy.  No GPU: the kernels are
held to the twin bit for bit in tests/test_rng_draws_gpu.py, so a property shown here for the twin is a property of the device draws.

Seeds are fixed, so every statistic below is ONE deterministic number, not a random test.  Counts are judged by Pearson's chi-square with its
degrees of freedom, one-sided ("too uniform" is not a failure); correlations by r sqrt(N), two-sided.  The bound of a test that takes the maximum
over m statistics is the upper-tail 1e-6 / m quantile of the statistic's own null distribution (`chi2_bound`, `z_bound`: scipy.stats if it imports,
else Wilson-Hilferty and an erfc bisection).  To compare groups with different degrees of freedom, the docstrings record the worst statistic of
each group as the |z| with the same tail probability (chi-square through Wilson-Hilferty); the bound of a single statistic is |z| = 4.75 one-sided
/ 4.89 two-sided.  Observed worst values are from this file's own run (`pytest -s` prints them).

The last tests plant six defects, built from the twin's own parts, and require the SAME statistics at the SAME bounds to reject each.  Observed: the
exploration uniform read at tau 0's index |z| = 64.0 (own_corr), row stride 31 |z| = 64.0 (row_corr), keys that ignore the counter chi-square 2.0e6
(call_pairs), one multiply for the hash 7.3e5 (serial), a one-round Feistel z >= 35 in all four replay statistics, an action that ignores the step
4.2e6 (pairs).

What the battery cannot see: it guards structure and indexing -- which index, which key, which counter reaches which draw -- and does not certify
the hash.  Dropping one of `u01`'s two fmix32 rounds, or one of its two keys, still passes every test here."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import rng_twin as T      # noqa: E402

P = 1e-6
SEEDS = (0, 123, 2**63 - 1, 2**64 - 1)
CTRS = (0, 1, 2**32 - 1, 2**32)
KEYS = [(s, c) for s in SEEDS for c in CTRS]
N = 4096


# ---- null distributions -------------------------------------------------------------------------------------------------------------------------
def _norm_isf(p):
    lo, hi = 0.0, 40.0
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if 0.5 * math.erfc(mid / math.sqrt(2.0)) > p else (lo, mid)
    return 0.5 * (lo + hi)


def z_bound(p, two_sided=True):
    return _norm_isf(p / 2 if two_sided else p)


def chi2_bound(df, p):
    try:
        from scipy.stats import chi2
        return float(chi2.isf(p, df))
    except ImportError:
        a = 2.0 / (9.0 * df)
        return df * (1.0 - a + _norm_isf(p) * math.sqrt(a)) ** 3


def chi2_z(x, df):
    """Wilson-Hilferty: the normal deviate with the tail probability of chi-square `x` at `df` degrees of freedom (for the recorded figures)."""
    a = 2.0 / (9.0 * df)
    return ((np.asarray(x, dtype=np.float64) / df) ** (1.0 / 3.0) - (1.0 - a)) / math.sqrt(a)


def chi2_counts(counts, expected):
    counts, expected = np.asarray(counts, dtype=np.float64), np.asarray(expected, dtype=np.float64)
    return float(((counts - expected) ** 2 / expected).sum())


def chi2_uniform(cells, n_cells):
    c = np.bincount(np.asarray(cells).ravel(), minlength=n_cells)
    return chi2_counts(c, np.full(n_cells, c.sum() / n_cells))


def corr_z(x, y):
    """r sqrt(N) of every column of x [N, a] against every column of y [N, b]: [a, b]."""
    x = x.astype(np.float64) - x.mean(0)
    y = y.astype(np.float64) - y.mean(0)
    r = (x.T @ y) / np.sqrt(np.outer((x * x).sum(0), (y * y).sum(0)))
    return r * math.sqrt(x.shape[0])


def _judge(name, stats, bound, df=None):
    """Print the group's worst statistic (as a normal deviate) and return whether it stays under the bound."""
    worst = float(np.max(np.abs(stats)))
    z = float(chi2_z(worst, df)) if df else worst
    print(f"{name}: m = {np.size(stats)}, worst = {worst:.2f} (|z| = {z:.2f}), bound = {bound:.2f}")
    return worst <= bound


# ---- the act call's draws -----------------------------------------------------------------------------------------------------------------------
def twin_act(seed, ctr, n):
    d = T.act_draws(seed, ctr, n)
    return d[:n * 32].reshape(n, 32), d[n * 32:]


def _bits24(v):
    return np.round(v.astype(np.float64) * 16777216.0).astype(np.int64)


def _pair16(a, b):
    return chi2_uniform((_bits24(a) >> 20) * 16 + (_bits24(b) >> 20), 256)


def act_uniformity(gen):
    hi, lo = [], []
    for s, c in KEYS:
        taus, u = gen(s, c, N)
        b = _bits24(np.concatenate([taus.ravel(), u]))
        hi.append(chi2_uniform(b >> 16, 256)); lo.append(chi2_uniform(b & 255, 256))
    return np.array(hi + lo)


def act_serial(gen):
    """16 x 16 cells of non-overlapping pairs (v[i], v[i + lag]) of the flat buffer, lag 1 and lag 32."""
    out = []
    for s, c in KEYS:
        taus, u = gen(s, c, N)
        v = np.concatenate([taus.ravel(), u])
        out.append(_pair16(v[0::2], v[1::2]))
        w = v.reshape(-1, 2, 32)      # (33 n / 64 blocks of 64): element i of the first half against element i + 32
        out.append(_pair16(w[:, 0].ravel(), w[:, 1].ravel()))
    return np.array(out)


def act_row_corr(gen):
    """The 33 x 33 correlations between row e's draws (32 taus, then its exploration uniform) and row e + 1's."""
    out = []
    for s, c in KEYS:
        taus, u = gen(s, c, N)
        rows = np.concatenate([taus, u[:, None]], axis=1)
        out.append(corr_z(rows[:-1], rows[1:]))
    return np.array(out)


def act_own_corr(gen):
    """The 32 correlations of a row's exploration uniform with its own taus."""
    return np.array([corr_z(u[:, None], taus) for taus, u in (gen(s, c, N) for s, c in KEYS)])


def act_call_pairs(gen):
    """16 x 16 cells of (draw i of call c, draw i of call c + 1), and of (call 0, call 2^32) per seed."""
    out = []
    for s, c in KEYS + [(s, None) for s in SEEDS]:
        c0, c1 = (0, 2**32) if c is None else (c, c + 1)
        (ta, ua), (tb, ub) = gen(s, c0, N), gen(s, c1, N)
        out.append(_pair16(np.concatenate([ta.ravel(), ua]), np.concatenate([tb.ravel(), ub])))
    return np.array(out)


ACT_GROUPS = {      # name: (statistics of a generator, degrees of freedom or None for two-sided normal deviates)
    "uniformity": (act_uniformity, 255), "serial": (act_serial, 255), "row_corr": (act_row_corr, None), "own_corr": (act_own_corr, None),
    "call_pairs": (act_call_pairs, 255),
}


def _group(groups, name, gen):
    fn, df = groups[name]
    stats = fn(gen)
    bound = chi2_bound(df, P / stats.size) if df else z_bound(P / stats.size)
    return stats, bound, df


@pytest.mark.parametrize("name", list(ACT_GROUPS))
def test_act_draws(name):
    """Per (seed, ctr) of {0, 123, 2^63 - 1, 2^64 - 1} x {0, 1, 2^32 - 1, 2^32} at n = 4 096: 256-bin uniformity of all 33 n values and of the low
    8 of their 24 bits; 16 x 16 serial pairs at lag 1 and 32; the 33 x 33 correlations of row e with row e + 1; a row's uniform against its own
    taus; 16 x 16 pairs of the same index in calls c and c + 1 (and 0 and 2^32).
    Observed worst |z|: uniformity 2.32 (m = 32, bound 5.41), serial 1.47 (32, 5.41), row_corr 4.33 (17 424, 6.55), own_corr 3.83 (512, 6.00),
    call_pairs 2.68 (20, 5.33)."""
    stats, bound, df = _group(ACT_GROUPS, name, twin_act)
    assert _judge("act " + name, stats, bound, df)


def test_act_draws_are_24_bit_fractions_below_cvar():
    cv_rows = (np.arange(N) % 7 + 1).astype(np.float32) / np.float32(8.0)
    for s, c in KEYS:
        for cvar in (1.0, 0.25, cv_rows):
            d = T.act_draws(s, c, N, cvar)
            u = d[N * 32:]
            assert d.dtype == np.float32 and np.all(u >= 0) and np.all(u < 1) and np.all(u * 16777216.0 == np.floor(u * 16777216.0))
            taus = d[:N * 32].reshape(N, 32)
            lim = np.broadcast_to(np.asarray(cvar, dtype=np.float32).reshape(-1, 1), taus.shape)
            assert np.all(taus >= 0) and np.all(taus <= lim) and np.all(taus < 1)
            if not np.ndim(cvar) and cvar == 1.0:
                assert np.all(taus * 16777216.0 == np.floor(taus * 16777216.0))
        sh = T.act_draws(s, c, N, 0.25, shared=True)
        full = T.act_draws(s, c, N, 0.25)
        assert sh.shape == (32 + N,) and np.array_equal(sh[:32], full[:32]) and np.all(sh[32:] < 1)
        assert np.array_equal(sh[32:], T.u01(np.arange(32, 32 + N), *T.draw_keys(s, c)))


# ---- the exploration epilogue -------------------------------------------------------------------------------------------------------------------
def explore_stats(gen, eps):
    """Over the 16 calls' uniforms: 9-bin uniformity of the explored action, the 9 x 9 table of action against an independent greedy action, and the
    explored share as a binomial deviate (None at eps = 1: the share must be exactly 1)."""
    u = np.concatenate([gen(s, c, N)[1] for s, c in KEYS])
    greedy = np.random.default_rng(2024).integers(0, 9, u.size)
    act = T.explore_action(u, eps, greedy)
    ex = ~(u > np.float32(eps))
    assert np.array_equal(act[~ex], greedy[~ex]) and act.min() >= 0 and act.max() <= 8
    tab = np.bincount(act[ex] * 9 + greedy[ex], minlength=81).reshape(9, 9).astype(np.float64)
    indep = chi2_counts(tab, np.outer(tab.sum(1), tab.sum(0)) / tab.sum())
    share = None if eps >= 1.0 else (ex.sum() - u.size * eps) / math.sqrt(u.size * eps * (1 - eps))
    return chi2_uniform(act[ex], 9), indep, share, float(ex.mean())


@pytest.mark.parametrize("eps", [1.0, 0.3, 0.05])
def test_exploration_action(eps):
    """Among rows with u <= eps the action is uniform over 9 and independent of the greedy action; the explored share is eps.
    Observed z at eps 1.0 / 0.3 / 0.05: uniformity -1.03 / -0.02 / -0.18, independence -0.78 / 0.60 / 0.22, share exact / 1.23 / 0.53 (bounds 4.75, 4.75,
    4.89)."""
    uni, indep, share, frac = explore_stats(twin_act, eps)
    ok = _judge(f"explore eps {eps} uniform", [uni], chi2_bound(8, P), 8)
    ok &= _judge(f"explore eps {eps} independence", [indep], chi2_bound(64, P), 64)
    if share is None:
        assert frac == 1.0
    else:
        ok &= _judge(f"explore eps {eps} share", [share], z_bound(P))
    assert ok


def test_exploration_action_edges():
    for eps in (1.0, 0.3, 0.05):
        e32 = np.float32(eps)
        below = np.nextafter(e32, np.float32(0))
        above = np.nextafter(e32, np.float32(2))
        got = T.explore_action(np.array([0.0, e32, below, above], dtype=np.float32), eps, [4, 4, 4, 4])
        assert got.tolist() == [0, 8, 8, 4], (eps, got)
    assert T.explore_action(np.float32([0.0, 0.5]), 0.0, [3, 6]).tolist() == [3, 6]      # eps = 0: always greedy
    # the nine cells are the intervals [a / 9, (a + 1) / 9) of u / eps
    u = (np.arange(9, dtype=np.float32) + np.float32(0.5)) / np.float32(9) * np.float32(0.3)
    assert T.explore_action(u, 0.3, np.full(9, -1)).tolist() == list(range(9))


# ---- the gradient step's taus -------------------------------------------------------------------------------------------------------------------
def tau_stats(gen):
    out = []
    for count in (2 * 256 * 8, 2 * 1024 * 8):
        for s, c in KEYS:
            v = gen(T.sample_base(s, c), count)
            b = _bits24(v)
            assert v.dtype == np.float32 and b.min() >= 0 and b.max() < 2**24 and np.array_equal(b.astype(np.float32) / np.float32(2**24), v)
            out += [chi2_uniform(b >> 16, 256), _pair16(v[0::2], v[1::2])]
    return np.array(out)


def test_sample_taus():
    """256-bin uniformity and 16 x 16 lag-1 pairs at 2 * 256 * 8 and 2 * 1 024 * 8 draws, over the same seeds and counters.
    Observed worst |z|: 3.20 (m = 64, bound 5.53)."""
    stats = tau_stats(T.sample_taus)
    assert _judge("sample_taus", stats, chi2_bound(255, P / stats.size), 255)


# ---- the replay batch ---------------------------------------------------------------------------------------------------------------------------
BIJECTION_N = (1, 2, 3, 4, 5, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1000, 4097)


@pytest.mark.parametrize("n", BIJECTION_N)
def test_perm_row_is_a_bijection(n):
    for s, c in KEYS:
        p = T.perm_row(T.sample_base(s, c), n, np.arange(n))
        assert p.dtype == np.int64 and np.array_equal(np.sort(p), np.arange(n)), (n, s, c)


@pytest.mark.parametrize("n", [100_000, 2**31 - 1])
def test_perm_row_large_rings(n):
    for s, c in KEYS:
        p = T.perm_row(T.sample_base(s, c), n, np.arange(1024))
        assert p.min() >= 0 and p.max() < n and np.unique(p).size == 1024
    spread = np.concatenate([T.perm_row(T.sample_base(s, c), n, np.arange(1024)) for s, c in KEYS])
    assert spread.max() > n // 2      # (the images are not confined to a low sub-range)


REPS, BATCH = 3000, 64


def perm_calls(n, rounds=4):
    """[REPS + 1][64]: the batches of calls 0 .. REPS under seed 123."""
    return T.perm_row(T.sample_base(123, np.arange(REPS + 1, dtype=np.uint64))[:, None], n, np.arange(BATCH)[None, :], rounds)


def _bins8(x, n):
    return x * 8 // n


def perm_stats(n, rounds=4):
    """Of 3 000 batches of 64 from a ring of n: inclusion frequency, slot-0 uniformity, adjacent-slot pairs, the same slot in consecutive calls."""
    calls = perm_calls(n, rounds)
    rows, nxt = calls[:REPS], calls[1:]
    p = BATCH / n
    cnt = np.bincount(rows.ravel(), minlength=n).astype(np.float64)
    # the indicator vector of one call has covariance p (1 - p) n / (n - 1) (I - J / n) under sampling WITHOUT replacement, so the sum of squares over
    # the n rows, divided by that variance, is chi-square with n - 1 degrees of freedom
    incl = float(((cnt - REPS * p) ** 2).sum() / (REPS * p * (1 - p) * n / (n - 1)))
    sizes = np.bincount(_bins8(np.arange(n), n), minlength=8).astype(np.float64)      # true bin sizes
    slot0 = chi2_counts(np.bincount(_bins8(rows[:, 0], n), minlength=8), REPS * sizes / n)
    a, b = _bins8(rows[:, :-1], n).ravel(), _bins8(rows[:, 1:], n).ravel()
    exp_adj = REPS * (BATCH - 1) * sizes[:, None] * (sizes[None, :] - np.eye(8)) / (n * (n - 1.0))      # exact: two DISTINCT rows
    adj = chi2_counts(np.bincount(a * 8 + b, minlength=64).reshape(8, 8), exp_adj)
    cross = chi2_counts(np.bincount((_bins8(rows, n) * 8 + _bins8(nxt, n)).ravel(), minlength=64).reshape(8, 8),
                        REPS * BATCH * np.outer(sizes, sizes) / (n * n))
    return {"inclusion": (incl, n - 1), "slot0": (slot0, 7), "adjacent": (adj, 63), "next_call": (cross, 63)}


PERM_N = (65, 129, 300)


def _perm_verdict(name, all_stats):
    ok = True
    for key in ("inclusion", "slot0", "adjacent", "next_call"):
        zs, fine = [], True
        for n, st in all_stats.items():
            x, df = st[key]
            fine &= x <= chi2_bound(df, P / len(all_stats))
            zs.append(float(chi2_z(x, df)))
        print(f"{name} {key}: |z| per n {dict(zip(all_stats, [round(z, 2) for z in zs]))}, bound |z| = {z_bound(P / len(all_stats), two_sided=False):.2f}")
        ok &= fine
    return ok


def test_perm_row_sampling_statistics():
    """3 000 calls of batch 64 at n in {65, 129, 300}: inclusion frequency (variance of sampling without replacement), slot-0 uniformity over 8
    bins of true size, 8 x 8 adjacent-slot pairs against the exact without-replacement expectation reps 63 s_a (s_b - [a = b]) / (n (n - 1)),
    8 x 8 pairs of slot k in call c and call c + 1.  (The 63 adjacent pairs of a call overlap and are drawn without replacement: chi-square with
    63 degrees of freedom is the conventional approximation of that statistic's null, not its exact law.)
    Observed z at n = 65 / 129 / 300 (bound 4.97): inclusion 1.32 / -0.10 / -0.56, slot0 -0.40 / -0.11 / -2.09, adjacent -1.67 / -2.44 / 0.32,
    next_call -2.52 / 0.49 / 0.23 (negative = more even than independent draws: a batch of 64 out of 65 rows is nearly the whole ring)."""
    assert _perm_verdict("perm_row", {n: perm_stats(n) for n in PERM_N})


# ---- the random policy's action -----------------------------------------------------------------------------------------------------------------
def _pair81(a, b):
    return chi2_uniform(np.asarray(a, dtype=np.int64) * 9 + b, 81)


def action_stats(gen):
    U = lambda x: np.asarray(x, dtype=np.uint64)
    steps64, envs = U(np.arange(64))[:, None], U(np.arange(65536))[None, :]
    long_steps = U(np.arange(65536))
    uni, pairs = [], []
    for seed in (0, 42, 2**64 - 1):
        block = gen(seed, steps64, envs)
        assert block.min() >= 0 and block.max() <= 8
        uni.append(chi2_uniform(block, 9))                                     # 65 536 envs x 64 steps
        one_env = gen(seed, long_steps, 7)
        uni.append(chi2_uniform(one_env, 9))                                   # one env over 65 536 steps
        pairs.append(_pair81(one_env[0::2], one_env[1::2]))                    # (step t, t + 1), one env
        pairs.append(_pair81(block[3, 0::2], block[3, 1::2]))                  # (env e, e + 1), one step
        for env0 in (65536, 2**32 + 5):
            for step0 in (2**32, 2**64 - 2):      # (the step counter wraps past 2^64 - 1, as the device's does)
                far = gen(seed, T.u64(step0) + steps64[:8], T.u64(env0) + envs)
                uni.append(chi2_uniform(far, 9))
                pairs.append(_pair81(far[0], block[0]))                        # against (step 0, env 0 ..): no 32-bit aliasing of step or env
        pairs.append(_pair81(gen(seed, steps64[:8], T.u64(2**32) + envs), block[:8]))
        pairs.append(_pair81(gen(seed, T.u64(2**32) + steps64[:8], envs), block[:8]))
    return np.array(uni), np.array(pairs)


def test_random_action():
    """9-bin uniformity over 65 536 envs x 64 steps and of one env over 65 536 steps; 81-bin pairs of (step t, t + 1) for one env and (env e, e + 1)
    for one step; the same at env0 offsets 65 536 and 2^32 + 5 and steps from 2^32 and 2^64 - 2, whose draws are also paired against the un-offset
    ones (a step or env index cut to 32 bits would repeat them).  Observed worst |z|: uniformity 1.21 (m = 18, bound 5.31), pairs 1.87 (24, 5.36)."""
    uni, pairs = action_stats(T.random_action)
    ok = _judge("random_action uniformity", uni, chi2_bound(8, P / uni.size), 8)
    ok &= _judge("random_action pairs", pairs, chi2_bound(80, P / pairs.size), 80)
    assert ok
    x = np.array([0, 1, 2**64 - 1, 2**63, (2**64) // 9, (2**64) // 9 + 1, 0x123456789ABCDEF0], dtype=np.uint64)
    assert [int(v) for v in T.mulhi9(x)] == [(int(v) * 9) >> 64 for v in x]


# ---- power: the same statistics at the same bounds reject planted defects ---------------------------------------------------------------------
def _rejected(groups, name, gen):
    stats, bound, df = _group(groups, name, gen)
    return not _judge("planted, " + name, stats, bound, df)


def _keyed(seed, ctr, n, u_index=None, stride=32, hash_fn=T.u01):
    k0, k1 = T.draw_keys(seed, ctr)
    e = np.arange(n, dtype=np.uint64)
    taus = hash_fn((e[:, None] * np.uint64(stride) + np.arange(32, dtype=np.uint64)[None, :]), k0, k1)
    u = hash_fn(e * np.uint64(32) if u_index == "tau0" else np.uint64(32 * n) + e, k0, k1)
    return taus, u


def test_battery_rejects_uniform_read_at_tau0():
    assert np.array_equal(np.concatenate([x.ravel() for x in _keyed(5, 9, 64)]), T.act_draws(5, 9, 64))      # the parts do rebuild the twin
    assert _rejected(ACT_GROUPS, "own_corr", lambda s, c, n: _keyed(s, c, n, u_index="tau0"))


def test_battery_rejects_row_stride_31():
    assert _rejected(ACT_GROUPS, "row_corr", lambda s, c, n: _keyed(s, c, n, stride=31))


def test_battery_rejects_keys_that_ignore_the_counter():
    assert _rejected(ACT_GROUPS, "call_pairs", lambda s, c, n: twin_act(s, 0, n))
    # ... and a counter that enters only with its low 32 bits
    assert _rejected(ACT_GROUPS, "call_pairs", lambda s, c, n: twin_act(s, c & 0xFFFFFFFF, n))


def test_battery_rejects_a_single_multiply_for_the_hash():
    def weak(idx, k0, k1):
        with np.errstate(over="ignore"):
            h = (idx.astype(np.uint32) ^ k0) * np.uint32(0x85EBCA6B) + k1
        return (h >> np.uint32(8)).astype(np.float32) * np.float32(2.0**-24)
    assert _rejected(ACT_GROUPS, "serial", lambda s, c, n: _keyed(s, c, n, hash_fn=weak))


def test_battery_rejects_a_one_round_feistel():
    assert not _perm_verdict("planted, one-round perm_row", {n: perm_stats(n, rounds=1) for n in PERM_N})


def test_battery_rejects_an_action_that_ignores_the_step():
    uni, pairs = action_stats(lambda seed, step, env: T.random_action(seed, np.zeros_like(T.u64(step)), env))
    assert not _judge("planted, random_action pairs", pairs, chi2_bound(80, P / pairs.size), 80)
