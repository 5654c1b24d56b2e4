"""Host twin of every random draw the kernels make, in plain numpy integer arithmetic: the act call's taus and exploration uniforms
(csrc/iqn_act_common.h, iqn_act_split.h), the epsilon-greedy epilogue (iqn_act_exact.h / _split.h / _tiled.h), the gradient step's taus
(csrc/iqn_train.hip `sample_tau`), the replay batch (csrc/mn_train_shared.h `perm_row`) and the random-policy action (csrc/mn_rollout.hip
`draw_action`).  Written from those formulas: uint32 / uint64 arrays with wrap-around, float32 only where the kernel uses float32.  No torch, no GPU.
tests/test_rng_twin_cpu.py states what these streams must satisfy; tests/test_rng_draws_gpu.py holds the kernels to them bit for bit.
Plain helper module, no fixtures.  Seeds, counters, steps and env indices are full 64-bit values: a Python int of any sign is taken modulo 2^64,
an int64 array is reinterpreted."""
import numpy as np

K_TAUS = 32
N_ACTIONS = 9
_M64 = (1 << 64) - 1
_GOLDEN = np.uint64(0x9E3779B97F4A7C15)
_TAU_KEY = np.uint64(0xD1B54A32D192ED03)
_ROUND_KEY = np.uint64(0xA24BAED4963EE407)
_INV24 = np.float32(1.0 / 16777216.0)


def u64(x):
    """`x` as uint64 (array or 0-d array): Python ints modulo 2^64, int64 arrays reinterpreted."""
    if isinstance(x, (int, np.integer)) and not isinstance(x, np.uint64):
        return np.asarray(int(x) & _M64, dtype=np.uint64)
    a = np.asarray(x)
    if a.dtype == np.uint64:
        return a
    if a.dtype == np.int64:
        return a.view(np.uint64)
    if a.dtype == object:
        return np.array([int(v) & _M64 for v in a.ravel()], dtype=np.uint64).reshape(a.shape)
    assert a.dtype.kind in "iu", a.dtype
    return a.astype(np.int64).view(np.uint64)


def _u32(x):
    return np.asarray(x).astype(np.uint32)


def mix64(x):
    """splitmix64 finaliser (iqn_act_common.h `mix64`, mn_train_shared.h `mix64`, mn_rollout.hip `mix64r`: the same function)."""
    x = u64(x)
    with np.errstate(over="ignore"):
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return x ^ (x >> np.uint64(31))


def fmix32(x):
    """murmur3 finaliser (iqn_act_common.h `fmix32`, mn_train_shared.h `mix32`)."""
    x = _u32(x)
    with np.errstate(over="ignore"):
        x = (x ^ (x >> np.uint32(16))) * np.uint32(0x85EBCA6B)
        x = (x ^ (x >> np.uint32(13))) * np.uint32(0xC2B2AE35)
        return x ^ (x >> np.uint32(16))


def call_base(seed, ctr):
    """mix64(seed + golden * (ctr + 1)): the 64-bit key of call number `ctr` -- `draw_keys` splits it, `sample_base_at` uses it whole."""
    with np.errstate(over="ignore"):
        return mix64(u64(seed) + _GOLDEN * (u64(ctr) + np.uint64(1)))


def draw_keys(seed, ctr):
    """(k0, k1) of act call number `ctr` under `seed`: the low and the high word of the call's base."""
    base = call_base(seed, ctr)
    return _u32(base & np.uint64(0xFFFFFFFF)), _u32(base >> np.uint64(32))


def u01(idx, k0, k1):
    """Draw number `idx` (taken modulo 2^32) under the keys: a 24-bit uniform in [0, 1), float32."""
    with np.errstate(over="ignore"):
        h = fmix32(fmix32(_u32(idx) ^ k0) + k1)
    return (h >> np.uint32(8)).astype(np.float32) * _INV24


def act_draws(seed, ctr, n, cvar=1.0, shared=False):
    """The draw buffer of one act call, float32.  Per-row taus: [32 n] taus x cvar (a scalar, or [n] per row), then [n] exploration uniforms.
    `shared`: [32] taus x the scalar cvar, then [n] uniforms."""
    k0, k1 = draw_keys(seed, ctr)
    n_tau = K_TAUS if shared else n * K_TAUS
    d = u01(np.arange(n_tau + n, dtype=np.uint64), k0, k1)
    cv = np.asarray(cvar, dtype=np.float32)
    if cv.ndim:
        assert not shared and cv.shape == (n,)
        cv = np.repeat(cv, K_TAUS)
    d[:n_tau] = d[:n_tau] * cv
    return d


def explore_action(u, eps, greedy):
    """IQNAgent.act's epilogue as the kernels write it: greedy iff u > eps, else min((int)(u / eps * 9.0f), 8) in float32."""
    u = np.asarray(u, dtype=np.float32)
    eps = np.float32(eps)
    greedy = np.asarray(greedy)
    if not eps > 0:
        return greedy.astype(np.int32)
    x = (u / eps).astype(np.float32) * np.float32(N_ACTIONS)
    act = np.minimum(x.astype(np.int32), N_ACTIONS - 1)
    return np.where(u > eps, greedy, act).astype(np.int32)


def sample_base(seed, ctr):
    """`sample_base_at`: the key of the batch draw made at call counter `ctr`."""
    return call_base(seed, ctr)


def sample_taus(base, count):
    """`sample_tau(base, e)` for e in [0, count): the gradient step's taus, float32 (target network's 8 per row first)."""
    with np.errstate(over="ignore"):
        x = mix64(u64(base) ^ (_TAU_KEY * (np.arange(count, dtype=np.uint64) + np.uint64(1))))
    return (x >> np.uint64(40)).astype(np.float32) * _INV24


def perm_row(base, n, k, rounds=4):
    """Ring row of batch slot(s) `k`: the keyed permutation of [0, n) -- a balanced Feistel network of `rounds` (the kernels: 4) rounds on the
    smallest even-width power-of-two domain >= n, cycle-walked into [0, n).  `base` may be an array that broadcasts against `k` (one key per call);
    int64 array of the broadcast shape."""
    n = int(n)
    assert 1 <= n <= 0xFFFFFFFF
    bits = (n - 1).bit_length() if n > 1 else 1
    half = np.uint32((bits + 1) >> 1)
    mask = np.uint32((1 << int(half)) - 1)
    base = u64(base)
    shape = np.broadcast_shapes(base.shape, np.shape(k))
    with np.errstate(over="ignore"):
        rk = [np.broadcast_to(_u32(mix64(base + _ROUND_KEY * np.uint64(r + 1)) >> np.uint64(32)), shape) for r in range(rounds)]
    x = np.broadcast_to(_u32(k), shape).copy()
    todo = np.ones(shape, dtype=bool)
    while todo.any():
        v = x[todo]
        L, R = v >> half, v & mask
        for r in range(rounds):
            with np.errstate(over="ignore"):
                L, R = R, L ^ (fmix32(R + rk[r][todo]) & mask)
        x[todo] = (L << half) | R
        todo &= x >= np.uint32(n)
    return x.astype(np.int64)


def mulhi9(x):
    """High 64 bits of the 128-bit product x * 9 (`__umul64hi(x, 9)`), from the two 32-bit halves."""
    x = u64(x)
    nine, s32 = np.uint64(N_ACTIONS), np.uint64(32)
    lo, hi = x & np.uint64(0xFFFFFFFF), x >> s32
    return (hi * nine + ((lo * nine) >> s32)) >> s32


def random_action(seed, step, env):
    """`draw_action`: the random policy's action of global env `env` at step `step` (broadcast against each other), int32."""
    with np.errstate(over="ignore"):
        k = mix64(u64(seed) + _GOLDEN * (u64(step) + np.uint64(1)))
        x = mix64(k ^ (_TAU_KEY * (u64(env) + np.uint64(1))))
    return mulhi9(x).astype(np.int32)
