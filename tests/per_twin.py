"""Host twin of the priority store of prioritized replay (csrc/per.hip; the rule: include/marinenav_hip.h, "Prioritized replay"), in numpy integer arithmetic
and Python ints, built on tests/rng_twin.py: the append, the exact stratified sampler with its importance weights, and the priority update.  Masses are uint32,
block sums uint64 over blocks of 1 024 rows; every sum is an integer sum.  float32 only where the kernels use float32 (weights, the mass rule); the `*_f64`
helpers give the same quantities in float64 as a yardstick.  Plain helper module, no fixtures, no torch, no GPU.
tests/test_per_cpu.py holds this twin to a brute-force restatement; tests/test_per_gpu.py and tests/test_per_scale_gpu.py hold the kernels to the twin."""
import numpy as np

import rng_twin as R

MASS_ONE = 1 << 16
BLOCK = 1024
MAX_CAPACITY = 1 << 20
MASS_MAX = (1 << 31) - 1
_PER_KEY = np.uint64(0x8CB92BA72F3D8DD7)


class Store:
    """mass [capacity] u32, bsum [ceil(capacity / 1024)] u64, mmax: what the device holds."""

    def __init__(self, capacity):
        assert 1 <= capacity <= MAX_CAPACITY
        self.capacity = int(capacity)
        self.mass = np.zeros(self.capacity, dtype=np.uint32)
        self.bsum = np.zeros((self.capacity + BLOCK - 1) // BLOCK, dtype=np.uint64)
        self.mmax = MASS_ONE

    def set_masses(self, mass):
        """Hand-made masses: rows [0, len(mass)), block sums formed anew."""
        mass = np.asarray(mass, dtype=np.uint32)
        self.mass[:] = 0
        self.mass[:len(mass)] = mass
        self.bsum[:] = block_sums(self.mass)

    @property
    def total(self):
        return sum(int(b) for b in self.bsum)


def hand_made(name, size, capacity=2053):
    """The hand-made mass vectors of the issue, `size` rows in a ring of `capacity`."""
    g = np.random.default_rng(7)
    m = np.zeros(size, dtype=np.uint32)
    if name == "equal":              # targets fall exactly on row boundaries: "exceeds" decides
        m[:] = MASS_ONE
    elif name == "one_heavy":        # one row holds 99 % of the mass: repeats
        m[:] = 1
        m[size // 3] = 99 * (size - 1)
    elif name == "holes":            # zero-mass holes, a whole empty block among them when there is one
        m[:] = g.integers(1, 5 * MASS_ONE, size)
        m[g.random(size) < 0.4] = 0
        m[1024:2048] = 0
        m[0] = 0
        m[size - 1] = 3
    elif name == "random":
        m[:] = g.integers(1, MASS_MAX, size, dtype=np.int64) >> g.integers(0, 30, size)
        m[m == 0] = 1
    else:
        raise KeyError(name)
    st = Store(capacity)
    st.set_masses(m)
    return st


LARGE_VECTORS = ("random", "saturated", "ones", "holes_wide", "heavy_far", "young")


def hand_made_large(name, size, capacity):
    """Mass vectors for rings of the sizes training uses (65 blocks and more: the sampler's scan crosses wavefronts), `size` rows in a ring of `capacity`."""
    g = np.random.default_rng(7)
    m = np.zeros(size, dtype=np.uint32)
    if name == "random":
        m[:] = g.integers(1, MASS_MAX, size, dtype=np.int64) >> g.integers(0, 30, size)
        m[m == 0] = 1
    elif name == "saturated":        # the largest total the store admits: just under 2^51 at 2^20 rows
        m[:] = MASS_MAX
    elif name == "ones":             # the smallest total: q = size // batch
        m[:] = 1
    elif name == "holes_wide":       # zero-mass holes, the first block and the whole of blocks 64..127 -- one wavefront of the scan -- among them
        m[:] = g.integers(1, MASS_MAX, size, dtype=np.int64) >> g.integers(0, 30, size)
        m[m == 0] = 1
        m[g.random(size) < 0.4] = 0
        m[:1024] = 0
        m[64 * BLOCK:128 * BLOCK] = 0
        m[size - 1] = 3
    elif name == "heavy_far":        # one row of the last non-empty block holds 99 % of the mass: repeats, as far into the ring as its rows go
        m[:] = 1
        first = (size - 1) // BLOCK * BLOCK
        m[first + (size - first) // 3] = 99 * (size - 1)
    elif name == "young":            # a ring that has just reached its batch size: every later block is empty
        m[:] = MASS_ONE
    else:
        raise KeyError(name)
    st = Store(capacity)
    st.set_masses(m)
    return st


# (capacity, size): 64 blocks -- the last size one wavefront scans --, 65, train_iqn --per's default ring full and one row into block 64, a capacity that
# is no multiple of 4, --env-budget reference's ring, and the most the ABI admits
LARGE_GRID = [(65_536, 65_536), (66_560, 66_560), (100_000, 100_000), (100_000, 65_537), (99_997, 99_997), (1_000_000, 1_000_000), (1_048_576, 1_048_576)]


def large_case(name, capacity, size, batch):
    """(store, rows in use) of one vector at one place of the grid; `young` holds just `batch` rows, whatever the grid's size."""
    n = batch if name == "young" else size
    return hand_made_large(name, n, capacity), n


def rows_by_cumsum(mass, targets):
    """The rule restated without blocks, at sizes where Python ints are too slow: ONE cumulative sum over all rows in uint64 (exact: a total stays below
    2^51), then for every target the least row whose inclusive prefix exceeds it."""
    cs = np.cumsum(np.asarray(mass, dtype=np.uint64), dtype=np.uint64)
    t = np.array([int(x) for x in targets], dtype=np.uint64)
    assert int(t.max()) < int(cs[-1]), "target beyond the total mass"
    return np.searchsorted(cs, t, side="right").astype(np.int64)


def block_sums(mass):
    m = np.asarray(mass, dtype=np.uint64)
    pad = (-len(m)) % BLOCK
    return np.concatenate([m, np.zeros(pad, dtype=np.uint64)]).reshape(-1, BLOCK).sum(axis=1, dtype=np.uint64)


def append(st, ptr, n):
    """Rows [ptr, ptr + n) mod capacity get mass mmax; their blocks' sums move by the integer difference."""
    assert 0 <= ptr < st.capacity and 1 <= n <= st.capacity
    for i in range(n):
        slot = (ptr + i) % st.capacity
        old = int(st.mass[slot])
        st.mass[slot] = st.mmax
        st.bsum[slot // BLOCK] = np.uint64(int(st.bsum[slot // BLOCK]) + st.mmax - old)


def stratum_words(seed, ctr, batch):
    """U_k, k < batch: the 24-bit words of the call, Python ints."""
    base = R.sample_base(seed, ctr)
    with np.errstate(over="ignore"):
        x = R.mix64(base ^ (_PER_KEY * (np.arange(batch, dtype=np.uint64) + np.uint64(1))))
    return [int(v) >> 40 for v in x]


def targets(total, seed, ctr, batch):
    """target_k = k q + mulhi64(U_k << 40, q), q = total // batch."""
    q = total // batch
    return [k * q + (((u << 40) * q) >> 64) for k, u in enumerate(stratum_words(seed, ctr, batch))]


def find_row(st, target):
    """The least row whose inclusive prefix sum exceeds `target`, the kernel's way: the last block whose exclusive prefix is <= target, then that block's
    masses in order."""
    ex, b = 0, 0
    acc = 0
    for i, s in enumerate(st.bsum):
        if acc <= target:
            ex, b = acc, i
        acc += int(s)
    rem = target - ex
    cs = np.cumsum(st.mass[b * BLOCK:(b + 1) * BLOCK], dtype=np.uint64)      # (a block's sum is below 2^41: exact)
    r = int(np.searchsorted(cs, np.uint64(rem), side="right"))      # the first row of the block whose inclusive prefix exceeds the remainder
    assert r < len(cs), "target beyond the total mass"
    return b * BLOCK + r


def weights_f32(mass_rows, size, total, beta):
    """w_k = powf(size * m_k / total, -beta) / max: float32 throughout (numpy's float32 power stands in for powf: agreement is asked to 1e-5, not bits)."""
    f = np.float32
    x = (f(size) * np.asarray(mass_rows).astype(np.float32)) / f(total)
    w = np.power(x, f(-beta), dtype=np.float32)
    return w / w.max()


def weights_f64(mass_rows, size, total, beta):
    x = float(size) * np.asarray(mass_rows, dtype=np.float64) / float(total)
    w = x ** (-float(np.float32(beta)))
    return w / w.max()


def sample(st, size, batch, beta, seed, ctr):
    """One sampler call at call counter `ctr`: (idx int64 [B], weights float32 [B], taus float32 [2][B][8]); the caller advances the counter by one."""
    total = st.total
    assert batch <= size <= st.capacity and total >= batch
    idx = np.array([find_row(st, t) for t in targets(total, seed, ctr, batch)], dtype=np.int64)
    w = weights_f32(st.mass[idx], size, total, beta)
    taus = R.sample_taus(R.sample_base(seed, ctr), 2 * batch * 8).reshape(2, batch, 8)
    return idx, w, taus


def new_mass_f64(absdelta, alpha, eps):
    """clamp(floor((delta + eps) ** alpha * 65536 + 0.5), 1, 2^31 - 1) in float64, from the float32 inputs the kernel gets."""
    d = np.asarray(absdelta, dtype=np.float32).astype(np.float64) + float(np.float32(eps))
    v = np.floor(d ** float(np.float32(alpha)) * 65536.0 + 0.5)
    v = np.where(np.isnan(v), 1.0, v)
    return np.clip(v, 1, MASS_MAX).astype(np.int64)


def new_mass_f32(absdelta, alpha, eps):
    """The same in float32, operation by operation (the sum, the power, the product and the + 0.5 each round)."""
    f = np.float32
    d = np.asarray(absdelta, dtype=np.float32) + f(eps)
    v = np.floor(np.power(d, f(alpha), dtype=np.float32) * f(65536.0) + f(0.5))
    out = np.ones(d.shape, dtype=np.int64)
    ok = v >= 1      # (NaN: 1)
    out[ok] = np.minimum(v[ok].astype(np.float64), MASS_MAX).astype(np.int64)
    return out


def update(st, idx, new_mass):
    """Masses `new_mass` written to rows `idx`: the highest slot wins a repeated row; block sums move by the difference; mmax follows the masses written."""
    idx = np.asarray(idx)
    for k in range(len(idx)):
        row = int(idx[k])
        if row < 0 or row >= st.capacity or row in idx[k + 1:]:
            continue
        m, old = int(new_mass[k]), int(st.mass[row])
        st.mass[row] = m
        st.bsum[row // BLOCK] = np.uint64(int(st.bsum[row // BLOCK]) + m - old)
        st.mmax = max(st.mmax, m)
