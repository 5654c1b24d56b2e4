"""Priority store of proportional prioritized experience replay (Schaul et al. 2016), next to the replay ring.

The rule, operation by operation: include/marinenav_hip.h, "Prioritized replay".  A row's priority is an integer mass (MASS_ONE = 1 << 16 is priority 1.0),
blocks of 1 024 rows carry an integer sum, so every sum is exact and the sampler is a function of the masses alone.  On a CUDA device the store is three
kernels of csrc/per.hip (`mn_per_append`, `mn_per_sample`, `mn_per_update`: one launch each, nothing synchronises with the host); on the CPU the same rule in
numpy integers / Python ints, row for row what the kernels choose (tests/per_twin.py is the test suite's independent restatement).

Tensors: `mass` [capacity] int32 and `mmax` [1] int32 hold the kernels' uint32 words (a mass never exceeds 2^31 - 1), `bsum` [ceil(capacity / 1024)] int64
their uint64 block sums (< 2^51), `rng_state` [2] int64 = {seed, call counter}, the state `mn_iqn_sample` uses.
"""
import ctypes as C

import numpy as np
import torch

MASS_ONE = 1 << 16
BLOCK = 1024
MAX_CAPACITY = 1 << 20
MAX_BATCH = 1024
MASS_MAX = (1 << 31) - 1
N_TAUS = 8

_M64 = (1 << 64) - 1
_GOLDEN, _TAU_KEY, _PER_KEY = 0x9E3779B97F4A7C15, 0xD1B54A32D192ED03, 0x8CB92BA72F3D8DD7


def _mix64(x):
    """splitmix64 finaliser on uint64 arrays (csrc/mn_train_shared.h `mix64`)."""
    with np.errstate(over="ignore"):
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return x ^ (x >> np.uint64(31))


def _keyed(base, key, count):
    """mix64(base ^ key (e + 1)) for e in [0, count)."""
    with np.errstate(over="ignore"):
        return _mix64(np.uint64(base) ^ (np.uint64(key) * (np.arange(count, dtype=np.uint64) + np.uint64(1))))


def beta_at(beta0, step, total_steps):
    """The importance exponent at gradient step `step` of a run of `total_steps`: linear from beta0 to 1 (constant beta0 where the run's length is unknown)."""
    if not total_steps:
        return float(beta0)
    return float(beta0) + (1.0 - float(beta0)) * min(1.0, max(0.0, step / float(total_steps)))


class PriorityStore:
    def __init__(self, capacity, device, seed):
        capacity = int(capacity)
        if capacity < 1 or capacity > MAX_CAPACITY:
            raise ValueError(f"prioritized replay holds at most {MAX_CAPACITY} rows (2^20: 1 024 block sums of 1 024 rows, one scan in one workgroup); "
                             f"a ring of {capacity} rows is refused")
        self.capacity = capacity
        self.device = torch.device(device)
        self.mass = torch.zeros(capacity, dtype=torch.int32, device=self.device)
        self.bsum = torch.zeros((capacity + BLOCK - 1) // BLOCK, dtype=torch.int64, device=self.device)
        self.mmax = torch.full((1,), MASS_ONE, dtype=torch.int32, device=self.device)
        self.rng_state = torch.tensor([int(seed) & 0x7FFFFFFFFFFFFFFF, 0], dtype=torch.int64, device=self.device)
        self._out = {}

    @property
    def _cuda(self):
        return self.device.type == "cuda"

    def _buffers(self, batch):
        if batch not in self._out:
            self._out[batch] = (torch.empty(batch, dtype=torch.int64, device=self.device), torch.empty(batch, dtype=torch.float32, device=self.device),
                                torch.empty(2, batch, N_TAUS, dtype=torch.float32, device=self.device))
        return self._out[batch]

    # ---- the three operations ------------------------------------------------------------------
    def append(self, ptr, n):
        """The ring wrote rows [ptr, ptr + n) mod capacity: they get mass mmax.  Call behind the write, before `ptr` moves."""
        ptr, n = int(ptr), int(n)
        if n <= 0:
            return
        if self._cuda:
            from .. import _capi
            p = lambda t: C.c_void_p(t.data_ptr())
            rc = _capi.lib().mn_per_append(p(self.mass), p(self.bsum), p(self.mmax), ptr, n, self.capacity, _capi.stream_ptr(self.device))
            if rc:
                raise _capi.MarineNavHipError(f"mn_per_append failed ({rc})")
            return
        assert 0 <= ptr < self.capacity and n <= self.capacity
        mass, bsum, mmax = self.mass.numpy(), self.bsum.numpy(), int(self.mmax[0])
        rows = (ptr + np.arange(n, dtype=np.int64)) % self.capacity
        np.add.at(bsum, rows // BLOCK, np.int64(mmax) - mass[rows].astype(np.int64))
        mass[rows] = mmax

    def sample(self, size, batch, beta):
        """One stratified draw of `batch` rows among the first `size`: (idx [B] int64, weights [B] float32, taus [2][B][8] float32), in buffers the next call of
        this batch size overwrites.  The call counter advances by one."""
        size, batch = int(size), int(batch)
        idx, w, taus = self._buffers(batch)
        if self._cuda:
            from .. import _capi
            p = lambda t: C.c_void_p(t.data_ptr())
            rc = _capi.lib().mn_per_sample(p(self.mass), p(self.bsum), size, self.capacity, batch, C.c_float(beta), p(self.rng_state), p(idx), p(w), p(taus),
                                           _capi.stream_ptr(self.device))
            if rc:
                raise _capi.MarineNavHipError(f"mn_per_sample failed ({rc}): need batch <= {MAX_BATCH} and batch <= size <= capacity")
            return idx, w, taus
        assert 1 <= batch <= MAX_BATCH and batch <= size <= self.capacity
        mass, bsum = self.mass.numpy(), self.bsum.numpy()
        seed, ctr = (int(v) & _M64 for v in self.rng_state.tolist())
        base = int(_mix64(np.asarray((seed + _GOLDEN * (ctr + 1)) & _M64, dtype=np.uint64)))
        ex = np.concatenate([[0], np.cumsum(bsum)[:-1]])      # exclusive prefix of the block sums (< 2^51: int64 is exact)
        total = int(bsum.sum())
        q = total // batch
        rows = np.empty(batch, dtype=np.int64)
        for k, x in enumerate(_keyed(base, _PER_KEY, batch)):
            target = k * q + ((((int(x) >> 40) << 40) * q) >> 64)
            b = int(np.searchsorted(ex, target, side="right")) - 1      # the last block whose exclusive prefix is <= target
            cs = np.cumsum(mass[b * BLOCK:(b + 1) * BLOCK], dtype=np.int64)
            rows[k] = b * BLOCK + int(np.searchsorted(cs, target - int(ex[b]), side="right"))      # the first row whose inclusive prefix exceeds it
        f = np.float32
        wk = np.power((f(size) * mass[rows].astype(np.float32)) / f(total), f(-beta), dtype=np.float32)
        idx.copy_(torch.from_numpy(rows))
        w.copy_(torch.from_numpy(wk / wk.max()))
        t = (_keyed(base, _TAU_KEY, 2 * batch * N_TAUS) >> np.uint64(40)).astype(np.float32) * f(1.0 / 16777216.0)
        taus.copy_(torch.from_numpy(t).view(2, batch, N_TAUS))
        self.rng_state[1] += 1
        return idx, w, taus

    def update(self, idx, absdelta, alpha, eps):
        """Slot k's priority |delta_k| becomes mass clamp(floor((delta_k + eps) ** alpha * 65536 + 0.5), 1, 2^31 - 1) of row idx[k]; the highest slot wins a
        repeated row."""
        batch = int(idx.shape[0])
        if self._cuda:
            from .. import _capi
            assert idx.is_cuda and idx.dtype == torch.int64 and idx.is_contiguous() and absdelta.is_cuda and absdelta.dtype == torch.float32 and absdelta.is_contiguous()
            p = lambda t: C.c_void_p(t.data_ptr())
            rc = _capi.lib().mn_per_update(p(self.mass), p(self.bsum), p(self.mmax), p(idx), p(absdelta), batch, C.c_float(alpha), C.c_float(eps), self.capacity,
                                           _capi.stream_ptr(self.device))
            if rc:
                raise _capi.MarineNavHipError(f"mn_per_update failed ({rc})")
            return
        f = np.float32
        mass, bsum = self.mass.numpy(), self.bsum.numpy()
        d = absdelta.detach().to(torch.float32).numpy() + f(eps)
        v = np.floor(np.power(d, f(alpha), dtype=np.float32) * f(65536.0) + f(0.5))
        rows = idx.numpy()
        seen = set()
        mmax = int(self.mmax[0])
        for k in range(batch - 1, -1, -1):      # from the highest slot down: the first to name a row is its writer
            row = int(rows[k])
            if row in seen or row < 0 or row >= self.capacity:
                continue
            seen.add(row)
            m = int(min(float(v[k]), MASS_MAX)) if v[k] >= 1 else 1      # (NaN: 1)
            bsum[row // BLOCK] += m - int(mass[row])
            mass[row] = m
            mmax = max(mmax, m)
        self.mmax[0] = mmax

    # ---- checkpoints ---------------------------------------------------------------------------
    def state_dict(self, size):
        """Masses of rows [0, size) (a row never written has mass 0), mmax and the generator state; the block sums are formed anew on load."""
        return dict(mass=self.mass[:int(size)].cpu(), mmax=int(self.mmax[0]), rng_state=self.rng_state.cpu())

    def load_state_dict(self, sd, size):
        """`sd` None (a ring saved without priorities): its `size` rows load as uniform, mass MASS_ONE each."""
        self.mass.zero_()
        if sd is None:
            self.mass[:int(size)] = MASS_ONE
            self.mmax.fill_(MASS_ONE)
            self.rng_state[1] = 0
        else:
            self.mass[:sd["mass"].shape[0]].copy_(sd["mass"])
            self.mmax.fill_(int(sd["mmax"]))
            self.rng_state.copy_(sd["rng_state"])
        pad = (-self.capacity) % BLOCK
        m = torch.cat([self.mass.to(torch.int64), torch.zeros(pad, dtype=torch.int64, device=self.device)])
        self.bsum.copy_(m.view(-1, BLOCK).sum(dim=1))
