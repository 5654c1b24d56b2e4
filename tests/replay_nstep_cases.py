"""What the n-step replay tests share (test_replay_nstep_cpu.py, test_replay_nstep_gpu.py): a plain per-stream restatement of the window rule of
include/marinenav_hip.h ("n-step window") -- a deque per stream, np.float32 arithmetic in the rule's order, a list as the ring -- and the inputs: random
streams with planted rewards and the hand-made done patterns."""
from collections import deque

import numpy as np
import torch

GAMMA = 0.99
RING = ("states", "next_states", "actions", "rewards", "dones")
# rewards that show a contracted multiply-add, a reordered sum or a dropped `0 + x`: -0.0 (0 + -0 = +0), a tiny and a huge magnitude beside unit ones
PLANTED = (np.float32(-0.0), np.float32(1e-30), np.float32(np.float32(3e38) * np.float32(0.3)))


class PlainNstep:
    """The rule, one stream at a time.  `add(rows)` takes k transitions (s [26], a, r, ns [26], d) -- row i is stream i's -- and writes what the call emits into
    a ring of python lists: slot (ptr + i) mod capacity, only the newest `capacity` rows of a call."""

    def __init__(self, capacity, k, n_step, mode, gamma=GAMMA):
        self.cap, self.k, self.n, self.mode = capacity, k, n_step, mode
        self.g = [np.float32(gamma ** i) for i in range(n_step)]
        self.win = [deque(maxlen=n_step) for _ in range(k)]
        self.ring = [None] * capacity
        self.ptr = self.size = 0

    def emit(self, w):
        n = self.n
        dones = [bool(t[4]) for t in w]
        j = dones.index(True) if (self.mode == "episode" and any(dones)) else n - 1
        ret = np.float32(0.0)
        for i in range(j + 1):
            ret = np.float32(ret + np.float32(self.g[i] * np.float32(w[i][2])))
        done = any(dones) if self.mode == "episode" else dones[n - 1]
        return w[0][0], w[0][1], ret, w[j][3], np.float32(1.0 if done else 0.0)

    def add(self, rows):
        out = []
        for i, t in enumerate(rows):
            self.win[i].append(t)
            if len(self.win[i]) == self.n:
                out.append(self.emit(list(self.win[i])))
        for t in out[-self.cap:]:
            self.ring[self.ptr] = t
            self.ptr = (self.ptr + 1) % self.cap
            self.size = min(self.cap, self.size + 1)


def same_as_plain(buf, plain):
    """The torch / HIP ring `buf` holds exactly what the restatement holds: ptr, size, and every written slot bit for bit."""
    assert (buf.ptr, buf.size) == (plain.ptr, plain.size)
    s, ns, a, r, d = (getattr(buf, name).cpu().numpy() for name in RING)
    for slot, t in enumerate(plain.ring):
        if t is None:
            continue
        assert s[slot].tobytes() == t[0].tobytes() and ns[slot].tobytes() == t[3].tobytes(), slot
        assert int(a[slot, 0]) == int(t[1]) and r[slot, 0].tobytes() == np.float32(t[2]).tobytes() and d[slot, 0].tobytes() == t[4].tobytes(), (slot, r[slot, 0], t[2])


def same_rings(a, b, window=True):
    """Two rings of the package are equal: the five ring tensors, ptr, size and (window) every window tensor and the window's count."""
    assert (a.ptr, a.size) == (b.ptr, b.size)
    for name in RING:
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    if window:
        ha, hb = a._hist, b._hist
        assert (ha is None) == (hb is None)
        if ha is not None:
            assert ha.keys() == hb.keys() and ha["count"] == hb["count"]
            for key in ha:
                if key != "count":
                    assert ha[key].dtype == hb[key].dtype and torch.equal(ha[key], hb[key]), key


DONE_PATTERNS = ("random", "none", "all", "newest", "head", "two")


def done_pattern(name, adds, k, n_step, rng):
    """dones [adds][k] u8.  random: p = 0.25.  none / all.  newest: a done every n_step-th add, so that (stream 0's) full windows see it in their newest slot
    first and never two at once.  head: the same one step earlier -- together the two put a single done into every slot of some window, the head and the
    newest among them.  two: dones in pairs of consecutive adds (and, n_step = 2 aside, two steps apart as well): two in one window.  Streams are
    staggered by their index so that one call holds windows in different phases."""
    d = np.zeros((adds, k), np.uint8)
    t = np.arange(adds)[:, None] + np.arange(k)[None, :]
    if name == "random":
        d = (rng.random((adds, k)) < 0.25).astype(np.uint8)
    elif name == "all":
        d[:] = 1
    elif name == "newest":
        d = (t % n_step == n_step - 1).astype(np.uint8)
    elif name == "head":
        d = (t % n_step == 0).astype(np.uint8)
    elif name == "two":
        period = n_step + 3
        d = ((t % period == 0) | (t % period == 1) | (t % period == min(3, n_step))).astype(np.uint8)
    else:
        assert name == "none"
    return d


def make_stream(adds, k, n_step, pattern, seed):
    """`adds` vector steps of k streams as numpy arrays in the HIP env's dtypes: obs / next_obs [adds][k][26] f32, actions [adds][k] i32, rewards [adds][k]
    f32 (standard normal, with PLANTED values at seeded places), dones [adds][k] u8."""
    rng = np.random.default_rng(seed)
    obs = rng.standard_normal((adds, k, 26)).astype(np.float32)
    nxt = rng.standard_normal((adds, k, 26)).astype(np.float32)
    act = rng.integers(0, 9, (adds, k)).astype(np.int32)
    rew = rng.standard_normal((adds, k)).astype(np.float32)
    flat = rew.reshape(-1)
    where = rng.choice(flat.size, size=max(3, flat.size // 6), replace=False)
    for i, w in enumerate(where):
        flat[w] = PLANTED[i % 3]
    return obs, act, rew, nxt, done_pattern(pattern, adds, k, n_step, rng)


def rows_of(stream, t):
    """The k transitions of vector step t as the restatement takes them."""
    obs, act, rew, nxt, dn = stream
    return [(obs[t, i], int(act[t, i]), rew[t, i], nxt[t, i], int(dn[t, i])) for i in range(obs.shape[1])]
