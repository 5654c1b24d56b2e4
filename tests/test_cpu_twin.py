"""oracle/libmarinenav_cpu.so -- the CPU twin of the env entry points of include/marinenav_hip.h (same names, same
signatures, host pointers) -- driven through the SAME ctypes table (`_capi.SIGNATURES`) as the HIP library.
CPU: the twin replays the reference's golden traces through the mn_* API.  GPU: one driver function, two libraries,
same results."""
import ctypes as C
import os

import numpy as np
import pytest

from distributional_rl_navigation_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")
TWIN = os.path.join(ROOT, "oracle", "libmarinenav_cpu.so")
ENV_SYMBOLS = ("mn_default_params", "mn_create", "mn_destroy", "mn_last_error", "mn_num_envs", "mn_set_params", "mn_get_params",
               "mn_seed", "mn_set_schedule", "mn_set_start_goal", "mn_reset", "mn_step", "mn_step_append", "mn_build_info",
               "mn_reset_done", "mn_load_worlds", "mn_get_worlds", "mn_get_state", "mn_set_state", "mn_enable_obs64", "mn_get_obs64",
               "mn_get_reward64", "mn_peek_next_double", "mn_last_done_count", "mn_profile_begin", "mn_profile_end", "mn_profile_reset_end")


def bind(path):
    """The package's own binding table applied to an arbitrary library exporting the env entry points."""
    L = C.CDLL(path)
    for name, res, args in _capi.SIGNATURES:
        if name in ENV_SYMBOLS:
            fn = getattr(L, name)
            fn.restype, fn.argtypes = res, args
    return L


class Driver:
    """Minimal client of the C-ABI, written once, used with both libraries.  `alloc` makes the I/O buffers (numpy for the
    twin, torch device tensors for the HIP library); `ptr` / `host` turn them into pointers / numpy arrays."""

    def __init__(self, L, n, alloc, ptr, host, precision=_capi.PRECISION_F64, seeds=None):
        self.L, self.n, self.ptr, self.host = L, n, ptr, host
        self.p = _capi.MnParams()
        assert L.mn_default_params(C.byref(self.p)) == 0
        self.p.precision = precision
        self.h = C.c_void_p()
        assert L.mn_create(n, C.byref(self.p), C.byref(self.h)) == 0, L.mn_last_error(None)
        if precision == _capi.PRECISION_F64:
            assert L.mn_enable_obs64(self.h, 1) == 0      # float64 observation / reward copies are opt-in
        s = np.ascontiguousarray(np.arange(n) if seeds is None else seeds, dtype=np.uint32)
        assert L.mn_seed(self.h, s.ctypes.data_as(C.POINTER(C.c_uint32)), None) == 0
        self.obs = [alloc((n, 26), np.float32), alloc((n, 26), np.float32)]
        self.rew = alloc((n,), np.float32); self.done = alloc((n,), np.uint8); self.info = alloc((n,), np.uint8)
        self.act = alloc((n,), np.int32)
        self.cur = 0

    def set(self, **kw):
        for k, v in kw.items():
            setattr(self.p, k, v)
        assert self.L.mn_set_params(self.h, C.byref(self.p)) == 0

    def reset(self):
        assert self.L.mn_reset(self.h, None, self.ptr(self.obs[self.cur]), None) == 0
        return self.obs64()

    def step(self, actions, set_actions):
        set_actions(self.act, actions)
        self.cur ^= 1
        assert self.L.mn_step(self.h, self.ptr(self.act), self.ptr(self.obs[self.cur]), self.ptr(self.rew), self.ptr(self.done),
                              self.ptr(self.info), None) == 0
        return self.obs64(), self.rew64(), self.host(self.done).copy(), self.host(self.info).copy()

    def reset_done(self):
        assert self.L.mn_reset_done(self.h, self.ptr(self.obs[self.cur]), None) == 0
        return self.obs64()

    def obs64(self):
        out = np.zeros((self.n, 26))
        assert self.L.mn_get_obs64(self.h, 0, self.n, out.ctypes.data_as(C.POINTER(C.c_double))) == 0
        return out

    def rew64(self):
        out = np.zeros(self.n)
        assert self.L.mn_get_reward64(self.h, 0, self.n, out.ctypes.data_as(C.POINTER(C.c_double))) == 0
        return out

    def state(self):
        s = np.zeros((self.n, 6)); ep = np.zeros(self.n, np.int32); tot = np.zeros(self.n, np.int64)
        assert self.L.mn_get_state(self.h, 0, self.n, s.ctypes.data_as(C.POINTER(C.c_double)), ep.ctypes.data_as(C.POINTER(C.c_int32)),
                                   tot.ctypes.data_as(C.POINTER(C.c_int64))) == 0
        return s, ep, tot

    def worlds(self):
        """mn_get_worlds: dict of the padded tables -- cores [n, 8, 4] = x, y, clockwise, Gamma; obstacles [n, 10, 3] = x, y, r; counts;
        start / goal [n, 2]; theta0 / speed0 [n]."""
        n, d, i = self.n, C.POINTER(C.c_double), C.POINTER(C.c_int32)
        nc = np.zeros(n, np.int32); no = np.zeros(n, np.int32); cw = np.zeros((n, 8), np.int32)
        cxy = np.zeros((n, 8, 2)); gm = np.zeros((n, 8)); oxy = np.zeros((n, 10, 2)); orr = np.zeros((n, 10))
        st = np.zeros((n, 2)); gl = np.zeros((n, 2)); th = np.zeros(n); sp = np.zeros(n)
        p = lambda a, t: a.ctypes.data_as(t)
        assert self.L.mn_get_worlds(self.h, 0, n, p(nc, i), p(cxy, d), p(cw, i), p(gm, d), p(no, i), p(oxy, d), p(orr, d), p(st, d), p(gl, d),
                                    p(th, d), p(sp, d)) == 0
        return dict(cores=np.concatenate([cxy, cw[:, :, None].astype(np.float64), gm[:, :, None]], axis=2),
                    obstacles=np.concatenate([oxy, orr[:, :, None]], axis=2), ncores=nc, nobs=no, start=st, goal=gl, theta0=th, speed0=sp)

    def load_worlds(self, cores, ncores, obstacles, nobs, start, goal, theta0, speed0):
        """mn_load_worlds for all n envs from padded tables laid out like worlds()'s; returns the first observations (float64)."""
        n, d, i = self.n, C.POINTER(C.c_double), C.POINTER(C.c_int32)
        cores = np.asarray(cores, np.float64); obstacles = np.asarray(obstacles, np.float64)
        f = lambda a: np.ascontiguousarray(a, np.float64)
        nc = np.ascontiguousarray(ncores, np.int32); no = np.ascontiguousarray(nobs, np.int32)
        cxy = f(cores[:, :, :2]); cw = np.ascontiguousarray(cores[:, :, 2] != 0, np.int32); gm = f(cores[:, :, 3])
        oxy = f(obstacles[:, :, :2]); orr = f(obstacles[:, :, 2])
        st = f(start); gl = f(goal); th = f(np.broadcast_to(theta0, (n,))); sp = f(np.broadcast_to(speed0, (n,)))
        p = lambda a, t: a.ctypes.data_as(t)
        assert self.L.mn_load_worlds(self.h, 0, n, p(nc, i), p(cxy, d), p(cw, i), p(gm, d), p(no, i), p(oxy, d), p(orr, d), p(st, d), p(gl, d),
                                     p(th, d), p(sp, d), self.ptr(self.obs[self.cur]), None) == 0, self.L.mn_last_error(self.h)
        return self.obs64()

    def set_state(self, state, ep_t):
        s = np.ascontiguousarray(state, np.float64); ep = np.ascontiguousarray(ep_t, np.int32)
        assert s.shape == (self.n, 6) and ep.shape == (self.n,)
        assert self.L.mn_set_state(self.h, 0, self.n, s.ctypes.data_as(C.POINTER(C.c_double)), ep.ctypes.data_as(C.POINTER(C.c_int32)), None) == 0

    def peek(self):
        out = np.zeros(self.n)
        assert self.L.mn_peek_next_double(self.h, 0, self.n, out.ctypes.data_as(C.POINTER(C.c_double))) == 0
        return out

    def close(self):
        self.L.mn_destroy(self.h)


def numpy_driver(L, n, **kw):
    def set_actions(buf, a):
        buf[:] = a
    d = Driver(L, n, lambda shape, dt: np.zeros(shape, dt), lambda a: a.ctypes.data_as(C.c_void_p), lambda a: a, **kw)
    d.set_actions = set_actions
    return d


def test_twin_exports_the_env_entry_points_with_the_header_signatures():
    assert os.path.exists(TWIN), "build it with `make -C oracle` (python -c 'import __graft_entry__ as g; g.build()')"
    L = bind(TWIN)                      # AttributeError if a symbol is missing
    p = _capi.MnParams()
    assert L.mn_default_params(C.byref(p)) == 0
    hip_defaults = {f[0]: getattr(p, f[0]) for f in _capi.MnParams._fields_ if not hasattr(getattr(p, f[0]), "__len__")}
    assert hip_defaults["num_cores"] == 8 and hip_defaults["N"] == 10 and hip_defaults["max_episode_steps"] == 1000
    assert L.mn_build_info() == 0
    h = C.c_void_p()
    assert L.mn_create(0, C.byref(p), C.byref(h)) == -1 and b"bad arguments" in L.mn_last_error(None)
    p.num_cores = 9
    assert L.mn_create(4, C.byref(p), C.byref(h)) == -1 and b"num_cores" in L.mn_last_error(None)      # same error contract


@pytest.mark.parametrize("fn", ["g2_trace_seed0_default.npz", "g2_trace_seed5_schedule.npz"])
def test_twin_replays_reference_trace(fn):
    """The reference's 1000-step golden trace (caller-side reset on done, incl. the curriculum schedule) through the
    twin's mn_* entry points."""
    z = np.load(os.path.join(G, fn))
    L = bind(TWIN)
    d = numpy_driver(L, 1, seeds=[int(z["seed"])])
    size = z["size"]
    if "sched_timesteps" in z.files:
        ts = np.ascontiguousarray(z["sched_timesteps"], np.int64); nc = np.ascontiguousarray(z["sched_num_cores"], np.int32)
        no = np.ascontiguousarray(z["sched_num_obstacles"], np.int32); md = np.ascontiguousarray(z["sched_min_dis"], np.float64)
        assert L.mn_set_schedule(d.h, 3, ts.ctypes.data_as(C.POINTER(C.c_int64)), nc.ctypes.data_as(C.POINTER(C.c_int32)),
                                 no.ctypes.data_as(C.POINTER(C.c_int32)), md.ctypes.data_as(C.POINTER(C.c_double)), 1.0) == 0
    else:
        d.set(num_cores=int(size[0]), num_obs=int(size[1]), min_start_goal_dis=float(size[2]))
    obs = d.reset()
    np.testing.assert_allclose(obs[0], z["obs0"], atol=1e-10)
    for t in range(len(z["actions"])):
        o, r, done, info = d.step([int(z["actions"][t])], d.set_actions)
        np.testing.assert_allclose(o[0], z["obs"][t], rtol=0, atol=2e-9)
        assert abs(r[0] - z["reward"][t]) < 1e-9 and bool(done[0]) == bool(z["done"][t]) and int(info[0]) == int(z["info"][t])
        s, ep, tot = d.state()
        assert ep[0] == z["ep_t"][t] and tot[0] == z["tot_t"][t]
        if done[0]:
            o = d.reset_done()
            np.testing.assert_allclose(o[0], z["reset_obs"][t], atol=1e-9)
    d.close()


@pytest.mark.gpu
def test_one_binding_two_libraries():
    """The same Driver over libmarinenav_hip.so (device buffers) and libmarinenav_cpu.so (host buffers): identical
    worlds and RNG positions bit for bit, float64 observations / rewards to 1e-9, done / info / counters exact, over
    free-running episodes with resets."""
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    n, T = 192, 150
    cpu = numpy_driver(bind(TWIN), n)

    def set_dev(buf, a):
        buf.copy_(torch.as_tensor(np.asarray(a, dtype=np.int32)))
    to_t = {np.float32: torch.float32, np.uint8: torch.uint8, np.int32: torch.int32}
    gpu = Driver(_capi.lib(), n, lambda shape, dt: torch.zeros(shape, dtype=to_t[dt], device="cuda:0"),
                 lambda t: C.c_void_p(t.data_ptr()), lambda t: (torch.cuda.synchronize(), t.cpu().numpy())[1])
    for d in (cpu, gpu):
        d.set(num_cores=8, num_obs=10, min_start_goal_dis=40.0)
    np.testing.assert_allclose(gpu.reset(), cpu.reset(), rtol=0, atol=1e-9)
    rng = np.random.RandomState(0)
    finished = 0
    for t in range(T):
        a = rng.randint(9, size=n)
        oc, rc, dc, ic = cpu.step(a, cpu.set_actions)
        og, rg, dg, ig = gpu.step(a, set_dev)
        assert np.array_equal(dc, dg) and np.array_equal(ic, ig)
        np.testing.assert_allclose(og, oc, rtol=0, atol=1e-5)      # chaotic flow amplifies libm-level differences over an episode
        np.testing.assert_allclose(rg, rc, rtol=0, atol=1e-5)
        finished += int(dc.sum())
        np.testing.assert_allclose(gpu.reset_done(), cpu.reset_done(), rtol=0, atol=1e-5)
        assert np.array_equal(gpu.peek(), cpu.peek())              # RNG streams in lock-step (bit-exact world generation)
        sc, sg = cpu.state(), gpu.state()
        assert np.array_equal(sc[1], sg[1]) and np.array_equal(sc[2], sg[2])
    assert finished > 20
    cpu.close(); gpu.close()
