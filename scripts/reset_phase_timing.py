"""Where ONE episode reset goes, phase by phase: s_memtime stamps of the reset wavefront of workgroup 0 inside mn_reset_env (MN_RTICK, csrc/mn_reset_body.h),
from the ABLATION build (libmarinenav_hip_ablation.so -- the only build with the stamps; the shipped library has none).  The env runs the training loop's
shape (float64 env kernels, random actions, a few hundred episode ends per vector step) and resets through the queue-driven mn_reset_kernel, which inlines
the same body as the preparation launch's reset blocks.   python scripts/reset_phase_timing.py [n_envs] [vector steps]"""
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from distributional_rl_navigation_amd import _capi

ABL = os.path.join(os.path.dirname(_capi.LIB_PATH), "libmarinenav_hip_ablation.so")
L = C.CDLL(ABL)
assert L.mn_build_info() == 1
for name, res, args in _capi.SIGNATURES:
    fn = getattr(L, name); fn.restype, fn.argtypes = res, args
_capi._lib = L
from distributional_rl_navigation_amd.marinenav_env.vec_env import VecMarineNavEnv

n = int(sys.argv[1]) if len(sys.argv) > 1 else 65536
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 400
env = VecMarineNavEnv(n, seed=0, device="cuda:0", precision="f64")
env.set_attrs(num_cores=8, num_obs=10, min_start_goal_dis=40.0)
env.reset()
g = torch.Generator(device="cuda:0"); g.manual_seed(0)
acts = [torch.randint(0, 9, (n,), device="cuda:0", dtype=torch.int32, generator=g) for _ in range(64)]
for t in range(300):      # steady state: episodes at all ages
    env.step(acts[t % 64]); env.reset_done()
torch.cuda.synchronize()
buf = (C.c_ulonglong * 8)()
assert L.mn_debug_reset_phases(buf, 1) == 0
ends = 0
for t in range(steps):
    env.step(acts[t % 64])
    ends += env.last_done_count()
    env.reset_done()
torch.cuda.synchronize()
assert L.mn_debug_reset_phases(buf, 0) == 0
v = [int(x) for x in buf]
k = max(v[7], 1)
names = ["RNG block in", "start / goal", "cores", "obstacles", "pose draw, world + RNG write-back", "compact tables, start velocity", "first observation"]
print(f"{n} envs, {steps} vector steps, {ends / steps:.0f} episode ends per step; workgroup 0 stamped {v[7]} resets")
tot = sum(v[:7])
for i, name in enumerate(names):
    print(f"  {name:36s} {v[i] / k:9.1f} ticks / reset  {100.0 * v[i] / max(tot, 1):5.1f} %")
print(f"  {'all phases':36s} {tot / k:9.1f} ticks / reset")
