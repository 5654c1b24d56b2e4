"""DQN learner alone: back-to-back gradient steps of the fused HIP step (csrc/dqn_train.hip, batch drawn in the launch) against eager
DQNAgent.train, on a 100 000-row ring filled from a rollout of the HIP env, B = 32 and 256, one process, warmed up, timed with a synchronize.
usage: python scripts/dqn_learner_bench.py [reps]"""
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch
from distributional_rl_navigation_amd.dqn import DQNAgent
from distributional_rl_navigation_amd.marinenav_env.vec_env import VecMarineNavEnv

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 2000
dev = "cuda:0"
env = VecMarineNavEnv(4096, seed=0, device=dev)
filler = DQNAgent(device=dev, buffer_size=100_000, seed=1)
obs = env.reset()
while len(filler.memory) < 100_000:
    a = filler.act_batch(obs, 1.0)
    nxt, r, d, _ = env.step(a)
    filler.memory.add_vector_step(obs, a, r, nxt, d)
    obs = env.reset_done()
env.close()
m0 = filler.memory
for B in (32, 256):
    res = {}
    for fused in (True, False):
        ag = DQNAgent(device=dev, buffer_size=100_000, batch_size=B, seed=1, fused_train=fused)
        for dst, src in zip((ag.memory.states, ag.memory.actions, ag.memory.rewards, ag.memory.next_states, ag.memory.dones),
                            (m0.states, m0.actions, m0.rewards, m0.next_states, m0.dones)):
            dst.copy_(src)
        ag.memory.size = m0.size
        n = reps if fused else max(50, reps // 20)
        for _ in range(20):
            ag.train()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            ag.train()
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / n
        res[fused] = dt
        print(f"B {B:3d} {'fused' if fused else 'eager'}: {1e6 * dt:8.2f} us per step  {1 / dt:9.0f} steps/s  ({n} steps)", flush=True)
    print(f"B {B:3d} fused speed-up over eager: {res[False] / res[True]:.1f}x", flush=True)
