"""What prioritized replay costs per gradient step and per vector step (csrc/per.hip; the weighted step of csrc/iqn_train.hip).

    python scripts/per_bench.py [--out profiles/per_bench.txt]

1. The gradient step: `IQNAgent.train_from_memory` with per = True (mn_per_sample + mn_iqn_train_grad_per + mn_iqn_train_adam + mn_per_update) against
   the uniform step as it ships (the batch drawn inside the fused launch), batch 32 and 256, a ring of 100 000 rows.
2. The three launches of the priority store alone -- append of one vector step's rows, sample, update -- at ring sizes 100 000 and 1 000 000.
3. The whole vector step in the reference cadence (80 envs, 20 gradient steps of batch 32 per vector step), uniform against prioritized.
Host clock around one device synchronisation per window (1, 2: the launches of a window are enqueued back to back) or per vector step (3); every shape warmed
up; medians of 5 alternating windows of ~0.3 s with min-max ranges -- the method of scripts/nstep_bench.py.  Nothing is promised.  Without a GPU the script fails."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
WINDOWS, WINDOW_S, EPS = 5, 0.3, 0.05
DEV = "cuda:0"


def _window(torch, fn, n, sync_each):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
        if sync_each:
            torch.cuda.synchronize()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n


def _compare(torch, lines, name, forms, sync_each=False):
    for _, fn in forms:
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    calls = [max(5, int(WINDOW_S / max(_window(torch, fn, 20, sync_each), 1e-7))) for _, fn in forms]
    t = [[] for _ in forms]
    for _ in range(WINDOWS):
        for k, (_, fn) in enumerate(forms):
            t[k].append(1e6 * _window(torch, fn, calls[k], sync_each))
    row, med = f"{name:44s}", []
    for k, (label, _) in enumerate(forms):
        us = sorted(t[k])
        med.append(statistics.median(us))
        row += f" | {label}: {med[-1]:8.1f} us [{us[0]:.1f}-{us[-1]:.1f}]"
    for k in range(1, len(forms)):
        row += f" | {forms[k][0]} / {forms[0][0]} = {med[k] / med[0]:.2f}x"
    lines.append(row)
    print(row, flush=True)
    return med


def _agent(torch, batch, ring, per, fill):
    from distributional_rl_navigation_amd.iqn.agent import IQNAgent
    ag = IQNAgent(26, 9, BATCH_SIZE=batch, BUFFER_SIZE=ring, device=DEV, seed=11, UPDATE_EVERY=1, learning_starts=0, per=per)
    g = torch.Generator(device=DEV).manual_seed(5)
    for lo in range(0, fill, 50_000):
        k = min(50_000, fill - lo)
        ag.memory.add_batch(torch.randn(k, 26, generator=g, device=DEV), torch.randint(0, 9, (k,), generator=g, device=DEV), torch.randn(k, generator=g, device=DEV),
                            torch.randn(k, 26, generator=g, device=DEV), (torch.rand(k, generator=g, device=DEV) < 0.05).float())
    return ag


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "per_bench.txt"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("per_bench: no GPU visible -- everything measured here is a HIP kernel")
    from distributional_rl_navigation_amd.marinenav_env.vec_env import VecMarineNavEnv
    lines = []
    say = lambda s: (lines.append(s), print(s, flush=True))
    say("# scripts/per_bench.py")
    say(f"{torch.cuda.get_device_name(0)}: medians of {WINDOWS} alternating windows of ~{WINDOW_S} s [min-max], host clock; 'call' = one gradient step (1), one launch (2), "
        "one vector step with a device synchronisation (3)")
    # 1. the gradient step
    for batch in (32, 256):
        uni, per = _agent(torch, batch, 100_000, False, 100_000), _agent(torch, batch, 100_000, True, 100_000)
        m = _compare(torch, lines, f"gradient step, batch {batch}, ring 100 000", [("uniform", uni.train_from_memory), ("prioritized", per.train_from_memory)])
        pr = per.memory.priority
        idx, w, taus = pr.sample(per.memory.size, batch, 0.4)
        ad = torch.rand(batch, device=DEV)
        ring = (per.memory.states, per.memory.actions, per.memory.rewards, per.memory.next_states, per.memory.dones)
        ft = per._fused_trainer()
        _compare(torch, lines, f"  its parts, batch {batch}", [("sample", lambda: pr.sample(per.memory.size, batch, 0.4)),
                                                                ("weighted step", lambda: ft.step_per(ring, idx, taus[0], taus[1], w)),
                                                                ("update", lambda: pr.update(idx, ad, 0.6, 1e-6))])
        say(f"  batch {batch}: prioritized - uniform = {m[1] - m[0]:+.1f} us per gradient step")
        del uni, per
        torch.cuda.empty_cache()
    # 2. the store's launches alone
    from distributional_rl_navigation_amd.iqn.priority import PriorityStore
    for ring in (100_000, 1_000_000):
        ps = PriorityStore(ring, DEV, 3)
        ps.append(0, ring)
        ps.update(torch.randint(0, ring, (1024,), device=DEV), torch.rand(1024, device=DEV) * 4, 0.6, 1e-6)
        for batch in (32, 256):
            idx = torch.randint(0, ring, (batch,), device=DEV)
            ad = torch.rand(batch, device=DEV)
            _compare(torch, lines, f"store alone, ring {ring}, batch {batch}", [("append 80 rows", lambda: ps.append(12_345, 80)), ("append 4096 rows", lambda: ps.append(12_345, 4096)),
                                                                               ("sample", lambda: ps.sample(ring, batch, 0.4)), ("update", lambda: ps.update(idx, ad, 0.6, 1e-6))])
        del ps
    # 3. the vector step in the reference cadence
    forms = []
    for per in (False, True):
        env = VecMarineNavEnv(80, seed=7, device=DEV, precision="f64")
        ag = _agent(torch, 32, 1_000_000, per, 20_000)
        ag.grad_steps_per_update = 20
        box = dict(obs=env.reset())

        def step(ag=ag, env=env, box=box):
            box["obs"] = ag.vec_step(env, box["obs"], EPS)[0]
        forms.append(("prioritized" if per else "uniform", step))
    m = _compare(torch, lines, "vector step, 80 envs, 20 x batch 32, ring 1 000 000", forms, sync_each=True)
    say(f"  prioritized - uniform = {m[1] - m[0]:+.1f} us per vector step = {(m[1] - m[0]) / 20:+.1f} us per gradient step")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
