"""What the greedy-on-mean and Double-IQN targets cost per gradient step and per vector step (`iqn_rule_fwdbwd_kernel<RULE>`, csrc/iqn_train.hip).

    python scripts/target_rule_bench.py [--out profiles/target_rule_bench.txt]

1. The gradient step: `IQNAgent.train_from_memory` under target_rule "max" (the plain step as it ships: the batch drawn inside the fused launch), "mean"
   (mn_iqn_sample for rows and two tau sets + mn_iqn_train_grad_rule + mn_iqn_train_adam), "double" (three tau sets; every workgroup runs the local weights over
   its next states first) and, for scale, the Munchausen step (the same two extra forwards per workgroup), batch 32 and 256, a ring of 100 000 rows.
2. The whole vector step in the reference cadence (80 envs, 20 gradient steps of batch 32 per vector step) under the same four.
Host clock around one device synchronisation per window (1: the launches of a window are enqueued back to back) or per vector step (2); every shape warmed up;
medians of 5 alternating windows of ~0.3 s with min-max ranges -- the method of scripts/munchausen_bench.py.  Nothing is promised.  Without a GPU the script fails."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
WINDOWS, WINDOW_S, EPS = 5, 0.3, 0.05
DEV = "cuda:0"
FORMS = (("max", dict()), ("mean", dict(target_rule="mean")), ("double", dict(target_rule="double")), ("munchausen", dict(munchausen=True)))


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
    row, med = f"{name:52s}", []
    for k, (label, _) in enumerate(forms):
        us = sorted(t[k])
        med.append(statistics.median(us))
        row += f" | {label}: {med[-1]:8.1f} us [{us[0]:.1f}-{us[-1]:.1f}]"
    lines.append(row)
    print(row, flush=True)
    return med


def _agent(torch, batch, ring, fill, **option):
    from distributional_rl_navigation_amd.iqn.agent import IQNAgent
    ag = IQNAgent(26, 9, BATCH_SIZE=batch, BUFFER_SIZE=ring, device=DEV, seed=11, UPDATE_EVERY=1, learning_starts=0, **option)
    g = torch.Generator(device=DEV).manual_seed(5)
    for lo in range(0, fill, 50_000):
        k = min(50_000, fill - lo)
        ag.memory.add_batch(torch.randn(k, 26, generator=g, device=DEV), torch.randint(0, 9, (k,), generator=g, device=DEV), torch.randn(k, generator=g, device=DEV),
                            torch.randn(k, 26, generator=g, device=DEV), (torch.rand(k, generator=g, device=DEV) < 0.05).float())
    return ag


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "target_rule_bench.txt"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("target_rule_bench: no GPU visible -- everything measured here is a HIP kernel")
    from distributional_rl_navigation_amd.marinenav_env.vec_env import VecMarineNavEnv
    lines = []
    say = lambda s: (lines.append(s), print(s, flush=True))
    say("# scripts/target_rule_bench.py")
    say(f"{torch.cuda.get_device_name(0)}: medians of {WINDOWS} alternating windows of ~{WINDOW_S} s [min-max], host clock; 'call' = one gradient step (1), "
        "one vector step with a device synchronisation (2)")
    # 1. the gradient step
    for batch in (32, 256):
        agents = [(label, _agent(torch, batch, 100_000, 100_000, **option)) for label, option in FORMS]
        m = _compare(torch, lines, f"gradient step, batch {batch}, ring 100 000", [(label, ag.train_from_memory) for label, ag in agents])
        say(f"  batch {batch}, against max: " + ", ".join(f"{label} {m[k] - m[0]:+.1f} us" for k, (label, _) in enumerate(FORMS) if k))
        del agents
        torch.cuda.empty_cache()
    # 2. the vector step in the reference cadence
    forms = []
    for label, option in FORMS:
        env = VecMarineNavEnv(80, seed=7, device=DEV, precision="f64")
        ag = _agent(torch, 32, 1_000_000, 20_000, **option)
        ag.grad_steps_per_update = 20
        box = dict(obs=env.reset())

        def step(ag=ag, env=env, box=box):
            box["obs"] = ag.vec_step(env, box["obs"], EPS)[0]
        forms.append((label, step))
    m = _compare(torch, lines, "vector step, 80 envs, 20 x batch 32, ring 1 000 000", forms, sync_each=True)
    say("  against max: " + ", ".join(f"{label} {m[k] - m[0]:+.1f} us per vector step = {(m[k] - m[0]) / 20:+.1f} us per gradient step" for k, (label, _) in enumerate(FORMS) if k))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
