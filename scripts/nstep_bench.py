"""What the n-step window costs per vector step in its three forms: the torch ops (`ReplayBuffer.use_nstep_kernel = False`: ~20 dependent launches), the one
launch `mn_replay_append_nstep` (csrc/replay.hip; the default), and -- as the floor -- n_step = 1, where the step kernel appends by itself (`mn_step_append`).

    python scripts/nstep_bench.py [--out profiles/nstep_bench.txt] [--envs 80,4096,65536] [--n-step 3] [--mode reference]

Per env count: the collect phase alone (act_batch, mn_step, the append, mn_reset_done: `IQNAgent.vec_collect` + `vec_finish`) and the whole vector step
(`vec_step`: the same plus the cadence's gradient steps -- 20 of batch 32 at 80 envs, the reference-budget cadence; one of batch 256 otherwise, the
learner-budget default).  One agent and one env per form, equal seeds, all three in one process; eps = 0.05.  Before timing the two n-step forms run the same
steps and their rings, windows and parameters are compared for equality.
Host clock around a synchronise, one device synchronisation per vector step; every shape warmed up; medians of 5 alternating windows of ~0.3 s with
min-max ranges.  Nothing is promised.  The last lines say whether the kernel form's median at 4 096 envs lies below the torch form's with ranges that do not
overlap: the condition under which it stays the default.  Without a GPU the script fails.
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
WINDOWS, WINDOW_S, CHECK_STEPS, EPS = 5, 0.3, 6, 0.05
DEV = "cuda:0"


def _window(torch, fn, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
        torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n


def _compare(torch, lines, name, forms):
    """`forms`: [(label, fn)] timed in alternating windows; one row with each form's median and range and every form over the first.  Returns the windows' times (us) per form."""
    for _, fn in forms:
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    calls = [max(3, int(WINDOW_S / max(_window(torch, fn, 3), 1e-6))) for _, fn in forms]
    t = [[] for _ in forms]
    for _ in range(WINDOWS):
        for k, (_, fn) in enumerate(forms):
            t[k].append(1e6 * _window(torch, fn, calls[k]))
    row, med = f"{name:36s}", []
    for k, (label, _) in enumerate(forms):
        us = sorted(t[k])
        med.append(statistics.median(us))
        row += f" | {label}: {med[-1]:9.1f} us [{us[0]:.1f}-{us[-1]:.1f}], {calls[k]} calls/window"
    for k in range(1, len(forms)):
        row += f" | {forms[k][0]} / {forms[0][0]} = {med[k] / med[0]:.2f}x"
    lines.append(row)
    print(row, flush=True)
    return t


class Lines(list):
    """The report: every line goes to the file as it is added, so a run that is cut short leaves what it measured."""

    def __init__(self, path):
        super().__init__()
        self.path = path
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)

    def append(self, line):
        super().append(line)
        with open(self.path, "w") as f:
            f.write("\n".join(self) + "\n")


class Form:
    """One agent on one env of `n` rows: n_step-step returns in `mode`, the window by the kernel or by torch ops."""

    def __init__(self, torch, n, n_step, mode, kernel):
        from distributional_rl_navigation_amd.iqn.agent import IQNAgent
        from distributional_rl_navigation_amd.marinenav_env.vec_env import VecMarineNavEnv
        small = n <= 80
        self.torch = torch
        self.env = VecMarineNavEnv(n, seed=7, device=DEV, precision="f64")
        self.agent = IQNAgent(26, 9, n_step=n_step, n_step_mode=mode, BATCH_SIZE=32 if small else 256, BUFFER_SIZE=max(16_384, 8 * n), device=DEV, seed=11,
                              UPDATE_EVERY=1, learning_starts=0)
        self.agent.grad_steps_per_update = 20 if small else 1
        self.agent.memory.use_nstep_kernel = kernel
        self.obs = self.env.reset()

    def collect(self):
        st = self.agent.vec_collect(self.env, self.obs, EPS)
        self.obs = self.agent.vec_finish(self.env, st)

    def step(self):
        self.obs = self.agent.vec_step(self.env, self.obs, EPS)[0]

    def close(self):
        self.torch.cuda.synchronize()
        self.env.close()


def _check_equal(torch, a, b, where):
    torch.cuda.synchronize()
    x, y = a.agent.memory, b.agent.memory
    same = (x.size, x.ptr, x._hist["count"]) == (y.size, y.ptr, y._hist["count"])
    for k in ("states", "next_states", "actions", "rewards", "dones"):
        same = same and torch.equal(getattr(x, k), getattr(y, k))
    same = same and all(torch.equal(x._hist[k], y._hist[k]) for k in x._hist if k != "count")
    same = same and all(torch.equal(p, q) for p, q in zip(a.agent.qnetwork_local.parameters(), b.agent.qnetwork_local.parameters()))
    if not same:
        raise SystemExit(f"nstep_bench: {where}: the kernel form and the torch form differ")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nstep_bench.txt"))
    ap.add_argument("--envs", default="80,4096,65536")
    ap.add_argument("--n-step", type=int, default=3)
    ap.add_argument("--mode", default="reference", choices=("reference", "episode"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("nstep_bench: no GPU visible -- the forms compared are HIP kernels and device-side torch ops, there is nothing to measure without one")
    lines = Lines(args.out)
    lines.append(f"# scripts/nstep_bench.py --envs {args.envs} --n-step {args.n_step} --mode {args.mode}")
    lines.append(f"{torch.cuda.get_device_name(0)}: medians of {WINDOWS} alternating windows of ~{WINDOW_S} s [min-max], host clock, one device synchronisation per vector "
                 f"step; 'call' = one vector step; eps = {EPS}; n_step = {args.n_step}, nstep_mode = {args.mode}; before timing, ring, window and parameters of the torch "
                 f"and the kernel form after {CHECK_STEPS} vector steps were compared for equality")
    verdict = None
    for n in (int(v) for v in args.envs.split(",")):
        tw, kn, fl = Form(torch, n, args.n_step, args.mode, False), Form(torch, n, args.n_step, args.mode, True), Form(torch, n, 1, "reference", True)
        for _ in range(CHECK_STEPS):
            tw.step(); kn.step(); fl.step()
        _check_equal(torch, tw, kn, f"{n} envs")
        grad = f"{tw.agent.grad_steps_per_update} x batch {tw.agent.BATCH_SIZE}"
        forms = lambda what: [("torch window", getattr(tw, what)), ("kernel", getattr(kn, what)), ("n_step = 1 (mn_step_append)", getattr(fl, what))]
        t = _compare(torch, lines, f"collect phase, {n} envs", forms("collect"))
        _compare(torch, lines, f"vector step, {n} envs, {grad}", forms("step"))
        if n == 4096:
            verdict = (statistics.median(t[1]) < statistics.median(t[0]) and max(t[1]) < min(t[0]), statistics.median(t[0]), statistics.median(t[1]))
        for f in (tw, kn, fl):
            f.close()
        del tw, kn, fl
        torch.cuda.empty_cache()
    if verdict is None:
        lines.append("4 096 envs not measured in this run: no verdict on the default")
    else:
        lines.append(f"collect phase at 4 096 envs: kernel {verdict[2]:.1f} us, torch window {verdict[1]:.1f} us; the kernel form's windows "
                     + ("all lie below the torch form's: the kernel stays the default (ReplayBuffer.use_nstep_kernel = True)" if verdict[0] else
                        "do NOT all lie below the torch form's: the kernel form should be opt-in"))


if __name__ == "__main__":
    main()
