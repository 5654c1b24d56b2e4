"""Times the minimum-time-to-goal field launch on one MI355X and writes profiles/time_field_bench.txt.

    python scripts/time_field_bench.py [--out FILE] [--reps 5] [--inner 3] [--host-program EXE]

Medians of `--reps` timed windows of `--inner` calls after a warm-up window, all cases alternating in one process; wall time per call of
VecMarineNavEnv.time_field (output and workspace allocation from torch's cache included), synchronised, with the range.  Cases, on the worlds of
tests/golden/eval_config_seed3.json with the default speed and clearance 0: 1 field (world 10) and the 30 worlds at 64 x 64; the same at 128 x 128;
300 fields at 32 x 32 (the 30 worlds ten times).  Beside each case the sweeps its fields ran.  For scale, the seconds tests/time_field_host.hip -- the
same body on one CPU core, row-major in-place sweeps -- reports for world 10 at 128 x 128 (built here with hipcc --cuda-host-only, or --host-program
EXE; left out if there is no compiler).  Nothing is asserted."""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
G = os.path.join(ROOT, "tests", "golden")


def host_seconds(exe, params, world, nx, ny):
    """What the host program reports for one field of `world` (a load_worlds dict), and its sweeps; a record as tests/test_time_field_cpu.py writes it."""
    import struct

    import numpy as np
    rec = np.zeros(1, dtype=np.dtype([("nc", "<i4"), ("no", "<i4"), ("cores", "<f8", (8, 3)), ("obst", "<f8", (10, 3)), ("start", "<f8", (2,)),
                                      ("goal", "<f8", (2,))]))
    c, o = np.asarray(world["cores"], dtype=np.float64).reshape(-1, 4), np.asarray(world["obstacles"], dtype=np.float64).reshape(-1, 3)
    rec["nc"][0], rec["no"][0] = len(c), len(o)
    rec["cores"][0, :len(c)] = np.stack((c[:, 0], c[:, 1], np.where(c[:, 2] != 0, c[:, 3], -c[:, 3])), axis=1)
    rec["obst"][0, :len(o)] = o
    rec["start"][0], rec["goal"][0] = world["start"], world["goal"]
    with tempfile.TemporaryDirectory() as d:
        fin, fout = os.path.join(d, "in"), os.path.join(d, "out")
        with open(fin, "wb") as f:
            f.write(struct.pack("<4i2d", 1, nx, ny, 4 * (nx + ny), 0.0, 0.0))
            f.write(bytes(params))
            f.write(rec.tobytes())
        subprocess.run([exe, fin, fout], check=True, timeout=600)
        raw = open(fout, "rb").read()
    nc = nx * ny
    sweeps = int(np.frombuffer(raw, dtype="<i4", count=1, offset=9 * nc + 4)[0])
    return float(np.frombuffer(raw[-8:], dtype="<f8")[0]), sweeps


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "time_field_bench.txt"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--inner", type=int, default=3)
    ap.add_argument("--host-program", default=None)
    ap.add_argument("--device", default="cuda:0")
    args = ap.parse_args(argv)
    import torch
    from distributional_rl_navigation_amd.marinenav_env.vec_env import VecMarineNavEnv
    with open(os.path.join(G, "eval_config_seed3.json")) as f:
        cfg = json.load(f)
    worlds = [VecMarineNavEnv.world_from_eval_config(cfg[f"env_{k}"]) for k in range(len(cfg))]
    env = VecMarineNavEnv(len(worlds), device=args.device, precision="f64")
    env.load_worlds(worlds)
    dev, nw = env.device, len(worlds)
    all30 = torch.arange(nw, dtype=torch.int32, device=dev)
    many = torch.arange(300, dtype=torch.int32, device=dev) % nw
    cases = [("1 field (world 10), 64 x 64", 10, 64), ("30 fields, 64 x 64", all30, 64), ("1 field (world 10), 128 x 128", 10, 128),
             ("30 fields, 128 x 128", all30, 128), ("300 fields, 32 x 32", many, 32)]
    times, sweeps = [[] for _ in cases], []
    for _, which, n in cases:      # the sweep counts, once, outside every window
        _, _, status, sw = env.time_field(which, n, n)
        assert int(status.max()) == 0, status.tolist()
        sweeps.append((int(sw.min()), int(sw.max())))
    for rep in range(args.reps + 1):      # the first round warms up
        for i, (_, which, n) in enumerate(cases):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.inner):
                env.time_field(which, n, n)
            torch.cuda.synchronize()
            if rep:
                times[i].append((time.perf_counter() - t0) / args.inner)
    lines = [f"device: {torch.cuda.get_device_name(0)}; medians of {args.reps} windows of {args.inner} calls after a warm-up window, the cases alternating in one "
             "process; wall time per call, synchronised",
             f"{'case':<40}{'median ms':>12}{'min':>10}{'max':>10}{'ms per field':>14}{'sweeps':>12}"]
    for (name, which, _), t, (s0, s1) in zip(cases, times, sweeps):
        med = sorted(t)[len(t) // 2]
        nf = 1 if isinstance(which, int) else int(which.shape[0])
        lines.append(f"{name:<40}{med * 1e3:>12.3f}{min(t) * 1e3:>10.3f}{max(t) * 1e3:>10.3f}{med / nf * 1e3:>14.4f}{f'{s0}..{s1}':>12}")
    exe = args.host_program
    tmp = None
    if exe is None and os.path.exists("/opt/rocm/bin/hipcc"):
        tmp = tempfile.TemporaryDirectory()
        exe = os.path.join(tmp.name, "time_field_host")
        csrc = os.path.join(ROOT, "distributional_rl_navigation_amd", "csrc")
        subprocess.run(["/opt/rocm/bin/hipcc", "--cuda-host-only", "-O2", "-std=c++17", "-ffp-contract=off", "-I" + os.path.join(ROOT, "include"), "-I" + csrc,
                        "-o", exe, os.path.join(ROOT, "tests", "time_field_host.hip")], check=True, timeout=900)
    if exe:
        runs = [host_seconds(exe, env.params, worlds[10], 128, 128) for _ in range(3)]
        lines.append(f"for scale: the host program (one CPU core, row-major in-place sweeps), world 10 at 128 x 128: {sorted(r[0] for r in runs)[1] * 1e3:.1f} ms "
                     f"(median of 3 runs), {runs[0][1]} sweeps")
    text = "\n".join(lines)
    print(text, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    env.close()


if __name__ == "__main__":
    main()
