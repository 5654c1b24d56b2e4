"""The field pilot on the CPU: whole episodes of the 30 evaluation worlds under tests/pilot_host.hip --episodes (the rule of csrc/mn_pilot_body.h on
the what-if step, fields from tests/time_field_host.hip), per horizon.  Writes profiles/pilot_host.txt: the success count and the min / median / max
of time / T(start) over the successful episodes.  The default horizon of maps.pilot_times / pilot_map is the least H of 1..6 with the most successes
at 128 x 128, clearance 0 (tests/test_pilot_cpu.py holds the code to this file).  No GPU is used.

  python scripts/pilot_host_episodes.py [--out profiles/pilot_host.txt]"""
import argparse
import os
import pathlib
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pilot_host.txt"))
    args = ap.parse_args()
    import test_pilot_cpu as PC
    d = pathlib.Path(tempfile.mkdtemp(prefix="pilot_host_"))
    pilot_exe, tf_exe = PC.build_host(d), PC.TF.build_host(d)
    worlds = PC.R.eval_worlds()
    lines = ["# tests/pilot_host.hip --episodes on the 30 worlds of tests/golden/eval_config_seed3.json (scripts/pilot_host_episodes.py); host arithmetic, no GPU",
             "# time / T(start): steps * N * dt over the field's value at the start cell, successful episodes only"]
    cases = [(H, 128, 0.0) for H in range(1, 7)] + [(8, 128, 0.0)] + [(H, 64, 0.0) for H in (1, 2, 3, 4)] + [(H, 128, 0.5) for H in (1, 2, 3, 4)]
    for H, n, clearance in cases:
        success, steps, ratio = PC.host_episodes(pilot_exe, tf_exe, d, worlds, H, nx=n, ny=n, clearance=clearance)
        r = ratio[success]
        stats = f"min {r.min():.2f} median {np.median(r):.2f} max {r.max():.2f}" if len(r) else "min - median - max -"
        failed = ", failed: " + " ".join(str(k) for k in np.flatnonzero(~success)) if (~success).any() else ""
        lines.append(f"H={H} grid={n}x{n} clearance={clearance:.1f}: {int(success.sum())}/30 successes, time / T(start) {stats}{failed}")
        print(lines[-1], flush=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
