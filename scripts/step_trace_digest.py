"""Digest of a rocprofv3 --kernel-trace CSV (…_kernel_trace.csv) of a bench.py run: the last WINDOW vector steps of the trace -- a vector step starts where
its step kernel starts -- with the step-start-to-step-start time and, per kernel, launches per step and the mean / median / p10 / p90 / sd of its duration.

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python bench.py --gpus 1 --steps 200 --warmup 20 --no-clock-probe --no-learner-only
    python scripts/step_trace_digest.py DIR/**/*_kernel_trace.csv [window = 150]
"""
import csv
import re
import sys

import numpy as np


def short(name):
    name = re.sub(r"\(anonymous namespace\)::", "", name)
    name = re.sub(r"^void ", "", name)
    return re.sub(r"\(.*$", "", name)[:60]


rows = [(r["Kernel_Name"], int(r["Start_Timestamp"]), int(r["End_Timestamp"])) for r in csv.DictReader(open(sys.argv[1]))]
window = int(sys.argv[2]) if len(sys.argv) > 2 else 150
rows.sort(key=lambda r: r[1])
steps = [i for i, r in enumerate(rows) if "mn_step_kernel" in r[0]]
assert len(steps) > window + 1, f"only {len(steps)} step kernels in the trace"
first, last = steps[-window - 1], steps[-1]
span = rows[first:last]
t0, t1 = rows[first][1], rows[last][1]
print(f"window: {window} vector steps, {(t1 - t0) / window / 1e3:.1f} us per step (step start to step start)")
by = {}
for name, s, e in span:
    by.setdefault(short(name), []).append((e - s) / 1e3)
for name, d in sorted(by.items(), key=lambda kv: -sum(kv[1])):
    d = np.array(d)
    print(f"  {name:60s} n/step {len(d) / window:5.2f}  mean {d.mean():7.2f} us  median {np.median(d):7.2f}  p10 {np.percentile(d, 10):7.2f}  "
          f"p90 {np.percentile(d, 90):7.2f}  sd {d.std():5.2f}  per step {d.sum() / window:7.2f} us")
# time with some kernel running: union of the intervals
busy, end = 0, t0
for name, s, e in span:
    s, e = max(s, end), min(e, t1)
    if e > s:
        busy += e - s
        end = e
print(f"  some kernel running {busy / window / 1e3:.1f} us per step, none {(t1 - t0 - busy) / window / 1e3:.1f} us")
