"""The few-rows act kernel (`sp::iqn_act_few_kernel`, csrc/iqn_act_few.h) exists in the code object once, within the budget it is written for: no scratch, no
spilled registers, at most 256 registers (two of its wavefronts on a SIMD), and a few KB of STATIC LDS only -- it is launched without the 154-KB dynamic image
of the forms it stands in for.  Read from the compile remarks, as tests/test_kernel_resources_cpu.py does; and the C ABI's side of it.  No GPU."""
import os
import re
import sys

sys.path.insert(0, os.path.dirname(__file__))
from test_kernel_resources_cpu import CSRC, ROOT, _pick, _usage      # noqa: E402


def test_few_rows_kernel_resources():
    u = _usage("iqn_act.hip", ["-ffp-contract=fast", "-fno-slp-vectorize"])
    few = _pick(u, "iqn_act_few_kernel")
    assert len(few) == 1, list(few)
    (k, v), = few.items()
    assert v["ScratchSize"] == 0 and v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0, (k, v)
    assert v["VGPRs"] + v.get("AGPRs", 0) <= 256, (k, v)
    assert 0 < v["LDS Size"] <= 8192, (k, v)      # the two feature buffers and the tau-mean hand-off
    host = open(os.path.join(CSRC, "iqn_act.hip")).read()
    assert re.search(r"hipLaunchKernelGGL\(sp::iqn_act_few_kernel, dim3\(few_grid\(c, n\)\), dim3\(64 \* sp::FEW_WAVES\), 0, s,", host)      # no dynamic LDS
    assert "iqn_act_few_kernel" not in "".join(k for k in u if "iqn_qvals_split_kernel" in k)      # a kernel of its own, not a form of the split kernel


def test_default_threshold_is_one_number():
    from distributional_rl_navigation_amd.iqn.fused_act import ActContext
    src = open(os.path.join(ROOT, "include", "marinenav_hip.h")).read()
    m = re.search(r"#define MN_IQN_FEW_ROWS_MAX_DEFAULT (-?\d+)\b", src)
    assert m and int(m.group(1)) == ActContext.FEW_ROWS_MAX_DEFAULT
    assert ActContext.FEW_ROWS_ALWAYS == 2 ** 31 - 1
