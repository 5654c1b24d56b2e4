"""The episode kernels' observation-noise instantiations, cross-compiled for gfx950 (hipcc's kernel-resource-usage remarks): no scratch, at most 256
vector registers, the LDS a CU has; and the instantiations WITHOUT noise are as many as they were, with the figures DESIGN records for the parent
(VGPRs, AGPRs, SGPRs, LDS, scratch): the NOISE flag costs the existing kernels nothing."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "distributional_rl_navigation_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
CU_LDS = 163840
STEP = ["-ffp-contract=off", "-fno-slp-vectorize"]                      # the Makefile's flags of mn_rollout.o / mn_rollout_dqn.o
IQN = ["-ffp-contract=fast-honor-pragmas", "-fno-slp-vectorize"]        # ... and of mn_rollout_iqn.o


def usage(src, flags):
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-I../../include", "-I.", "--cuda-device-only",
           "-Rpass-analysis=kernel-resource-usage", "-c", "-o", "/dev/null", *flags, src]
    r = subprocess.run(cmd, cwd=CSRC, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    out, cur = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            cur = out.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+)", line)
        if m and cur is not None:
            cur[m.group(1).strip()] = int(m.group(2))
    return out


def figures(v):
    return (v["VGPRs"], v["AGPRs"], v["TotalSGPRs"], v["LDS Size"], v["ScratchSize"])


@pytest.fixture(scope="module")
def kernels():
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    return {"policy": usage("mn_rollout.hip", STEP), "dqn": usage("mn_rollout_dqn.hip", STEP), "iqn": usage("mn_rollout_iqn.hip", IQN)}


def test_noisy_instantiations_have_no_scratch_and_fit(kernels):
    iqn = {k: v for k, v in kernels["iqn"].items() if "mn_rollout_iqn_noise_kernel" in k}
    dqn = {k: v for k, v in kernels["dqn"].items() if "mn_rollout_dqn_noise_kernel" in k}
    pol = {k: v for k, v in kernels["policy"].items() if "mn_rollout_policy_kernel" in k and "ELb1EEE" in k}      # <M, PARITY, 8, NOISE = true>
    assert len(iqn) == 2 and len(dqn) == 2          # both precisions
    assert len(pol) == 1 and "IdLb1ELi8ELb1E" in next(iter(pol))      # float64 handles only: the mixed-precision form is refused (DESIGN)
    iqn_dynamic = (37840 + 208 + 64) * 4            # the acting weight image + one feature buffer + the clean and the perceived row (IqnLds<false, true>)
    dqn_dynamic = 126912                            # mn_dqn_image_floats() * 4: the weight image (tests/test_rollout_dqn_cpu.py)
    for group, dynamic in ((iqn, iqn_dynamic), (dqn, dqn_dynamic), (pol, 0)):
        for k, v in group.items():
            assert v["ScratchSize"] == 0, (k, v)
            assert v["VGPRs"] <= 256 and v["VGPRs Spill"] == 0, (k, v)
            assert v["LDS Size"] + dynamic <= CU_LDS, (k, v)


def test_instantiations_without_noise_are_what_they_were(kernels):
    """Counts and figures (VGPRs, AGPRs, SGPRs, static LDS, scratch) of the parent commit's build, as DESIGN records them."""
    iqn = sorted(figures(v) for k, v in kernels["iqn"].items() if "mn_rollout_iqn_kernel" in k)
    dqn = sorted(figures(v) for k, v in kernels["dqn"].items() if "mn_rollout_dqn_kernel" in k)
    pol = sorted(figures(v) for k, v in kernels["policy"].items() if "mn_rollout_policy_kernel" in k and "ELb0EEE" in k)
    assert iqn == sorted([(256, 104, 106, 1920, 0), (256, 102, 106, 1600, 0)])
    assert dqn == sorted([(227, 56, 106, 3968, 0), (221, 56, 106, 3648, 0)])
    assert pol == sorted([(248, 0, 106, 2816, 0), (246, 0, 106, 2496, 0)])
    # every instantiation of the three episode kernels is one of the above or a noisy one: nothing else appeared
    assert len([k for k in kernels["iqn"] if "mn_rollout_iqn" in k]) == 4 and len([k for k in kernels["dqn"] if "mn_rollout_dqn" in k]) == 4
    assert len([k for k in kernels["policy"] if "mn_rollout_policy_kernel" in k]) == 3
