"""The greedy-on-mean forward / backward kernels (`iqn_rule_fwdbwd_kernel<RULE>`, csrc/iqn_train.hip) are held to the budget of the gradient step's other forms:
NO scratch and at most 256 registers, checked where they are compiled (hipcc cross-compiles gfx950 without a GPU; `-Rpass-analysis=kernel-resource-usage`).
Their name keeps them out of the three `iqn_train_fwdbwd<*, *>` instantiations and the one `iqn_munch_fwdbwd_kernel` the other resource tests count."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "distributional_rl_navigation_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
COMMON = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-I../../include", "-I.", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c", "-o", "/dev/null"]


def _usage(source, flags):
    """{mangled kernel name: {field: int}} from hipcc's resource-usage remarks, compiled with the Makefile's flags for that file."""
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    r = subprocess.run([HIPCC] + COMMON + flags + [source], cwd=CSRC, capture_output=True, text=True, timeout=900)
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


def test_target_rule_kernels_have_no_scratch():
    u = _usage("iqn_train.hip", ["-ffp-contract=off", "-mllvm", "-disable-machine-licm"])
    ks = {k: v for k, v in u.items() if "iqn_rule_fwdbwd_kernel" in k}
    assert len(ks) == 2, list(u)      # RULE = 1 (mean), 2 (double)
    for k, v in ks.items():
        print(k, v)
        assert v["ScratchSize"] == 0 and v["VGPRs"] + v.get("AGPRs", 0) <= 256, (k, v)
        assert v["LDS Size"] == next(w for n, w in u.items() if "iqn_munch_fwdbwd_kernel" in n)["LDS Size"]      # static LDS; the dynamic part is LDS_BYTES for every form
    assert len([k for k in u if "iqn_train_fwdbwd" in k]) == 3      # <XCHG, FUSED> = <false, false>, <false, true>, <true, true>, as before
    assert len([k for k in u if "iqn_munch_fwdbwd_kernel" in k]) == 1
