"""The two act kernel forms that evaluate only the listed rows (`iqn_qvals_split_kernel<.., LATE, ROWS = true>`, csrc/iqn_act.hip FORMS) exist in the
code object and hold the budget of the forms they stand in for: no scratch, <= 208 registers (two wavefronts per SIMD leave the 96 the reset kernel
beside them is compiled for).  Read from the compile remarks, as tests/test_kernel_resources_cpu.py does; no GPU."""
import os
import sys

sys.path.insert(0, os.path.dirname(__file__))
from test_kernel_resources_cpu import _pick, _usage      # noqa: E402


def test_listed_row_forms_exist_without_scratch():
    u = _usage("iqn_act.hip", ["-ffp-contract=fast", "-fno-slp-vectorize"])
    plain = _pick(u, "iqn_qvals_split_kernel", "Lb0ELb0ELi8ELb0ELb1E")      # <QUANT = false, SHARED = false, 8 waves, LATE = false, ROWS = true>
    late = _pick(u, "iqn_qvals_split_kernel", "Lb0ELb0ELi8ELb1ELb1E")       # <.., LATE = true, ROWS = true>
    assert len(plain) == 1 and len(late) == 1
    for k, v in {**plain, **late}.items():
        assert v["ScratchSize"] == 0 and v["VGPRs"] + v.get("AGPRs", 0) <= 208, (k, v)
    prep = _pick(u, "iqn_split_prep_kernel")      # the launch that builds the list
    for k, v in prep.items():
        assert v["ScratchSize"] == 0, (k, v)
