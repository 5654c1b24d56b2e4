"""How the episode-reset body (csrc/mn_reset_body.h) is compiled into the launches that run it alone on the chip, without a GPU: hipcc cross-compiles gfx950,
and the resource remarks and the assembly of `mn_prep_reset_kernel` (csrc/mn_prep_reset.hip) and `mn_reset_kernel` (csrc/mn_reset.hip) are read.

A reset is ONE wavefront's dependent chain, so the launch lasts as long as that chain has instructions: what is pinned is that the chain does not grow back.
  * no scratch in either kernel, both precisions;
  * the preparation launch keeps the waves per SIMD it had (three with float64 env kernels at 132 registers, four mixed at 125) and at most 8 KB of LDS per workgroup;
  * `mn_prep_reset_kernel<double, true>`, the training loop's, has fewer instructions and fewer v_readlane_b32 + v_writelane_b32 (broadcasts, and the moves of
    scalar registers spilled to a vector register) than before the body's short-chain form: 5 687 instructions and 521 lane moves then, counted by
    this file's own rule with the same compiler (ROCm's hipcc, -O3, the Makefile's flags for the file); 5 653 and 493 with it.  The broadcasts of the accepted
    objects ADD lane moves (they replace LDS reads), so the count only falls while the tail's array pointers come from memory instead of spilled kernel arguments
    (mn_reset_env's TAIL_MEM: 616 without it)."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "distributional_rl_navigation_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
COMMON = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-I../../include", "-I.", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage"]
FLAGS = {"mn_prep_reset.hip": ["-ffp-contract=fast-honor-pragmas", "-fno-slp-vectorize"], "mn_reset.hip": ["-ffp-contract=off"]}      # (csrc/Makefile)
# mn_prep_reset_kernel before this form of the body, by instructions() / lane_moves() below: <double, true> and the waves per SIMD of both precisions
BEFORE_INSTRUCTIONS, BEFORE_LANE_MOVES = 5687, 521
BEFORE_WAVES = {"IdLb1E": 3, "IfLb0E": 4}


def compile_(source):
    """({kernel: [instruction or label lines]}, {kernel: {resource field: int}}) of one source file under the Makefile's flags for it."""
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    r = subprocess.run([HIPCC] + COMMON + FLAGS[source] + ["-S", "-o", "-", source], cwd=CSRC, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    usage, cur = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            cur = usage.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+)", line)
        if m and cur is not None:
            cur[m.group(1).strip()] = int(m.group(2))
    bodies, cur = {}, None
    for line in r.stdout.splitlines():
        m = re.match(r"(_Z\w+):", line)
        if m:
            cur = bodies.setdefault(m.group(1), [])
            continue
        if cur is not None:
            if line.startswith(".Lfunc_end"):
                cur = None
            else:
                cur.append(line.split(";")[0].strip())
    return bodies, usage


def instructions(body):
    """The machine instructions of a kernel's text: no labels, no directives, no blank or comment lines."""
    return [l for l in body if l and not l.endswith(":") and not l.startswith(".")]


def lane_moves(body):
    return [l for l in instructions(body) if re.match(r"v_(read|write)lane_b32\b", l)]


@pytest.fixture(scope="module")
def prep():
    return compile_("mn_prep_reset.hip")


@pytest.fixture(scope="module")
def alone():
    return compile_("mn_reset.hip")


def _kernels(d, needle):
    ks = {k: v for k, v in d.items() if needle in k}
    assert len(ks) == 2 and any("IdLb1E" in k for k in ks) and any("IfLb0E" in k for k in ks), (needle, list(d))
    return ks


def test_no_scratch_in_the_launches_that_run_the_reset_alone(prep, alone):
    for usage, needle in ((prep[1], "mn_prep_reset_kernel"), (alone[1], "15mn_reset_kernel")):
        for k, v in _kernels(usage, needle).items():
            print(k, v)
            assert v["ScratchSize"] == 0, (k, v)


def test_preparation_launch_keeps_its_waves_per_simd_and_its_lds(prep):
    for k, v in _kernels(prep[1], "mn_prep_reset_kernel").items():
        before = BEFORE_WAVES["IdLb1E" if "IdLb1E" in k else "IfLb0E"]
        print(k, v, "waves per SIMD before:", before)
        assert v["Occupancy"] >= before, (k, v)
        assert v["LDS Size"] <= 8192, (k, v)


def test_standalone_reset_kernel_lds(alone):
    for k, v in _kernels(alone[1], "15mn_reset_kernel").items():
        assert v["LDS Size"] <= 8192, (k, v)


def test_training_loops_reset_chain_is_shorter_than_it_was(prep):
    ks = [k for k in prep[0] if "mn_prep_reset_kernel" in k and "IdLb1E" in k]
    assert len(ks) == 1, list(prep[0])
    body = prep[0][ks[0]]
    n, moves = len(instructions(body)), len(lane_moves(body))
    print(f"mn_prep_reset_kernel<double, true>: {n} instructions (before: {BEFORE_INSTRUCTIONS}), {moves} v_readlane_b32 + v_writelane_b32 "
          f"(before: {BEFORE_LANE_MOVES}), {sum(l.startswith('s_waitcnt') for l in body)} s_waitcnt")
    assert n < BEFORE_INSTRUCTIONS
    assert moves < BEFORE_LANE_MOVES
