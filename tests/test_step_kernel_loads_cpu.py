"""How the step kernel (csrc/mn_step.hip, MnLane::step in csrc/mn_step_body.h) is compiled, without a GPU: hipcc cross-compiles gfx950, and the
assembly of every `mn_step_kernel` instantiation is read for where its vector loads sit.

What is pinned: nothing is fetched from memory behind the sub-step loop (the beam tables and the action constants used to be -- per-lane indexed reads of
the by-value MnDev argument, issued behind the action's and the sub-steps' results: a second and a third memory round trip on a step's dependent chain),
the number of loads is what the lane's tables need, and the training loop's kernel starts its sub-steps while its obstacle rows and its share of the
obs_t row are still in flight."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "distributional_rl_navigation_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
MAX_CORES, MAX_OBS, NUM_BEAMS = 8, 10, 11
# (M, PARITY) as the mangled name spells them, lanes per env, APPEND
KERNELS = [(mp, L, ap) for mp in ("IdLb1E", "IfLb0E") for L in (1, 2, 4, 8) for ap in (0, 1)]


def _name(mp, L, ap):
    return f"mn_step_kernel{mp}Li{L}ELb{ap}EE"


@pytest.fixture(scope="module")
def compiled():
    """(assembly lines per kernel, resource usage per kernel) of mn_step.hip under the Makefile's flags for mn_step.o."""
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-I../../include", "-I.", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage",
           "-ffp-contract=off", "-fno-slp-vectorize", "-S", "-o", "-", "mn_step.hip"]
    r = subprocess.run(cmd, cwd=CSRC, capture_output=True, text=True, timeout=900)
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
        m = re.match(r"(_Z\w*mn_step_kernel\w+):", line)
        if m:
            cur = bodies.setdefault(m.group(1), [])
            continue
        if cur is not None:
            if line.startswith(".Lfunc_end"):
                cur = None
            else:
                cur.append(line.split(";")[0].strip())
    return bodies, usage


def _pick(d, mp, L, ap):
    ks = [k for k in d if _name(mp, L, ap) in k]
    assert len(ks) == 1, (mp, L, ap, list(d))
    return d[ks[0]]


def substep_loop(body):
    """Index of the label the sub-step loop branches back to: the first loop (a label with a branch back to it further down) that evaluates the current
    field, i.e. holds a reciprocal (v_rcp_f64 / v_rcp_f32 of the squared distance to a vortex core; the sonar scan's loop has square roots only, the heading
    wrap's loops neither)."""
    at = {m.group(1): i for i, l in enumerate(body) for m in [re.match(r"(\.LBB\d+_\d+):", l)] if m}
    loops = []
    for i, l in enumerate(body):
        m = re.match(r"s_cbranch_\w+\s+(\.LBB\d+_\d+)", l) or re.match(r"s_branch\s+(\.LBB\d+_\d+)", l)
        if m and at.get(m.group(1), i) < i and any(re.match(r"v_rcp_f(32|64)", x) for x in body[at[m.group(1)]:i]):
            loops.append(at[m.group(1)])
    assert loops, "no sub-step loop found"
    return min(loops)


def loads(body):
    return [i for i, l in enumerate(body) if l.startswith("global_load")]


def waits_in_front(body, loop):
    """vmcnt of every s_waitcnt in front of the loop's label that waits for vector memory at all."""
    return [int(m.group(1)) for l in body[:loop] if l.startswith("s_waitcnt") for m in [re.search(r"vmcnt\((\d+)\)", l)] if m]


def shares(L):
    cpl = MAX_CORES // L if L <= MAX_CORES else 1
    return cpl, -(-MAX_OBS // L), -(-NUM_BEAMS // L)


def test_all_sixteen_instantiations_are_there(compiled):
    bodies, usage = compiled
    assert len(bodies) == 16 and len([k for k in usage if "mn_step_kernel" in k]) == 16
    for mp, L, ap in KERNELS:
        assert _pick(bodies, mp, L, ap)


@pytest.mark.parametrize("mp,L,ap", KERNELS)
def test_no_load_behind_the_substep_loop_and_no_more_loads_than_the_tables_need(compiled, mp, L, ap):
    body = _pick(compiled[0], mp, L, ap)
    loop, ld = substep_loop(body), loads(body)
    cpl, opl, bpl = shares(L)
    bound = 11 + 3 * cpl + 3 * opl + (2 + bpl if ap else 0) + 2      # pose / goal / counters / action, cores, obstacles, obs_t row, MnDev's small tables
    print(f"{_name(mp, L, ap)}: {len(ld)} global_load (bound {bound}), {sum(i > loop for i in ld)} behind the sub-step loop, "
          f"waits in front of it vmcnt {waits_in_front(body, loop)}")
    assert not [body[i] for i in ld if i > loop]
    assert len(ld) <= bound, [body[i] for i in ld]


def test_headline_kernel_keeps_four_waves_and_starts_its_substeps_under_the_table_loads(compiled):
    """mn_step_kernel<double, true, 4, true>, the training loop's: <= 128 VGPRs and no scratch (4 waves per SIMD: 65 536 envs are one round), and no wait in
    front of the sub-step loop drains the vector-memory counter: the obstacle rows and this lane's share of the obs_t row -- issued last, counted in order --
    stay outstanding, 3 OPL + 1 + BPL of them or more."""
    bodies, usage = compiled
    u, body = _pick(usage, "IdLb1E", 4, 1), _pick(bodies, "IdLb1E", 4, 1)
    assert u["VGPRs"] <= 128 and u.get("AGPRs", 0) == 0 and u["ScratchSize"] == 0, u
    w = waits_in_front(body, substep_loop(body))
    cpl, opl, bpl = shares(4)
    print("headline:", u, "waits", w)
    assert w and min(w) > 0, w
    assert min(w) >= 3 * opl + 1 + bpl, w
