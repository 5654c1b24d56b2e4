"""CPU-side checks of the stacked collect (`mn_iqn_actor_group_*`, csrc/iqn_act.hip + iqn_act_group.h + replay.hip; iqn/group_collect.py; `train_iqn
--together --stack-envs`): the header and the binding, the checks `CollectorGroup` makes before it needs a device, the driver's refusals and `--dry-run`,
and the compiled resources of the grouped kernels beside the act kernel's existing forms, whose body they share."""
import json
import os
import re
import subprocess
import sys
from types import SimpleNamespace

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "distributional_rl_navigation_amd", "csrc")
HEADER = os.path.join(ROOT, "include", "marinenav_hip.h")
HIPCC = "/opt/rocm/bin/hipcc"
CONFIG_IQN = {"agent": "IQN", "seed": [0, 1, 2, 3, 4], "total_timesteps": 3_000_000, "eval_freq": 10_000, "save_dir": "iqn_runs"}      # the reference's config_IQN.json
CALLS = ("mn_iqn_actor_group_create", "mn_iqn_actor_group_destroy", "mn_iqn_actor_group_act", "mn_iqn_actor_group_append")
FIELDS = ["ctx", "weights", "rng_state", "draws", "ring_states", "ring_next_states", "ring_actions", "ring_rewards", "ring_dones"]


def test_header_declares_and_capi_binds_the_actor_group_calls():
    import ctypes
    from distributional_rl_navigation_amd import _capi
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"typedef struct mn_iqn_actor \{(.*?)\} mn_iqn_actor;", src, flags=re.S)
    assert m, "mn_iqn_actor"
    fields = [f for decl in m.group(1).split(";") for f in re.findall(r"\*\s*(?!const\b)(\w+)", decl)]      # (`*const *weights`: a const pointer is no name)
    assert fields == FIELDS
    assert [f for f, _ in _capi.MnIqnActor._fields_] == fields and ctypes.sizeof(_capi.MnIqnActor) == 8 * len(fields)      # 9 pointers, no padding
    assert all(t is ctypes.c_void_p for _, t in _capi.MnIqnActor._fields_)
    assert re.search(r"#define MN_IQN_MAX_ACTORS 64\b", src) and _capi.IQN_MAX_ACTORS == 64
    assert re.search(r"typedef struct mn_iqn_actor_group mn_iqn_actor_group;", src)
    bound = {s[0]: s for s in _capi.SIGNATURES}
    n_args = lambda name: len(re.search(rf"\bint {name}\s*\((.*?)\);", src, flags=re.S).group(1).split(","))
    for name, n in zip(CALLS, (4, 1, 6, 9)):
        assert re.search(rf"\bint {name}\s*\(", src), name
        assert name in bound, name
        assert n_args(name) == len(bound[name][2]) == n, name
    if not os.path.exists(_capi.LIB_PATH):
        _capi.build()
    lib = _capi.lib()
    for name in CALLS:
        assert hasattr(lib, name), name


def _fake(**kw):
    """What `check_agents` reads of an IQNAgent."""
    d = dict(device="cuda:0", use_fused_act=True, use_library_rng=True, n_step=1, shared_taus=False, variant=2, distributed=False, act_greedy_rows_only=True,
             capacity=1000, ptr=160)
    d.update(kw)
    net = SimpleNamespace(_act_ctx=None if d["variant"] is None else SimpleNamespace(variant=d["variant"]))
    return SimpleNamespace(device=d["device"], use_fused_act=d["use_fused_act"], use_library_rng=d["use_library_rng"], n_step=d["n_step"], shared_taus=d["shared_taus"],
                           qnetwork_local=net, distributed=d["distributed"], act_greedy_rows_only=d["act_greedy_rows_only"],
                           memory=SimpleNamespace(capacity=d["capacity"], ptr=d["ptr"]))


@pytest.mark.parametrize("kw,word", [(dict(device="cuda:1"), "one GPU"), (dict(device="cpu"), "one GPU"), (dict(use_fused_act=False), "fused act kernel"),
                                     (dict(use_library_rng=False), "library's generator"), (dict(n_step=3), "n_step"), (dict(shared_taus=True), "shared taus"),
                                     (dict(variant=0), "variant"), (dict(act_greedy_rows_only=False), "greedy-rows"), (dict(capacity=2000), "ring capacity"),
                                     (dict(ptr=176), "ptr"), (dict(distributed=True), "distributed")])
def test_check_agents_names_the_difference(kw, word):
    from distributional_rl_navigation_amd.iqn.group_collect import check_agents
    assert len(check_agents([_fake(), _fake(variant=None), _fake()], 48)) == 3
    with pytest.raises(ValueError, match=word):
        check_agents([_fake(), _fake(**kw)], 32)


def test_check_agents_group_size_repeats_and_rows():
    from distributional_rl_navigation_amd.iqn.group_collect import MAX_ACTORS, check_agents
    assert MAX_ACTORS == 64
    with pytest.raises(ValueError, match="1..64"):
        check_agents([])
    with pytest.raises(ValueError, match="1..64"):
        check_agents([_fake() for _ in range(65)])
    assert len(check_agents([_fake() for _ in range(64)], 64 * 8)) == 64
    a = _fake()
    with pytest.raises(ValueError, match="twice"):
        check_agents([a, a])
    with pytest.raises(ValueError, match="equal groups"):
        check_agents([_fake(), _fake(), _fake()], 32)


def test_collector_group_refuses_cpu_agents_before_it_needs_a_device():
    """Real agents on the CPU: the refusal comes from the checks, not from a failed device call."""
    from distributional_rl_navigation_amd.iqn.agent import IQNAgent
    from distributional_rl_navigation_amd.iqn.group_collect import CollectorGroup
    mk = lambda **kw: IQNAgent(26, 9, device="cpu", **dict(dict(BUFFER_SIZE=256, BATCH_SIZE=8, seed=5), **kw))
    with pytest.raises(ValueError, match="one GPU"):
        CollectorGroup([mk(), mk()], SimpleNamespace(n_envs=32))


def test_stacked_seeds_and_rows():
    import numpy as np
    from distributional_rl_navigation_amd.marinenav_env.vec_env import StackedRows, shard_seeds, stacked_seeds
    s = stacked_seeds(16, [3, 4, 2 ** 32 - 2])
    assert s.dtype == np.uint32 and s.shape == (48,)
    for g, seed in enumerate((3, 4, 2 ** 32 - 2)):
        assert np.array_equal(s[16 * g:16 * (g + 1)], shard_seeds(16, seed))
    env = SimpleNamespace(n_envs=48, device="cuda:0", discount=0.99)
    v = StackedRows(env, 2, 16)
    assert v.n_envs == 16 and v.rows == slice(32, 48) and v.discount == 0.99 and v.close() is None
    with pytest.raises(ValueError, match="not rows"):
        StackedRows(env, 3, 16)


def _train_iqn(tmp_path, *extra, env=None):
    cfg = tmp_path / "config_IQN.json"
    cfg.write_text(json.dumps(CONFIG_IQN))
    return subprocess.run([sys.executable, "-m", "distributional_rl_navigation_amd.train_iqn", "-C", str(cfg), *extra], cwd=ROOT, capture_output=True,
                          text=True, timeout=300, env=dict(os.environ, CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="", **(env or {})))


def test_stack_envs_refusals(tmp_path):
    from distributional_rl_navigation_amd.train_iqn import TOGETHER_REFUSALS, run_trials_together
    assert TOGETHER_REFUSALS["stack_envs"] == "--stack-envs stacks the envs of seeds that train together in one handle; it needs --together"
    r = _train_iqn(tmp_path, "--stack-envs", "--dry-run")
    assert r.returncode != 0 and TOGETHER_REFUSALS["stack_envs"] in r.stderr, r.stderr[-1000:]
    r = _train_iqn(tmp_path, "--together", "--stack-envs", "--shared-taus", "--dry-run")
    assert r.returncode != 0 and TOGETHER_REFUSALS["stack_shared_taus"] in r.stderr, r.stderr[-1000:]
    two = [dict(CONFIG_IQN, seed=0, training_time="t"), dict(CONFIG_IQN, seed=1, training_time="t")]
    with pytest.raises(ValueError, match="n_step > 1"):
        run_trials_together("cuda:0", two, 16, stack_envs=True, n_step=3)      # (before it needs a device)
    with pytest.raises(ValueError, match="launch-shared taus"):
        run_trials_together("cuda:0", two, 16, stack_envs=True, shared_taus=True)


def test_dry_run_names_the_stacked_handle(tmp_path):
    r = _train_iqn(tmp_path, "--together", "--stack-envs", "--dry-run", "--env-budget", "reference")
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
    groups = [l for l in lines if "together" in l]
    assert len(groups) == 1
    assert groups[0]["together"] == [dict(group=0, seeds=[0, 1, 2, 3, 4], grouped_gradient_launches=True, stacked_env_rows=400, rows_per_seed=80)]
    r = _train_iqn(tmp_path, "--together", "--stack-envs", "--dry-run")
    assert r.returncode == 0 and json.loads([l for l in r.stdout.splitlines() if "together" in l][0])["together"][0]["stacked_env_rows"] == 5 * 4096
    # without the option the group line is what it was
    r = _train_iqn(tmp_path, "--together", "--dry-run")
    assert r.returncode == 0 and "stacked_env_rows" not in r.stdout


def _resource_usage(source, *flags):
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-I../../include", "-I.", *flags, "--cuda-device-only",
           "-Rpass-analysis=kernel-resource-usage", "-c", "-o", os.devnull, source]      # csrc/Makefile's flags for the file
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
    return usage


def test_grouped_kernels_have_no_scratch_and_the_act_forms_keep_theirs():
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    usage = _resource_usage("iqn_act.hip", "-ffp-contract=fast", "-fno-slp-vectorize")
    grouped = {k: v for k, v in usage.items() if "iqn_group_act_kernelILb" in k}
    assert sorted(re.search(r"iqn_group_act_kernelILb(\d)E", k).group(1) for k in grouped) == ["0", "1"], list(usage)      # exactly two: every row / the listed rows
    for k, v in grouped.items():
        assert v["ScratchSize"] == 0 and v["VGPRs Spill"] == 0 and v["VGPRs"] + v.get("AGPRs", 0) <= 256, (k, v)
        assert v["LDS Size"] == 0, (k, v)      # no static LDS on top of the dynamic image + feature buffers ...
    host = open(os.path.join(CSRC, "iqn_act.hip")).read()
    body = host[host.index('extern "C" int mn_iqn_actor_group_act'):]
    assert re.search(r"const size_t lds = sp::LDS_ACT_FLOATS \* sizeof\(float\);", body)      # ... which is what both are launched with, the single acting forms' size
    assert len(re.findall(r"iqn_group_act_kernel<(?:true|false)>, grid, block, lds, s,", body)) == 2
    single = {k: v for k, v in usage.items() if "iqn_qvals_split_kernelILb" in k}
    assert len(single) == 7, list(single)      # the seven forms of FORMS: the shared body is emitted nowhere else
    for k, v in single.items():
        assert v["ScratchSize"] == 0, (k, v)
    acting = [v for k, v in single.items() if "iqn_qvals_split_kernelILb0ELb0ELi8E" in k]
    assert len(acting) == 4 and all(204 <= v["VGPRs"] <= 206 and v["VGPRs Spill"] == 0 for v in acting), acting      # what they were before the body moved into its own file
    for name in ("iqn_group_consts_kernelE", "iqn_group_prep_kernelE"):
        ks = [k for k in usage if name in k]
        assert len(ks) == 1 and usage[ks[0]]["ScratchSize"] == 0, (name, ks)
    usage = _resource_usage("replay.hip")
    ks = [k for k in usage if "replay_append_groups_kernelE" in k]
    assert len(ks) == 1 and usage[ks[0]]["ScratchSize"] == 0, list(usage)
