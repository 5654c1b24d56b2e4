"""CPU-side checks of the DQN collect on the device (`mn_dqn_act_rng`, `mn_dqn_actor_group_*`: csrc/dqn_collect.hip + replay.hip; dqn/group_collect.py;
`train_dqn --fused-collect`, `--together --stack-envs`): the compiled resources of the new kernels, the host twin of their draws (tests/dqn_rng_twin.py),
the checks `CollectorGroup` makes before it needs a device, the driver's refusals and `--dry-run`."""
import json
import os
import re
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import dqn_rng_twin as D      # noqa: E402
import rng_twin as T      # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "distributional_rl_navigation_amd", "csrc")
HEADER = os.path.join(ROOT, "include", "marinenav_hip.h")
HIPCC = "/opt/rocm/bin/hipcc"
CONFIG_DQN = {"agent": "DQN", "seed": [0, 1, 2, 3, 4], "total_timesteps": 3_000_000, "eval_freq": 10_000, "save_dir": "dqn_runs"}      # the reference's config_DQN.json
CALLS = ("mn_dqn_act_rng", "mn_dqn_actor_group_create", "mn_dqn_actor_group_destroy", "mn_dqn_actor_group_set_grid", "mn_dqn_actor_group_act",
         "mn_dqn_actor_group_append")
FIELDS = ["weights", "image", "seed", "ring_states", "ring_next_states", "ring_actions", "ring_rewards", "ring_dones"]


# ---- the compiled kernels ---------------------------------------------------------------------------------------------------------------------------------
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


def _image_floats():
    """IMAGE_FLOATS of csrc/dqn_net.h from its stage table: per stage 256 floats per (M tile, K tile) of weights and 16 per M tile of biases."""
    src = open(os.path.join(CSRC, "dqn_net.h")).read()
    m = re.search(r"LM\[N_LAYERS\] = \{([^}]*)\}, LK\[N_LAYERS\] = \{([^}]*)\}", src)
    lm, lk = ([int(x) for x in g.split(",")] for g in m.groups())
    return sum(a * b * 256 for a, b in zip(lm, lk)) + sum(a * 16 for a in lm)


def test_collect_kernels_have_no_scratch_and_only_the_image_in_lds():
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    usage = _resource_usage("dqn_collect.hip")
    names = ("dqn_act_rng_kernel", "dqn_group_act_rng_kernel", "dqn_group_pack_kernel")
    assert len(usage) == len(names), list(usage)
    for name in names:
        ks = [k for k in usage if name + "E" in k]      # (the mangled name: <length><name>E<argument types>)
        assert len(ks) == 1, (name, list(usage))
        v = usage[ks[0]]
        assert v["ScratchSize"] == 0 and v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0, (name, v)
        assert v["LDS Size"] == 0, (name, v)      # no static LDS: the act kernels' LDS is the dynamic size of their launches alone ...
    image_bytes = _image_floats() * 4
    assert image_bytes <= 160 * 1024
    host = open(os.path.join(CSRC, "dqn_collect.hip")).read()
    launches = re.findall(r"hipLaunchKernelGGL\((dqn_\w+), dim3\([^;]*?\), dim3\(\d+\), ([^,]+), s,", host)      # ... which is the image, and nothing for the pack
    assert sorted(launches) == [("dqn_act_rng_kernel", "IMAGE_FLOATS * sizeof(float)"), ("dqn_group_act_rng_kernel", "IMAGE_FLOATS * sizeof(float)"),
                                ("dqn_group_pack_kernel", "0")], launches
    from distributional_rl_navigation_amd import _capi
    if not os.path.exists(_capi.LIB_PATH):
        _capi.build()
    assert _capi.lib().mn_dqn_image_floats() == _image_floats() == 31_728      # 124 KB
    usage = _resource_usage("replay.hip")
    for name in ("replay_append_dqn_groups_kernel", "replay_append_groups_kernel"):
        ks = [k for k in usage if name + "E" in k]
        assert len(ks) == 1 and usage[ks[0]]["ScratchSize"] == 0 and usage[ks[0]]["LDS Size"] == 0, (name, list(usage))


def test_header_declares_and_capi_binds_the_collect_calls():
    import ctypes
    from distributional_rl_navigation_amd import _capi
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"typedef struct mn_dqn_actor \{(.*?)\} mn_dqn_actor;", src, flags=re.S)
    assert m, "mn_dqn_actor"
    fields = [f for decl in m.group(1).split(";") for f in re.findall(r"(?:\*\s*(?!const\b)|uint64_t\s+)(\w+)", decl)]
    assert fields == FIELDS
    assert [f for f, _ in _capi.MnDqnActor._fields_] == fields and ctypes.sizeof(_capi.MnDqnActor) == 8 * len(fields)      # 8-byte members, no padding
    assert dict(_capi.MnDqnActor._fields_)["seed"] is ctypes.c_uint64
    assert re.search(r"#define MN_DQN_MAX_ACTORS 64\b", src) and _capi.DQN_MAX_ACTORS == 64
    bound = {s[0]: s for s in _capi.SIGNATURES}
    n_args = lambda name: len(re.search(rf"\bint {name}\s*\((.*?)\);", src, flags=re.S).group(1).split(","))
    for name, n in zip(CALLS, (12, 4, 1, 2, 7, 9)):
        assert name in bound, name
        assert n_args(name) == len(bound[name][2]) == n, name
    if not os.path.exists(_capi.LIB_PATH):
        _capi.build()
    lib = _capi.lib()
    for name in CALLS:
        assert hasattr(lib, name), name
    # the argument checks that need no device: nothing is dereferenced, nothing launched
    assert lib.mn_dqn_act_rng(None, None, None, 0, 1, 0, 0.5, None, None, None, 16, None) != 0
    assert lib.mn_dqn_actor_group_create(None, 1, 16, ctypes.byref(ctypes.c_void_p())) != 0
    assert lib.mn_dqn_actor_group_act(None, None, 0.5, 0, None, None, None) != 0 and lib.mn_dqn_actor_group_destroy(None) != 0
    assert lib.mn_dqn_actor_group_append(None, None, None, None, None, None, 0, 16, None) != 0


# ---- the host twin ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed,ctr", [(0, 0), (4321 + 103, 7), (2 ** 64 - 1, 2 ** 32 + 5), (-3, 2 ** 63)])
def test_twin_uniforms_are_24_bit_fractions_and_prefix_stable(seed, ctr):
    u = D.dqn_act_uniforms(seed, ctr, 4099)
    assert u.dtype == np.float32 and u.shape == (4099,)
    assert (u >= 0).all() and (u < 1).all()
    k = u.astype(np.float64) * 2 ** 24
    assert np.array_equal(k, np.floor(k))      # k / 2^24 exactly
    for m in (1, 16, 17, 4098):
        assert np.array_equal(D.dqn_act_uniforms(seed, ctr, m), u[:m])      # row e's draw does not depend on n
    assert np.array_equal(u, T.u01(np.arange(4099), *T.draw_keys(seed, ctr)))
    assert 0.45 < u.mean() < 0.55


def test_twin_streams_differ_by_call_and_by_seed():
    base = D.dqn_act_uniforms(11, 0, 2048)
    for other in (D.dqn_act_uniforms(11, 1, 2048), D.dqn_act_uniforms(11, 2 ** 32, 2048), D.dqn_act_uniforms(12, 0, 2048)):
        assert (other == base).mean() < 0.01      # (equal 24-bit values by chance: 2^-24 per row)
        assert abs(np.corrcoef(base, other)[0, 1]) < 0.1
    # the act stream of IQNAgent under the same (seed, ctr) starts with taus: the DQN call's row e is that buffer's element e
    assert np.array_equal(base[:64], T.act_draws(11, 0, 2)[:64])


def test_twin_actions_at_the_edges_of_eps():
    n = 5000
    greedy = (np.arange(n) % 9).astype(np.int32)
    u = D.dqn_act_uniforms(5, 3, n)
    for eps in (0.0, -1.0, float("nan")):      # !(eps > 0): greedy everywhere
        assert np.array_equal(D.dqn_actions(5, 3, eps, greedy), greedy)
    a = D.dqn_actions(5, 3, 1.0, greedy)      # u < 1 = eps: every row explores, floor(9 u)
    assert np.array_equal(a, np.minimum((u * np.float32(9)).astype(np.int32), 8)) and a.min() == 0 and a.max() == 8
    assert np.bincount(a, minlength=9).min() > n / 9 * 0.8
    a = D.dqn_actions(5, 3, 0.05, greedy)
    exp = u <= np.float32(0.05)
    assert 0.03 < exp.mean() < 0.07 and np.array_equal(a[~exp], greedy[~exp]) and (a[exp] >= 0).all() and (a[exp] <= 8).all()
    # u == eps explores (greedy iff u > eps), and u / eps * 9 = 9 is clamped to action 8
    eps = float(u[17])
    assert eps > 0
    a = D.dqn_actions(5, 3, eps, np.full(n, 4, np.int32))
    assert a[17] == 8 and T.explore_action(u[17], eps, 4) == 8
    above = u > np.float32(eps)
    assert (a[above] == 4).all()
    assert a.dtype == np.int32


# ---- the checks in front of a grouped launch -----------------------------------------------------------------------------------------------------------------
def _fake(**kw):
    """What `check_agents` reads of a DQNAgent."""
    d = dict(device="cuda:0", fused_collect=True, use_fused_act=True, capacity=1000, ptr=160)
    d.update(kw)
    return SimpleNamespace(device=d["device"], fused_collect=d["fused_collect"], policy=SimpleNamespace(use_fused_act=d["use_fused_act"]),
                           memory=SimpleNamespace(capacity=d["capacity"], ptr=d["ptr"]))


@pytest.mark.parametrize("kw,word", [(dict(device="cuda:1"), "one GPU"), (dict(device="cpu"), "one GPU"), (dict(fused_collect=False), "fused_collect"),
                                     (dict(use_fused_act=False), "use_fused_act"), (dict(capacity=2000), "ring capacity"), (dict(ptr=176), r"ptr\) \(176 against 160\)")])
def test_check_agents_names_the_difference(kw, word):
    from distributional_rl_navigation_amd.dqn.group_collect import check_agents
    assert len(check_agents([_fake(), _fake(), _fake()], 48)) == 3
    with pytest.raises(ValueError, match=word):
        check_agents([_fake(), _fake(**kw)], 32)


def test_check_agents_group_size_repeats_and_rows():
    from distributional_rl_navigation_amd.dqn.group_collect import MAX_ACTORS, check_agents
    assert MAX_ACTORS == 64
    with pytest.raises(ValueError, match="1..64"):
        check_agents([])
    with pytest.raises(ValueError, match="1..64"):
        check_agents([_fake() for _ in range(65)])
    assert len(check_agents([_fake() for _ in range(64)], 64 * 8)) == 64
    a = _fake()
    with pytest.raises(ValueError, match="twice"):
        check_agents([a, a])
    with pytest.raises(ValueError, match="equal groups"):      # equal row counts
        check_agents([_fake(), _fake(), _fake()], 32)


def test_collector_group_refuses_cpu_agents_before_it_needs_a_device():
    """Real agents on the CPU: the refusal comes from the checks, not from a failed device call."""
    from distributional_rl_navigation_amd.dqn import DQNAgent
    from distributional_rl_navigation_amd.dqn.group_collect import CollectorGroup
    mk = lambda **kw: DQNAgent(device="cpu", **dict(dict(buffer_size=256, batch_size=8, seed=5, fused_collect=True), **kw))
    a = mk()
    assert a.fused_collect and not a.uses_fused_collect() and a.act_seed == 5 + 4321 and a.act_calls == 0
    with pytest.raises(ValueError, match="one GPU"):
        CollectorGroup([a, mk()], SimpleNamespace(n_envs=32))


def test_cpu_agent_with_fused_collect_acts_as_without():
    """On the CPU the switch changes nothing: the same torch.Generator draws, and the call counter stays."""
    import torch
    from distributional_rl_navigation_amd.dqn import DQNAgent
    mk = lambda fc: DQNAgent(device="cpu", buffer_size=64, batch_size=8, seed=9, fused_collect=fc)
    a, b = mk(True), mk(False)
    obs = torch.randn(40, 26, generator=torch.Generator().manual_seed(1))
    for eps in (1.0, 0.5, 0.0):
        assert torch.equal(a.act_batch(obs, eps), b.act_batch(obs, eps))
    assert a.act_calls == 0


# ---- the driver -------------------------------------------------------------------------------------------------------------------------------------------
def _train_dqn(tmp_path, *extra):
    cfg = tmp_path / "config_DQN.json"
    cfg.write_text(json.dumps(CONFIG_DQN))
    return subprocess.run([sys.executable, "-m", "distributional_rl_navigation_amd.train_dqn", "-C", str(cfg), *extra], cwd=ROOT, capture_output=True,
                          text=True, timeout=300, env=dict(os.environ, CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES=""))


def test_stack_envs_refusals(tmp_path):
    from distributional_rl_navigation_amd.train_dqn import TOGETHER_REFUSALS, run_trials_together
    assert TOGETHER_REFUSALS["stack_envs"] == "--stack-envs stacks the envs of seeds that train together in one handle; it needs --together"
    r = _train_dqn(tmp_path, "--stack-envs", "--dry-run")
    assert r.returncode != 0 and TOGETHER_REFUSALS["stack_envs"] in r.stderr, r.stderr[-1000:]
    r = _train_dqn(tmp_path, "--together", "--torch-train", "--stack-envs", "--dry-run")
    assert r.returncode != 0 and TOGETHER_REFUSALS["torch_train"] in r.stderr, r.stderr[-1000:]
    two = [dict(CONFIG_DQN, seed=0, training_time="t", save_dir=str(tmp_path)), dict(CONFIG_DQN, seed=1, training_time="t", save_dir=str(tmp_path))]
    with pytest.raises(ValueError, match="no grouped form of the eager"):
        run_trials_together("cuda:0", two, 16, torch_train=True, stack_envs=True)      # (before it needs a device)
    with pytest.raises(ValueError, match="stack_envs: the stacked collect runs on HIP kernels"):
        run_trials_together("cpu", two, 16, stack_envs=True)
    assert not os.listdir(tmp_path) or os.listdir(tmp_path) == ["config_DQN.json"]      # refused before a trial directory was made


def test_dry_run_names_the_stacked_handle_and_is_unchanged_without_the_flags(tmp_path):
    lines = lambda r: [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
    r = _train_dqn(tmp_path, "--together", "--stack-envs", "--dry-run", "--env-budget", "reference")
    assert r.returncode == 0, r.stderr[-2000:]
    groups = [l for l in lines(r) if "together" in l]
    assert len(groups) == 1
    assert groups[0]["together"] == [dict(group=0, seeds=[0, 1, 2, 3, 4], one_launch_per_gradient_step=True, stacked_env_rows=400, rows_per_seed=80)]
    assert all(t["fused_collect"] is True for t in lines(r) if "seed" in t)      # --stack-envs implies --fused-collect
    r = _train_dqn(tmp_path, "--together", "--stack-envs", "--dry-run")
    assert r.returncode == 0 and [l for l in lines(r) if "together" in l][0]["together"][0]["stacked_env_rows"] == 5 * 4096
    r = _train_dqn(tmp_path, "--fused-collect", "--dry-run")
    assert r.returncode == 0 and all(t["fused_collect"] is True for t in lines(r)) and "together" not in r.stdout
    # without the new flags: the keys and values of every line are what they were -- no word of the collect
    for extra in ((), ("--together",)):
        r = _train_dqn(tmp_path, "--dry-run", "--env-budget", "reference", *extra)
        assert r.returncode == 0 and "stacked_env_rows" not in r.stdout and "fused_collect" not in r.stdout and "rows_per_seed" not in r.stdout
        trials = [l for l in lines(r) if "seed" in l]
        assert [list(t) for t in trials] == [["seed", "n_envs", "batch", "replay", "fused", "eval_one_launch", "eval_deferred", "env_budget", "episode_log",
                                              "eps_start", "eps_end", "plan"]] * 5
        if extra:
            assert [l for l in lines(r) if "together" in l] == [dict(together=[dict(group=0, seeds=[0, 1, 2, 3, 4], one_launch_per_gradient_step=True)])]
