"""CPU-side checks of the grouped DQN gradient step (`mn_dqn_group_*`, csrc/dqn_train.hip; dqn/group_train.py; `train_dqn --together`): the header and
the binding, the checks `LearnerGroup` makes before it needs a device, how the driver groups the seeds of a config (`--dry-run`), and the compiled
resources of every kernel of dqn_train.hip, old and new."""
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
CONFIG_DQN = {"agent": "DQN", "seed": [0, 1, 2, 3, 4], "total_timesteps": 3_000_000, "eval_freq": 10_000, "save_dir": "dqn_runs"}
CALLS = ("mn_dqn_group_create", "mn_dqn_group_destroy", "mn_dqn_group_train_step", "mn_dqn_group_train_steps")


def test_header_declares_and_capi_binds_the_group_calls():
    import ctypes
    from distributional_rl_navigation_amd import _capi
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"typedef struct mn_dqn_learner \{(.*?)\} mn_dqn_learner;", src, flags=re.S)
    assert m, "mn_dqn_learner"
    fields = re.findall(r"\*\s*(\w+)", m.group(1))
    assert fields == ["ring_states", "ring_next_states", "ring_actions", "ring_rewards", "ring_dones", "rng_state", "params_local", "params_target", "grad",
                      "exp_avg", "exp_avg_sq", "step"]
    assert [f for f, _ in _capi.MnDqnLearner._fields_] == fields and ctypes.sizeof(_capi.MnDqnLearner) == 8 * len(fields)
    assert re.search(r"#define MN_DQN_MAX_LEARNERS 64\b", src) and _capi.DQN_MAX_LEARNERS == 64
    assert re.search(r"typedef struct mn_dqn_group mn_dqn_group;", src)
    bound = {s[0]: s for s in _capi.SIGNATURES}
    for name in CALLS:
        assert re.search(rf"\bint {name}\s*\(", src), name
        assert name in bound, name
    # argument counts of the two launches: the multi-step call has n_steps in addition
    n_args = lambda name: len(re.search(rf"\bint {name}\s*\((.*?)\);", src, flags=re.S).group(1).split(","))
    assert n_args("mn_dqn_group_train_step") == len(bound["mn_dqn_group_train_step"][2]) == 14
    assert n_args("mn_dqn_group_train_steps") == len(bound["mn_dqn_group_train_steps"][2]) == 15
    if not os.path.exists(_capi.LIB_PATH):
        _capi.build()
    lib = _capi.lib()
    for name in CALLS:
        assert hasattr(lib, name), name


def _fake(**kw):
    """What `check_agents` reads of a DQNAgent."""
    d = dict(batch_size=32, capacity=1000, size=640, gamma=0.99, learning_rate=1e-4, max_grad_norm=10, device="cuda:0", fused=True)
    d.update(kw)
    return SimpleNamespace(batch_size=d["batch_size"], memory=SimpleNamespace(capacity=d["capacity"], size=d["size"]), gamma=d["gamma"],
                           learning_rate=d["learning_rate"], max_grad_norm=d["max_grad_norm"], device=d["device"], fused_train=d["fused"],
                           _uses_fused=lambda: d["fused"])


@pytest.mark.parametrize("kw,word", [(dict(batch_size=64), "batch size"), (dict(capacity=2000), "ring capacity"), (dict(size=320), "ring fill"),
                                     (dict(gamma=0.9), "gamma"), (dict(learning_rate=3e-4), "learning rate"), (dict(max_grad_norm=5), "max_grad_norm"),
                                     (dict(device="cuda:1"), "one GPU"), (dict(device="cpu"), "one GPU"), (dict(fused=False), "fused path")])
def test_check_agents_names_the_difference(kw, word):
    from distributional_rl_navigation_amd.dqn.group_train import check_agents
    assert len(check_agents([_fake(), _fake(), _fake()])) == 3
    with pytest.raises(ValueError, match=word):
        check_agents([_fake(), _fake(**kw)])


def test_check_agents_group_size_and_repeats():
    from distributional_rl_navigation_amd.dqn.group_train import MAX_LEARNERS, check_agents
    assert MAX_LEARNERS == 64
    with pytest.raises(ValueError, match="1..64"):
        check_agents([])
    with pytest.raises(ValueError, match="1..64"):
        check_agents([_fake() for _ in range(65)])
    a = _fake()
    with pytest.raises(ValueError, match="twice"):
        check_agents([a, a])


def test_learner_group_refuses_mismatched_agents_before_it_needs_a_device():
    """Real agents on the CPU: the refusal comes from the checks, not from a failed device call."""
    from distributional_rl_navigation_amd.dqn import DQNAgent
    from distributional_rl_navigation_amd.dqn.group_train import LearnerGroup
    mk = lambda **kw: DQNAgent(device="cpu", **dict(dict(buffer_size=256, batch_size=8, seed=5, fused_train=True), **kw))
    with pytest.raises(ValueError, match="batch size"):
        LearnerGroup([mk(), mk(batch_size=16)])
    with pytest.raises(ValueError, match="ring capacity"):
        LearnerGroup([mk(), mk(buffer_size=512)])
    with pytest.raises(ValueError, match="one GPU"):
        LearnerGroup([mk(), mk()])


def _train_dqn(tmp_path, *extra):
    cfg = tmp_path / "config_DQN.json"
    cfg.write_text(json.dumps(CONFIG_DQN))
    return subprocess.run([sys.executable, "-m", "distributional_rl_navigation_amd.train_dqn", "-C", str(cfg), *extra], cwd=ROOT, capture_output=True,
                          text=True, timeout=300, env=dict(os.environ, CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES=""))


def test_dry_run_names_one_group_of_five(tmp_path):
    r = _train_dqn(tmp_path, "--together", "--dry-run", "--env-budget", "reference")
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
    trials, groups = [l for l in lines if "seed" in l], [l for l in lines if "together" in l]
    assert [t["seed"] for t in trials] == [0, 1, 2, 3, 4] and len(groups) == 1
    assert groups[0]["together"] == [dict(group=0, seeds=[0, 1, 2, 3, 4], one_launch_per_gradient_step=True)]
    # without the option the output is what it was: no group line
    r = _train_dqn(tmp_path, "--dry-run", "--env-budget", "reference")
    assert r.returncode == 0 and "together" not in r.stdout


def test_group_trials():
    from distributional_rl_navigation_amd.train_dqn import group_trials
    mk = lambda seed, **kw: dict(dict(agent="DQN", seed=seed, total_timesteps=1000, eval_freq=100, save_dir="x", training_time="t"), **kw)
    assert group_trials([mk(s) for s in range(5)]) == [[0, 1, 2, 3, 4]]
    assert group_trials([mk(0), mk(1, total_timesteps=2000), mk(2)]) == [[0, 2], [1]]
    assert group_trials([mk(7)]) == [[0]]
    big = group_trials([mk(s) for s in range(130)])
    assert [len(g) for g in big] == [64, 64, 2] and sum(big, []) == list(range(130))


def test_together_with_torch_train_is_refused(tmp_path):
    r = _train_dqn(tmp_path, "--together", "--torch-train", "--dry-run")
    assert r.returncode != 0 and "--together needs the fused HIP gradient step" in r.stderr
    from distributional_rl_navigation_amd.train_dqn import run_trials_together
    with pytest.raises(ValueError, match="no grouped form of the eager"):
        run_trials_together("cuda:0", [dict(CONFIG_DQN, seed=0, training_time="t"), dict(CONFIG_DQN, seed=1, training_time="t")], 16, torch_train=True)


def test_every_kernel_of_the_file_has_no_scratch_and_the_chains_fit_one_cu():
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-I../../include", "-I.", "-ffp-contract=off", "--cuda-device-only",
           "-Rpass-analysis=kernel-resource-usage", "-c", "-o", os.devnull, "dqn_train.hip"]
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
    names = ("dqn_train_step_kernel", "dqn_multi_target_kernel", "dqn_multi_chain_kernel", "dqn_train_step_groups_kernel", "dqn_multi_target_groups_kernel",
             "dqn_multi_chain_groups_kernel")
    assert len(usage) == len(names), list(usage)
    for name in names:
        ks = [k for k in usage if name + "E" in k]      # (the mangled name: <length><name>E<argument types>)
        assert len(ks) == 1, (name, list(usage))
    for k, v in usage.items():
        assert v["ScratchSize"] == 0, (k, v)
        if "dqn_multi_chain" in k:
            assert v["LDS Size"] <= 163_840, (k, v)
            # 1 024 threads are four waves on each SIMD: 512 / 4 vector registers a lane at the most, or the workgroup does not launch
            assert v["VGPRs"] + v.get("AGPRs", 0) <= 128, (k, v)
