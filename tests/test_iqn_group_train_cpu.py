"""CPU-side checks of the grouped IQN gradient step (`mn_iqn_group_*`, csrc/iqn_train.hip; iqn/group_train.py; `train_iqn --together`): the header and the
binding, the checks `LearnerGroup` makes before it needs a device, how the driver groups the seeds of a config (`--dry-run`), and the compiled resources of
the grouped kernels beside the three forward / backward instantiations they share their body with."""
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
CALLS = ("mn_iqn_group_create", "mn_iqn_group_destroy", "mn_iqn_group_train_step")
FIELDS = ["ring_states", "ring_next_states", "ring_actions", "ring_rewards", "ring_dones", "rng_state", "params_local", "params_target", "workspace", "grad",
          "loss", "exp_avg", "exp_avg_sq", "step", "idx_out", "taus_out"]


def test_header_declares_and_capi_binds_the_group_calls():
    import ctypes
    from distributional_rl_navigation_amd import _capi
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"typedef struct mn_iqn_learner \{(.*?)\} mn_iqn_learner;", src, flags=re.S)
    assert m, "mn_iqn_learner"
    fields = [f for decl in m.group(1).split(";") for f in re.findall(r"\*\s*(\w+)", decl)]
    assert fields == FIELDS
    assert [f for f, _ in _capi.MnIqnLearner._fields_] == fields and ctypes.sizeof(_capi.MnIqnLearner) == 8 * len(fields)      # 16 pointers, no padding
    assert all(t is ctypes.c_void_p for _, t in _capi.MnIqnLearner._fields_)
    assert re.search(r"#define MN_IQN_MAX_LEARNERS 64\b", src) and _capi.IQN_MAX_LEARNERS == 64
    assert re.search(r"typedef struct mn_iqn_group mn_iqn_group;", src)
    bound = {s[0]: s for s in _capi.SIGNATURES}
    n_args = lambda name: len(re.search(rf"\bint {name}\s*\((.*?)\);", src, flags=re.S).group(1).split(","))
    for name, n in zip(CALLS, (4, 1, 12)):
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
    d = dict(BATCH_SIZE=32, capacity=1000, size=640, GAMMA=0.99, n_step=1, LR=1e-4, N=8, device="cuda:0", use_fused_train=True, distributed=False)
    d.update(kw)
    return SimpleNamespace(BATCH_SIZE=d["BATCH_SIZE"], memory=SimpleNamespace(capacity=d["capacity"], size=d["size"]), GAMMA=d["GAMMA"], n_step=d["n_step"],
                           LR=d["LR"], N=d["N"], device=d["device"], use_fused_train=d["use_fused_train"], distributed=d["distributed"])


@pytest.mark.parametrize("kw,word", [(dict(BATCH_SIZE=64), "batch size"), (dict(capacity=2000), "ring capacity"), (dict(size=320), "ring fill"),
                                     (dict(GAMMA=0.9), "gamma"), (dict(n_step=3), "gamma"), (dict(LR=3e-4), "learning rate"), (dict(N=16), "number of taus"),
                                     (dict(device="cuda:1"), "one GPU"), (dict(device="cpu"), "one GPU"), (dict(use_fused_train=False), "fused gradient step"),
                                     (dict(distributed=True), "distributed")])
def test_check_agents_names_the_difference(kw, word):
    from distributional_rl_navigation_amd.iqn.group_train import check_agents
    assert len(check_agents([_fake(), _fake(), _fake()])) == 3
    with pytest.raises(ValueError, match=word):
        check_agents([_fake(), _fake(**kw)])


def test_check_agents_group_size_repeats_and_batch():
    from distributional_rl_navigation_amd.iqn.group_train import MAX_LEARNERS, check_agents
    assert MAX_LEARNERS == 64
    with pytest.raises(ValueError, match="1..64"):
        check_agents([])
    with pytest.raises(ValueError, match="1..64"):
        check_agents([_fake() for _ in range(65)])
    assert len(check_agents([_fake() for _ in range(64)])) == 64
    a = _fake()
    with pytest.raises(ValueError, match="twice"):
        check_agents([a, a])
    with pytest.raises(ValueError, match="even batch"):
        check_agents([_fake(BATCH_SIZE=7), _fake(BATCH_SIZE=7)])


def test_learner_group_refuses_cpu_agents_before_it_needs_a_device():
    """Real agents on the CPU: the refusal comes from the checks, not from a failed device call."""
    from distributional_rl_navigation_amd.iqn.agent import IQNAgent
    from distributional_rl_navigation_amd.iqn.group_train import LearnerGroup
    mk = lambda **kw: IQNAgent(26, 9, device="cpu", **dict(dict(BUFFER_SIZE=256, BATCH_SIZE=8, seed=5), **kw))
    with pytest.raises(ValueError, match="batch size"):
        LearnerGroup([mk(), mk(BATCH_SIZE=16)])
    with pytest.raises(ValueError, match="ring capacity"):
        LearnerGroup([mk(), mk(BUFFER_SIZE=512)])
    with pytest.raises(ValueError, match="one GPU"):
        LearnerGroup([mk(), mk()])


def test_group_trials():
    from distributional_rl_navigation_amd.train_iqn import group_trials
    mk = lambda seed, **kw: dict(dict(agent="IQN", seed=seed, total_timesteps=1000, eval_freq=100, save_dir="x", training_time="t"), **kw)
    assert group_trials([mk(s) for s in range(5)]) == [[0, 1, 2, 3, 4]]
    assert group_trials([mk(0), mk(1, total_timesteps=2000), mk(2)]) == [[0, 2], [1]]
    assert group_trials([mk(7)]) == [[0]]
    big = group_trials([mk(s) for s in range(70)])
    assert [len(g) for g in big] == [64, 6] and sum(big, []) == list(range(70))


def _train_iqn(tmp_path, *extra, env=None):
    cfg = tmp_path / "config_IQN.json"
    cfg.write_text(json.dumps(CONFIG_IQN))
    return subprocess.run([sys.executable, "-m", "distributional_rl_navigation_amd.train_iqn", "-C", str(cfg), *extra], cwd=ROOT, capture_output=True,
                          text=True, timeout=300, env=dict(os.environ, CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="", **(env or {})))


def test_dry_run_names_one_group_of_five(tmp_path):
    r = _train_iqn(tmp_path, "--together", "--dry-run", "--env-budget", "reference")
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
    trials, groups = [l for l in lines if "seed" in l], [l for l in lines if "together" in l]
    assert [t["seed"] for t in trials] == [0, 1, 2, 3, 4] and len(groups) == 1
    assert groups[0]["together"] == [dict(group=0, seeds=[0, 1, 2, 3, 4], grouped_gradient_launches=True)]
    assert all(t["plan"]["grad_steps_per_vector_step"] == 20 and t["batch"] == 32 for t in trials)
    # without the option the output is what it was: no group line
    r = _train_iqn(tmp_path, "--dry-run", "--env-budget", "reference")
    assert r.returncode == 0 and "together" not in r.stdout


@pytest.mark.parametrize("extra,env,sentence", [(("--torch-train",), None, "--together needs the fused HIP gradient step"),
                                                (("--shared-learner",), None, "--together trains independent learners"),
                                                (("-P", "2"), None, "--together runs the seeds in ONE process"),
                                                ((), dict(WORLD_SIZE="2"), "--together is the single-process, single-GPU form")])
def test_together_refuses_what_it_cannot_group(tmp_path, extra, env, sentence):
    r = _train_iqn(tmp_path, "--together", "--dry-run", *extra, env=env)
    assert r.returncode != 0 and sentence in r.stderr, r.stderr[-1000:]


def test_run_trials_together_refuses_before_it_needs_a_device():
    from distributional_rl_navigation_amd.train_iqn import run_trials_together
    two = [dict(CONFIG_IQN, seed=0, training_time="t"), dict(CONFIG_IQN, seed=1, training_time="t")]
    with pytest.raises(ValueError, match="no grouped form of the PyTorch step"):
        run_trials_together("cuda:0", two, 16, torch_train=True)
    with pytest.raises(ValueError, match="differ only in their seed"):
        run_trials_together("cuda:0", [two[0], dict(two[1], eval_freq=5_000)], 16)


def test_grouped_kernels_have_no_scratch_and_the_forward_backward_instantiations_stay_three():
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-I../../include", "-I.", "-ffp-contract=off", "-mllvm", "-disable-machine-licm",
           "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c", "-o", os.devnull, "iqn_train.hip"]      # csrc/Makefile's flags for this file
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
    grouped = {k: v for k, v in usage.items() if "iqn_group_" in k}
    for name in ("iqn_group_fwdbwd_kernel", "iqn_group_reduce_kernel", "iqn_group_adam_kernel"):
        assert len([k for k in grouped if name + "E" in k]) == 1, (name, list(usage))      # (the mangled name: <length><name>E<argument types>)
    assert len(grouped) == 3, list(grouped)
    for k, v in grouped.items():
        assert v["ScratchSize"] == 0, (k, v)
        if "iqn_group_fwdbwd_kernel" in k:
            assert v["VGPRs"] + v.get("AGPRs", 0) <= 256, (k, v)
    single = {k: v for k, v in usage.items() if "iqn_train_fwdbwd" in k}
    assert len(single) == 3, list(single)      # <XCHG, FUSED> = <false, false>, <false, true>, <true, true>: the shared body is emitted nowhere else
    for k, v in single.items():
        assert v["ScratchSize"] == 0 and v["VGPRs"] + v.get("AGPRs", 0) <= 256, (k, v)
    # the single kernels whose bodies the grouped reduction and Adam share
    for name in ("iqn_grad_reduceE", "iqn_adamE"):
        ks = [k for k in usage if name in k]
        assert len(ks) == 1 and usage[ks[0]]["ScratchSize"] == 0, (name, ks)
