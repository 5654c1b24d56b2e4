"""Many DQN checkpoints in one episode launch (mn_rollout_dqn_groups, dqn/deferred_eval.py): what can be checked without a GPU -- the C-ABI
declarations and bindings, the Makefile rule, the grouped kernel's resource budget from hipcc's remarks, the host half of DeferredEvaluations on
synthetic traces, and the driver's flag."""
import io
import json
import os
import re
import subprocess
import sys
import zipfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "distributional_rl_navigation_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
IMAGE_BYTES = 126912      # mn_dqn_image_floats() * 4: the weight image in dynamic LDS (tests/test_rollout_dqn_cpu.py checks the number)


def test_header_declares_and_capi_binds():
    with open(os.path.join(ROOT, "include", "marinenav_hip.h")) as f:
        header = f.read()
    assert re.search(r"int mn_dqn_export_image\(const float \*const \*weights, float \*image_out_dev, void \*stream\);", header)
    assert re.search(r"int mn_rollout_dqn_groups\(mn_handle \*h, const float \*images_dev, int64_t image_stride, int32_t n_groups, int32_t rows_per_group,\s+int32_t n_steps",
                     header)
    from distributional_rl_navigation_amd import _capi
    sig = {s[0]: s for s in _capi.SIGNATURES}
    assert len(sig["mn_dqn_export_image"][2]) == 3
    assert len(sig["mn_rollout_dqn_groups"][2]) == 14
    assert len(sig["mn_rollout_dqn"][2]) == 13      # unchanged


def _makefile():
    with open(os.path.join(CSRC, "Makefile")) as f:
        return f.read()


def _recipe_flags(mk, target):
    """The hipcc flags of `target`'s recipe, unexpanded and expanded."""
    m = re.search(rf"^{re.escape(target)}:.*\n\t\$\(HIPCC\) (.*) -c \$< -o \$@", mk, flags=re.M)
    assert m, target
    var = dict(re.findall(r"^(\w+) \??= (.*)$", mk, flags=re.M))
    flags = m.group(1)
    for _ in range(3):
        flags = re.sub(r"\$\((\w+)\)", lambda v: var[v.group(1)], flags)
    return m.group(1), flags.split()


def test_makefile_builds_and_links_the_grouped_object_with_the_dqn_episode_flags():
    mk = _makefile()
    raw, flags = _recipe_flags(mk, "mn_rollout_dqn_groups.o")
    raw_single, flags_single = _recipe_flags(mk, "mn_rollout_dqn.o")
    assert raw == raw_single and flags == flags_single
    assert "-ffp-contract=off $(NOSLP)" in raw and "-ffp-contract=off" in flags and "-fno-slp-vectorize" in flags
    rule = re.search(r"^mn_rollout_dqn_groups\.o:(.*)$", mk, re.M).group(1)
    assert "mn_rollout_dqn_groups.hip" in rule and "mn_rollout_dqn_body.h" in rule
    assert "mn_rollout_dqn_body.h" in re.search(r"^mn_rollout_dqn\.o:(.*)$", mk, re.M).group(1)      # the body is shared, not copied
    assert "mn_rollout_dqn_groups.o" in re.search(r"^\$\(OUT\):(.*)$", mk, re.M).group(1)
    abl = re.search(r"^\$\(ABL\):.*\n(?:\t.*\n)*?\t(\$\(HIPCC\) --offload-arch=\$\(ARCH\) -shared .*)$", mk, re.M)
    assert abl and "mn_rollout_dqn_groups.o" in abl.group(1)      # the ablation link line
    with open(os.path.join(CSRC, "mn_rollout_dqn.hip")) as f:
        single = f.read()
    with open(os.path.join(CSRC, "mn_rollout_dqn_groups.hip")) as f:
        grouped = f.read()
    for src in (single, grouped):
        assert '#include "mn_rollout_dqn_body.h"' in src and "dqn_episode<" in src and "ln.template step" not in src


def test_grouped_kernel_has_no_scratch_and_fits_the_cu_lds():
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    _, flags = _recipe_flags(_makefile(), "mn_rollout_dqn.o")
    cmd = [HIPCC] + flags + ["--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c", "-o", "/dev/null", "mn_rollout_dqn_groups.hip"]
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
    ks = {k: v for k, v in out.items() if "mn_episode_dqn_groups_kernel" in k}
    assert len(ks) == 2, list(out)          # <double, parity, 8 lanes> and <float, compact, 8 lanes>
    assert not [k for k in out if "mn_rollout_dqn_kernel" in k]      # (test_rollout_dqn_cpu.py counts that name)
    for k, v in ks.items():
        assert v["ScratchSize"] == 0, (k, v)
        assert v["LDS Size"] + IMAGE_BYTES <= 163840, (k, v)


def _synthetic_traces(seed, T, G, R):
    """[T][G * R] traces, the construction of tests/test_rollout_iqn_groups_cpu.py::_synthetic_traces: groups 1 and 3 end early, one episode of group
    2 runs past T."""
    rng = np.random.RandomState(seed)
    n = G * R
    ends = rng.randint(1, T + 1, size=n)
    ends[1 * R:2 * R] = rng.randint(1, 8, size=R)
    ends[3 * R:4 * R] = rng.randint(1, 15, size=R)
    ends[2 * R + 1] = T + 20
    t_idx = np.arange(T)[:, None]
    alive_before = t_idx < ends[None, :]
    done = (t_idx >= ends[None, :] - 1).astype(np.uint8)
    info = np.where(t_idx == ends[None, :] - 1, rng.randint(2, 5, size=(T, n)), 0).astype(np.uint8)
    info = np.where(t_idx > ends[None, :] - 1, info[np.minimum(ends - 1, T - 1), np.arange(n)][None, :], info).astype(np.uint8)
    reward = np.where(alive_before, rng.standard_normal((T, n)).astype(np.float32), 0).astype(np.float32)
    action = np.where(alive_before, rng.randint(0, 9, size=(T, n)), -1).astype(np.int32)
    return dict(reward=reward, done=done, info=info, action=action)


def _eval_config(n_worlds):
    robot = dict(N=10, dt=0.05, a=[-0.4, 0.0, 0.4], w=[-0.5235988, 0.0, 0.5235988])
    return {f"env_{i}": dict(robot=robot) for i in range(n_worlds)}


def _zip_state(path):
    import torch
    with zipfile.ZipFile(path) as z:
        assert z.namelist() == ["policy.pth"]
        return torch.load(io.BytesIO(z.read("policy.pth")), map_location="cpu")


def test_host_half_logs_each_checkpoint_as_its_own_columns(tmp_path):
    import torch
    from distributional_rl_navigation_amd import train_dqn
    from distributional_rl_navigation_amd.dqn import DQNAgent
    from distributional_rl_navigation_amd.dqn.deferred_eval import DeferredEvaluations
    from distributional_rl_navigation_amd.episodes import energy_table, steps_run
    G, R, T = 5, 6, 50
    tr = _synthetic_traces(7, T, G, R)
    cfg = _eval_config(R)
    agent = DQNAgent(26, 9, buffer_size=64, device="cpu", seed=3)
    de = DeferredEvaluations(agent, cfg, str(tmp_path), max_pending=G, max_steps=T, verbose=False)
    timesteps = [1000 * (j + 1) for j in range(G)]
    P = sum(p.numel() for p in agent.q_net.parameters())
    local = torch.arange(G, dtype=torch.float32).view(G, 1).expand(G, P).contiguous()
    target = local + 100.0
    recs = de.log_traces(tr, timesteps, local, target, 0.99)

    etab = energy_table(cfg["env_0"]["robot"]["a"], cfg["env_0"]["robot"]["w"])
    best, best_j = -np.inf, None
    for j in range(G):
        sl = slice(j * R, (j + 1) * R)
        want = train_dqn.evaluation_from_rollout({k: tr[k][:, sl] for k in tr}, 0.99, etab, 0.05, 10)
        for k in ("rewards", "successes", "times", "energies"):
            for got in (de.log[k][j], recs[j][k]):
                assert got.dtype == want[k].dtype and got.tolist() == want[k].tolist(), (j, k)
        assert de.log["actions"][j] == want["actions"] == recs[j]["actions"], j
        assert de.log["timesteps"][j] == timesteps[j]
        assert recs[j]["steps_run"] == steps_run(tr["done"][:, sl]) == de.steps_run[j]
        mean_r = float(np.mean(want["rewards"]))
        if mean_r > best:      # run_trial's rule (`mean_r > best`), applied to these records in order: the FIRST checkpoint with the highest mean
            best, best_j = mean_r, j
    assert de.best == best and 0 < best_j        # (a later checkpoint wins: best_model.zip was rewritten on the way)
    assert de.steps_run[2] == T and max(de.steps_run[1], de.steps_run[3]) < 15
    # the zips hold the snapshot's parameters under save_zip's keys: best_model.zip the best checkpoint's, latest_model.zip the last one's
    keys = list(agent.state_dict())
    for name, j in (("best_model.zip", best_j), ("latest_model.zip", G - 1)):
        sd = _zip_state(tmp_path / name)
        assert list(sd) == keys
        for k, v in sd.items():
            assert v.shape == agent.state_dict()[k].shape and v.dtype == torch.float32
            assert bool((v == float(j) + (100.0 if k.startswith("q_net_target.") else 0.0)).all()), (name, k)
    # what DQNAgent.load / DQNPolicy.load read
    from distributional_rl_navigation_amd.dqn import DQNPolicy
    pol = DQNPolicy.load(str(tmp_path / "latest_model.zip"), device="cpu")
    assert all(bool((p == float(G - 1)).all()) for p in pol.parameters())
    # evaluations.npz: the keys, dtypes and shapes of the inline form (train_dqn.write_evaluations is what run_trial writes it with)
    z = np.load(tmp_path / "evaluations.npz", allow_pickle=True)
    assert sorted(z.files) == sorted(["timesteps", "rewards", "times", "energies", "successes", "actions"])
    assert z["timesteps"].dtype == np.int64 and z["timesteps"].tolist() == timesteps
    for k in ("rewards", "times", "energies"):
        assert z[k].dtype == np.float64 and z[k].shape == (G, R), k
    assert z["successes"].dtype == bool and z["successes"].shape == (G, R)
    assert z["actions"].dtype == object and z["actions"].shape == (G,) and len(z["actions"][0]) == R
    inline = tmp_path / "inline"
    inline.mkdir()
    train_dqn.write_evaluations(str(inline), de.log)
    zi = np.load(inline / "evaluations.npz", allow_pickle=True)
    for k in z.files:
        assert z[k].dtype == zi[k].dtype and z[k].shape == zi[k].shape and z[k].tolist() == zi[k].tolist(), k


def test_host_half_appends_across_flushes(tmp_path):
    """Two flushes of 2 and 3 checkpoints log what one flush of 5 logs: the log and the best mean carry over."""
    import torch
    from distributional_rl_navigation_amd.dqn import DQNAgent
    from distributional_rl_navigation_amd.dqn.deferred_eval import DeferredEvaluations
    G, R, T = 5, 6, 50
    tr = _synthetic_traces(7, T, G, R)
    agent = DQNAgent(26, 9, buffer_size=64, device="cpu", seed=3)
    P = sum(p.numel() for p in agent.q_net.parameters())
    local = torch.arange(G, dtype=torch.float32).view(G, 1).expand(G, P).contiguous()
    out = []
    for k, parts in enumerate(([(0, 5)], [(0, 2), (2, 5)])):
        d = tmp_path / f"run{k}"
        d.mkdir()
        de = DeferredEvaluations(agent, _eval_config(R), str(d), max_pending=G, max_steps=T, verbose=False)
        for a, b in parts:
            de.log_traces({key: v[:, a * R:b * R] for key, v in tr.items()}, [100 * (j + 1) for j in range(a, b)], local[a:b], local[a:b] + 1, 0.99)
        z = np.load(d / "evaluations.npz", allow_pickle=True)
        out.append(({key: z[key].tolist() for key in z.files}, de.best, {n: _zip_state(d / n) for n in ("best_model.zip", "latest_model.zip")}))
    assert out[0][0] == out[1][0] and out[0][1] == out[1][1]
    for n in ("best_model.zip", "latest_model.zip"):
        assert all(torch.equal(out[0][2][n][k], out[1][2][n][k]) for k in out[0][2][n])


def test_train_dqn_dry_run_reports_eval_deferred(tmp_path):
    cfg = tmp_path / "config_DQN.json"
    cfg.write_text(json.dumps({"agent": "DQN", "seed": [0, 1], "total_timesteps": 3_000_000, "eval_freq": 10_000, "save_dir": str(tmp_path)}))
    out = {}
    for extra in ((), ("--eval-deferred",), ("--eval-deferred", "--n-evals", "300")):
        r = subprocess.run([sys.executable, "-m", "distributional_rl_navigation_amd.train_dqn", "-C", str(cfg), "--dry-run", *extra],
                           cwd=ROOT, capture_output=True, text=True, timeout=300, env=dict(os.environ, CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES=""))
        assert r.returncode == 0, r.stderr[-2000:]
        out[extra] = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
    assert [t["eval_deferred"] for t in out[()]] == [False, False]
    assert [t["eval_deferred"] for t in out[("--eval-deferred",)]] == [True, True]
    assert [t["plan"] for t in out[()]] == [t["plan"] for t in out[("--eval-deferred",)]]      # the flag changes no plan
    assert [t["plan"]["n_evals"] for t in out[("--eval-deferred", "--n-evals", "300")]] == [300, 300]      # the reference's density reaches the plan


def test_run_trial_keeps_the_inline_form_where_the_launch_has_no_twin():
    """eval_deferred for a policy that does not act through the fused kernel (here: a CPU agent): `can_defer` is false -- run_trial then prints one
    line and keeps the evaluations inline."""
    from distributional_rl_navigation_amd.dqn import DQNAgent
    from distributional_rl_navigation_amd.dqn.deferred_eval import can_defer
    assert can_defer(DQNAgent(26, 9, buffer_size=64, device="cpu", seed=1)) is False
