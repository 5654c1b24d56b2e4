"""Many IQN checkpoints in one episode launch (mn_rollout_iqn_groups, iqn/deferred_eval.py): what can be checked without a GPU -- the C-ABI
declarations and bindings, the grouped kernel's resource budget from hipcc's remarks, the host half of DeferredEvaluations on synthetic traces, and
the evaluation cadence at the reference's density."""
import json
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "distributional_rl_navigation_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"


def test_header_declares_and_capi_binds():
    with open(os.path.join(ROOT, "include", "marinenav_hip.h")) as f:
        header = f.read()
    assert re.search(r"int32_t mn_iqn_image_floats\(void\);", header)
    assert re.search(r"int mn_iqn_export_image\(mn_iqn_ctx \*c, const float \*const \*weights, uint32_t \*image_out_dev, void \*stream\);", header)
    assert re.search(r"int mn_rollout_iqn_groups\(mn_handle \*h, const uint32_t \*images_dev, int64_t image_stride, int32_t n_groups, int32_t rows_per_group", header)
    from distributional_rl_navigation_amd import _capi
    sig = {s[0]: s for s in _capi.SIGNATURES}
    assert len(sig["mn_iqn_image_floats"][2]) == 0
    assert len(sig["mn_iqn_export_image"][2]) == 4
    assert len(sig["mn_rollout_iqn_groups"][2]) == 20


def test_grouped_kernel_has_no_scratch_and_fits_the_cu_lds():
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    with open(os.path.join(CSRC, "Makefile")) as f:
        mk = f.read()
    rule = re.search(r"^mn_rollout_iqn_groups\.o:.*\n\t(.*)$", mk, re.M)
    assert rule and "-ffp-contract=fast-honor-pragmas $(NOSLP)" in rule.group(1)      # mn_rollout_iqn.o's flags
    assert "mn_rollout_iqn_groups.o" in re.search(r"^\$\(OUT\):(.*)$", mk, re.M).group(1)
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-I../../include", "-I.", "--cuda-device-only",
           "-Rpass-analysis=kernel-resource-usage", "-c", "-o", "/dev/null", "-ffp-contract=fast-honor-pragmas", "-fno-slp-vectorize", "mn_rollout_iqn_groups.hip"]
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
    ks = {k: v for k, v in out.items() if "mn_episode_iqn_groups_kernel" in k}
    assert len(ks) == 2, list(out)          # <double, parity, 8 lanes> and <float, compact, 8 lanes>
    assert not [k for k in out if "mn_rollout_iqn_kernel" in k]      # (test_rollout_iqn_cpu.py counts that name)
    dynamic = (37840 + 208 + 32) * 4        # the acting weight image + one feature buffer + the observation row, as mn_rollout_iqn.hip
    for k, v in ks.items():
        assert v["ScratchSize"] == 0, (k, v)
        assert v["LDS Size"] + dynamic <= 163840, (k, v)


def _synthetic_traces(seed, T, G, R):
    """[T][G * R] traces built the way test_rollout_iqn_cpu.py builds them: groups 1 and 3 end early, one episode of group 2 runs past T."""
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


@pytest.mark.parametrize("adaptive", [True, False])
def test_host_half_logs_each_checkpoint_as_its_own_columns(tmp_path, adaptive):
    import torch
    from distributional_rl_navigation_amd.episodes import energy_table
    from distributional_rl_navigation_amd.iqn.agent import IQNAgent, evaluation_from_traces
    from distributional_rl_navigation_amd.iqn.deferred_eval import DeferredEvaluations
    from distributional_rl_navigation_amd.iqn.model import ObsEncoder
    G, R, T = 5, 6, 50
    W = R // 2 if adaptive else R
    tr = _synthetic_traces(7, T, G, R)
    cfg = _eval_config(W)
    agent = IQNAgent(26, 9, device="cpu", seed=3)
    de = DeferredEvaluations(agent, cfg, adaptive=adaptive, max_pending=G, max_steps=T, eval_log_path=str(tmp_path), verbose=False)
    metas = [dict(timestep=1000 * (j + 1), grad_steps=10 * j, vector_step=7 * j) for j in range(G)]
    P = sum(p.numel() for p in agent.qnetwork_local.parameters())
    params = torch.arange(G, dtype=torch.float32).view(G, 1).expand(G, P).contiguous()
    de.log_traces(tr, metas, params, 0.99)

    etab = energy_table(cfg["env_0"]["robot"]["a"], cfg["env_0"]["robot"]["w"])
    policies = ("greedy", "adaptive") if adaptive else ("greedy",)
    best = None
    for j in range(G):
        for p, policy in enumerate(policies):
            sl = slice(j * R + p * W, j * R + (p + 1) * W)
            want = evaluation_from_traces(tr["reward"][:, sl], tr["done"][:, sl], tr["info"][:, sl], tr["action"][:, sl], 0.99, etab, 0.05, 10)
            got = (agent.eval_actions[policy][j], agent.eval_rewards[policy][j], agent.eval_successes[policy][j], agent.eval_times[policy][j],
                   agent.eval_energies[policy][j])
            assert got == want, (j, policy)
            assert agent.eval_timesteps[policy][j] == metas[j]["timestep"]
            if policy == "greedy":      # learn_vec's rule (agent.py: `score > best`), applied to these records in order
                score = (int(sum(want[2])), float(np.mean(want[1])))
                if best is None or score > best[0]:
                    best = (score, j)
    for policy in policies:
        assert len(agent.eval_timesteps[policy]) == G
    if not adaptive:
        assert agent.eval_timesteps["adaptive"] == []
    assert agent.best_eval["score"] == best[0]
    assert (agent.best_eval["timestep"], agent.best_eval["grad_steps"], agent.best_eval["vector_step"]) == tuple(metas[best[1]][k] for k in ("timestep", "grad_steps", "vector_step"))
    with open(tmp_path / "best_evaluation.json") as f:
        bj = json.load(f)
    assert bj["successes"] == best[0][0] and bj["n_worlds"] == W and bj["timestep"] == metas[best[1]]["timestep"]
    # the checkpoints come from the parameter slots: best_* from the best one's, network_params.pth from the latest
    for prefix, j in (("best_", best[1]), ("", G - 1)):
        net = ObsEncoder.load(str(tmp_path), "cpu", prefix=prefix)
        assert list(net.state_dict()) == list(agent.qnetwork_local.state_dict())
        assert all(bool((v == float(j)).all()) for v in net.state_dict().values())
    # the npz files keep the reference's keys, one entry per checkpoint
    for policy in policies:
        z = np.load(tmp_path / f"{policy}_evaluations.npz", allow_pickle=True)
        assert sorted(z.files) == sorted(["timesteps", "actions", "rewards", "successes", "times", "energies"])
        assert all(len(z[k]) == G for k in z.files)
        assert z["timesteps"].tolist() == [m["timestep"] for m in metas]


def test_checkpoint_seed_formula():
    from distributional_rl_navigation_amd.iqn.agent import IQNAgent
    from distributional_rl_navigation_amd.iqn.deferred_eval import DeferredEvaluations, checkpoint_seed
    agent = IQNAgent(26, 9, device="cpu", seed=5)
    base = agent.gen.initial_seed()
    assert base == 5 + 12345
    de = DeferredEvaluations(agent, _eval_config(2))
    seen = set()
    for j in (0, 1, 2, 63, 299):
        want = (base + 0x9E3779B97F4A7C15 * (j + 1)) & 0x7FFFFFFFFFFFFFFF
        assert de.seed_of(j) == want == checkpoint_seed(base, j)
        assert 0 <= want < 2 ** 63 and want != base
        seen.add(want)
    assert len(seen) == 5


def test_cadence_plan_at_the_reference_density():
    from distributional_rl_navigation_amd.train_iqn import plan_cadence
    plan = plan_cadence(3_000_000, 10_000, 4096, 256, n_evals=300)
    assert plan["n_evals"] == 300 and plan["eval_every_vector_steps"] >= 1
    # the loop evaluates where learning_timestep % eval_every == 0, step 0 included; the spacing is floor(vector_steps / n_evals), so where the division
    # leaves a remainder one more point fits behind the 300th
    points = len(range(0, plan["vector_steps"], plan["eval_every_vector_steps"]))
    assert points in (300, 301), (plan["vector_steps"], plan["eval_every_vector_steps"])
    assert plan_cadence(3_000_000, 10_000, 4096, 256)["n_evals"] == 30      # the default stays
    # denser than one point per vector step is not possible: the spacing never drops below 1
    assert plan_cadence(3_000_000, 10_000, 65536 * 64, 256, n_evals=300)["eval_every_vector_steps"] >= 1


def test_learn_vec_keeps_the_inline_form_where_the_launch_has_no_twin(capsys):
    """eval_deferred on an acting form the grouped launch does not reproduce (here: a CPU agent): one log line, and the evaluations stay inline."""
    from distributional_rl_navigation_amd.iqn.agent import IQNAgent
    agent = IQNAgent(26, 9, device="cpu", seed=1)
    assert agent._deferred_evaluations(True, object(), _eval_config(2), True, None) is None
    out = capsys.readouterr().out
    assert out.count("\n") == 1 and "eval_deferred" in out and "inline" in out
