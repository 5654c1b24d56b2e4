"""Many IQN checkpoints in ONE episode launch (C-ABI `mn_rollout_iqn_groups`, csrc/mn_rollout_iqn_groups.hip; iqn/deferred_eval.py).

Claim under test: every group of rows of the grouped launch computes, bit for bit, what a launch of its own (`rollout_iqn`) computes with the group's
network, worlds and tau stream -- traces, final rows, poses, longest episode, call counter --; the evaluations `DeferredEvaluations` logs from it are
those of a fresh agent per checkpoint; and taking deferred evaluation points does not change the training run.  All comparisons are exact."""
import copy
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DEV = "cuda:0"
ALL_TRACES = ("reward", "done", "info", "action", "cvar", "q", "obs")


@pytest.fixture(scope="module")
def torch():
    import torch as t
    if not t.cuda.is_available():
        pytest.skip("no GPU")
    return t


def _cfg(n_worlds=2):
    with open(os.path.join(GOLD, "eval_config_seed3.json")) as f:
        cfg = json.load(f)
    return {k: cfg[k] for k in list(cfg)[:n_worlds]}


def _worlds(cfg):
    from distributional_rl_navigation_amd.marinenav_env.vec_env import VecMarineNavEnv
    return [VecMarineNavEnv.world_from_eval_config(c) for c in cfg.values()]


def _env(cfg, n_groups, precision, reps=2):
    """An env of n_groups x (the worlds of cfg, `reps` times), configured as IQNAgent.evaluation_vec configures its env."""
    from distributional_rl_navigation_amd.marinenav_env.vec_env import VecMarineNavEnv
    w = _worlds(cfg)
    env = VecMarineNavEnv(n_groups * reps * len(w), device=DEV, precision=precision)
    r0 = list(cfg.values())[0]["robot"]
    env.set_attrs(N=r0["N"], dt=r0["dt"])
    env.load_worlds(w * (n_groups * reps))
    return env


def _nets():
    """The shipped checkpoint and two randomly initialised networks: three policies that act differently."""
    from distributional_rl_navigation_amd.iqn.model import ObsEncoder
    return [ObsEncoder.load(os.path.join(GOLD, "pretrained_IQN_seed3"), DEV), ObsEncoder(26, 9, seed=21, device=DEV), ObsEncoder(26, 9, seed=22, device=DEV)]


def _images(torch, nets):
    from distributional_rl_navigation_amd.iqn.fused_act import export_image, image_floats
    img = torch.empty(len(nets), image_floats(), dtype=torch.int32, device=DEV)
    for j, net in enumerate(nets):
        export_image(net, img[j])
    return img


def _states(torch, seeds):
    return torch.tensor([[s, 0] for s in seeds], dtype=torch.int64, device=DEV)


def _bits(torch, x):
    return x.view(torch.int32) if x.dtype == torch.float32 else x


def _standalone(torch, net, seed, cfg, T, precision, launches=1):
    """`launches` consecutive stand-alone launches of one (network, seed) pair on a fresh env of the group's rows, the worlds reloaded in between:
    per launch (traces, final_obs, state, steps_run, counter)."""
    from distributional_rl_navigation_amd.iqn.fused_act import ActRng, rollout_iqn
    W = len(cfg)
    cv = torch.ones(2 * W)
    ad = torch.tensor([False] * W + [True] * W)
    env = _env(cfg, 1, precision)
    rng = ActRng(seed, DEV)
    out = []
    for k in range(launches):
        if k:
            env.load_worlds(_worlds(cfg) * 2)
        tr = rollout_iqn(net, env, T, rng, cvar_rows=cv, adaptive_rows=ad, trace=ALL_TRACES)
        assert tr is not None
        out.append(({k2: tr[k2].clone() for k2 in ALL_TRACES}, tr["final_obs"].clone(), env.get_state(), tr["steps_run"], int(rng.state[1])))
    env.close()
    return out


def _check_group(torch, got, env, states, g, R, ref):
    tr, final_obs, state, steps, counter = ref
    sl = slice(g * R, (g + 1) * R)
    for k in ALL_TRACES:
        assert torch.equal(_bits(torch, got[k][:, sl]), _bits(torch, tr[k])), (g, k)
    assert torch.equal(_bits(torch, got["final_obs"][sl]), _bits(torch, final_obs)), g
    s, ep, tot = env.get_state(g * R, R)
    assert np.array_equal(s.view(np.int64), state[0].view(np.int64)) and np.array_equal(ep, state[1]) and np.array_equal(tot, state[2]), g
    assert int(got["steps_run"][g]) == steps, g
    assert int(states[g, 1]) == counter, g


@pytest.mark.parametrize("precision,G,W,T", [("f64", 3, 2, 48), ("mixed", 2, 1, 24)])
def test_group_launch_equals_separate_launches(torch, precision, G, W, T):
    from distributional_rl_navigation_amd.iqn.fused_act import rollout_iqn_groups
    cfg = _cfg(W)
    R = 2 * W
    nets = _nets()[:G]
    seeds = [101, 202, 303][:G]
    env = _env(cfg, G, precision)
    states = _states(torch, seeds)
    cv = torch.ones(G * R)
    ad = torch.tensor(([False] * W + [True] * W) * G)
    got = rollout_iqn_groups(_images(torch, nets), env, T, states, R, cvar_rows=cv, adaptive_rows=ad, trace=ALL_TRACES)
    torch.cuda.synchronize()
    assert not got["group_words"].any()
    for g in range(G):
        _check_group(torch, got, env, states, g, R, _standalone(torch, nets[g], seeds[g], cfg, T, precision)[0])
    # the groups really act with their own images: two of them choose different action sequences on the same worlds
    a = got["action"]
    assert not torch.equal(a[:, 0:R], a[:, R:2 * R])
    assert got["steps_run"].shape == (G,) and int(states[:, 1].min()) >= 1
    env.close()


def test_more_workgroups_than_cus(torch):
    from distributional_rl_navigation_amd.iqn.fused_act import rollout_iqn_groups
    G, W, T = 75, 2, 24
    R = 2 * W
    cfg = _cfg(W)
    nets, seeds = _nets(), [11, 12, 13]
    refs = [_standalone(torch, nets[k], seeds[k], cfg, T, "f64", launches=2) for k in range(3)]
    images = _images(torch, nets)[torch.arange(G, device=DEV) % 3].contiguous()
    states = _states(torch, [seeds[g % 3] for g in range(G)])
    cv = torch.ones(G * R)
    ad = torch.tensor(([False] * W + [True] * W) * G)
    env = _env(cfg, G, "f64")
    assert G * R > torch.cuda.get_device_properties(0).multi_processor_count
    for launch in range(2):      # the second launch continues from the counters the first one left, like the stand-alone launches continued the same way
        if launch:
            env.load_worlds(_worlds(cfg) * (2 * G))
        got = rollout_iqn_groups(images, env, T, states, R, cvar_rows=cv, adaptive_rows=ad, trace=ALL_TRACES)
        torch.cuda.synchronize()
        assert not got["group_words"].any()
        for g in range(G):
            _check_group(torch, got, env, states, g, R, refs[g % 3][launch])
    env.close()


def test_export_image_is_the_image_a_fresh_context_builds(torch):
    from distributional_rl_navigation_amd import _capi
    from distributional_rl_navigation_amd.iqn.fused_act import act_context, export_image, image_floats, rollout_iqn_groups
    from distributional_rl_navigation_amd.iqn.model import ObsEncoder
    cfg, T = _cfg(2), 24
    net = ObsEncoder(26, 9, seed=31, device=DEV)
    img = torch.zeros(1, image_floats(), dtype=torch.int32, device=DEV)
    cv, ad = torch.ones(4), torch.tensor([False, False, True, True])
    for change in (False, True):
        if change:      # written through PyTorch: the context's cached image is stale and has to be rebuilt before it is copied
            with torch.no_grad():
                for p in net.parameters():
                    p.mul_(1.03125)
        before = img.clone()
        export_image(net, img[0])
        assert not torch.equal(before, img)
        env = _env(cfg, 1, "f64")
        states = _states(torch, [55])
        got = rollout_iqn_groups(img, env, T, states, 4, cvar_rows=cv, adaptive_rows=ad, trace=ALL_TRACES)
        torch.cuda.synchronize()
        _check_group(torch, got, env, states, 0, 4, _standalone(torch, copy.deepcopy(net), 55, cfg, T, "f64")[0])
        env.close()
    ctx = act_context(net)
    ctx.set_variant(0)
    with pytest.raises(_capi.MarineNavHipError):
        export_image(net, img[0])
    ctx.set_variant(2)
    export_image(net, img[0])


def _learn(torch, tmp_path, name, eval_freq, deferred, with_eval=True, snapshots=None):
    """The issue's run: learn_vec on 64 envs for 40 vector steps with a 2-world evaluation config, evaluation points every `eval_freq` learning steps
    (10: 4 points), deferred (episodes of 30 steps at most, 3 pending: one flush on the way, one at the end) or inline.  `snapshots`: a dict that
    receives the network's state_dict after every vector step."""
    from distributional_rl_navigation_amd.iqn.agent import IQNAgent
    from distributional_rl_navigation_amd.marinenav_env.vec_env import VecMarineNavEnv
    cfg = _cfg(2)
    agent = IQNAgent(26, 9, device=DEV, seed=1, BATCH_SIZE=64, BUFFER_SIZE=4096, learning_starts=1)
    train_env = VecMarineNavEnv(64, seed=0, device=DEV, precision="f64")
    eval_env = VecMarineNavEnv(2, device=DEV, precision="f64") if with_eval else None
    d = tmp_path / name
    d.mkdir()
    hook = None
    if snapshots is not None:
        hook = lambda it, stats: snapshots.__setitem__(it, {k: v.detach().clone() for k, v in agent.qnetwork_local.state_dict().items()})
    agent.learn_vec(total_vector_steps=40, train_env=train_env, eval_env=eval_env, eval_config=cfg, eval_freq=eval_freq, eval_log_path=str(d), verbose=False,
                    on_step=hook, eval_one_launch=True, eval_deferred=dict(max_steps=30, max_pending=3, verbose=False) if deferred else False)
    torch.cuda.synchronize()
    train_env.close()
    if eval_env is not None:
        eval_env.close()
    return agent, str(d)


def test_deferred_equals_inline_per_checkpoint(torch, tmp_path):
    from distributional_rl_navigation_amd.episodes import EPISODE_TRACES, energy_table, host_traces
    from distributional_rl_navigation_amd.iqn.agent import IQNAgent, evaluation_from_traces
    from distributional_rl_navigation_amd.iqn.deferred_eval import checkpoint_seed
    from distributional_rl_navigation_amd.iqn.fused_act import ActRng, rollout_iqn
    cfg = _cfg(2)
    snaps = {}
    agent, d = _learn(torch, tmp_path, "deferred", 10, True, snapshots=snaps)
    assert agent.eval_timesteps["greedy"] == agent.eval_timesteps["adaptive"] and len(agent.eval_timesteps["greedy"]) == 4
    inline, _ = _learn(torch, tmp_path, "inline", 10, False)
    assert inline.eval_timesteps == agent.eval_timesteps
    r0 = list(cfg.values())[0]["robot"]
    etab = energy_table(r0["a"], r0["w"])
    cv, ad = torch.ones(4), torch.tensor([False, False, True, True])
    points = [ts // 64 - 1 for ts in agent.eval_timesteps["greedy"]]      # the vector step after which current_timestep was the logged one
    for j, it in enumerate(points):
        fresh = IQNAgent(26, 9, device=DEV, seed=9)
        fresh.qnetwork_local.load_state_dict(snaps[it])
        fresh._act_rng = ActRng(checkpoint_seed(agent.gen.initial_seed(), j), DEV)
        env = _env(cfg, 1, "f64")
        tr = rollout_iqn(fresh.qnetwork_local, env, 30, fresh._act_rng, cvar_rows=cv, adaptive_rows=ad, trace=EPISODE_TRACES)
        data = evaluation_from_traces(**host_traces(tr), discount=env.discount, energy_tab=etab, dt=r0["dt"], N=r0["N"])
        env.close()
        for p, policy in enumerate(("greedy", "adaptive")):
            sl = slice(2 * p, 2 * p + 2)
            got = (agent.eval_actions[policy][j], agent.eval_rewards[policy][j], agent.eval_successes[policy][j], agent.eval_times[policy][j],
                   agent.eval_energies[policy][j])
            assert got == tuple(x[sl] for x in data), (j, policy)
    for policy in ("greedy", "adaptive"):
        z = np.load(os.path.join(d, f"{policy}_evaluations.npz"), allow_pickle=True)
        assert sorted(z.files) == sorted(["timesteps", "actions", "rewards", "successes", "times", "energies"])
        assert all(len(z[k]) == 4 for k in z.files)
        assert z["timesteps"].tolist() == agent.eval_timesteps[policy]
    # network_params.pth: the latest snapshot's parameters; best_*: those of the checkpoint best_eval names
    latest = torch.load(os.path.join(d, "network_params.pth"), map_location=DEV)
    assert all(torch.equal(latest[k], snaps[points[-1]][k]) for k in latest)
    best = torch.load(os.path.join(d, "best_network_params.pth"), map_location=DEV)
    assert all(torch.equal(best[k], snaps[agent.best_eval["vector_step"]][k]) for k in best)


def _train_state(agent):
    f = agent._fused
    assert f is not None and agent.grad_steps > 0
    return f.local.clone(), f.exp_avg.clone(), f.exp_avg_sq.clone(), int(f.step_dev.item())


def test_deferred_evaluation_density_does_not_touch_training(torch, tmp_path):
    """2 or 4 deferred evaluation points, or no evaluation env at all: the same parameters and Adam moments, bit for bit.  The inline form draws its
    evaluation taus from the agent's own act stream, the one training acts with, so there the number of points changes the run; that difference is why
    the deferred form exists and is not asserted here."""
    a4, _ = _learn(torch, tmp_path, "d4", 10, True)
    a2, _ = _learn(torch, tmp_path, "d2", 20, True)
    a0, _ = _learn(torch, tmp_path, "d0", 10, True, with_eval=False)
    assert len(a4.eval_timesteps["greedy"]) == 4 and len(a2.eval_timesteps["greedy"]) == 2 and len(a0.eval_timesteps["greedy"]) == 0
    s4, s2, s0 = _train_state(a4), _train_state(a2), _train_state(a0)
    for other in (s2, s0):
        for x, y in zip(s4[:3], other[:3]):
            assert torch.equal(x.view(torch.int32), y.view(torch.int32))
        assert s4[3] == other[3]
    assert int(a4._act_rng.state[1]) == int(a2._act_rng.state[1]) == int(a0._act_rng.state[1])


def test_evaluate_checkpoints_equals_single_network_calls(torch, tmp_path):
    from distributional_rl_navigation_amd.iqn.deferred_eval import evaluate_checkpoints
    cfg = _cfg(3)
    dirs = []
    for j, net in enumerate(_nets()):
        d = tmp_path / f"ckpt{j}"
        d.mkdir()
        net.save(str(d))
        dirs.append(str(d))
    seeds = [5, 6, 7]
    together = evaluate_checkpoints(dirs, cfg, DEV, seeds=seeds, max_steps=60)
    assert len(together) == 3 and all(set(r) == {"greedy", "adaptive", "steps_run"} for r in together)
    for j in range(3):
        alone = evaluate_checkpoints([dirs[j]], cfg, DEV, seeds=[seeds[j]], max_steps=60)
        assert alone == [together[j]], j
    assert together[0]["greedy"]["actions"] != together[1]["greedy"]["actions"]
    assert all(r["greedy"]["n_worlds"] == 3 and len(r["adaptive"]["rewards"]) == 3 for r in together)


def test_refusals_return_invalid_without_launching(torch):
    from distributional_rl_navigation_amd import _capi
    from distributional_rl_navigation_amd.iqn.fused_act import _p, image_floats
    lib = _capi.lib()
    cfg = _cfg(2)
    G, R, T = 2, 4, 8
    env = _env(cfg, G, "f64")
    nets = _nets()[:G]
    images = _images(torch, nets)
    states = _states(torch, [1, 2])
    words = torch.zeros(G, 2, dtype=torch.int32, device=DEV)
    obs0 = env.obs.clone()
    IMG = image_floats()

    def call(h=env.h, img=images, stride=IMG, n_groups=G, rows=R, n_steps=T, st=states, obs=env.obs, w=words):
        return lib.mn_rollout_iqn_groups(h, _p(img), stride, n_groups, rows, n_steps, _p(st), None, None, _p(obs), None, None, None, None, None, None, None,
                                         _p(w), None, env._stream())
    INVALID = -1
    assert call(n_groups=3) == INVALID and call(rows=3) == INVALID and call(n_groups=1) == INVALID
    assert call(stride=IMG - 4) == INVALID and call(stride=IMG + 2) == INVALID
    assert call(st=None) == INVALID and call(img=None) == INVALID and call(obs=None) == INVALID and call(w=None) == INVALID and call(h=None) == INVALID
    assert call(n_steps=0) == INVALID
    traj = torch.zeros(T, G * R, int(env.params.N), 2, dtype=torch.float64, device=DEV)
    env.set_trajectory_trace(traj)
    assert call() == INVALID          # the attachment is consumed and the call refused ...
    torch.cuda.synchronize()
    assert states[:, 1].tolist() == [0, 0] and torch.equal(env.obs, obs0) and not words.any() and not traj.any()      # nothing was launched
    assert call() == 0                # ... so the same call now runs
    torch.cuda.synchronize()
    assert min(states[:, 1].tolist()) >= 1 and not words.any() and not traj.any()
    env.close()
