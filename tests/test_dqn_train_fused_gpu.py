"""The DQN baseline's fused HIP gradient step (csrc/dqn_train.hip, dqn/fused_train.py) on the GPU: the reference's own step (G11), eager
PyTorch and a float64 evaluation as yardsticks; the in-launch batch draw, determinism, the one optimizer state shared with the eager path,
the act kernel's weight image after a fused step, learn_vec and the train_dqn driver end to end."""
import copy
import json
import os
import zipfile

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), "golden")
LR = 1e-4


@pytest.fixture(scope="module")
def torch():
    import torch as t
    if not t.cuda.is_available():
        pytest.skip("no GPU")
    return t


def _agent(torch, batch=32, buffer_size=20_000, seed=3):
    from distributional_rl_navigation_amd.dqn import DQNAgent
    return DQNAgent(device="cuda:0", buffer_size=buffer_size, batch_size=batch, seed=seed, fused_train=True)


@pytest.fixture(scope="module")
def ring(torch):
    """A replay ring filled from a real rollout of the HIP env (random actions, auto-reset): (states, actions, rewards, next_states, dones)."""
    from distributional_rl_navigation_amd.marinenav_env.vec_env import VecMarineNavEnv
    env = VecMarineNavEnv(1024, seed=5, device="cuda:0")
    ag = _agent(torch, buffer_size=16_384)
    obs = env.reset()
    for _ in range(16):
        a = ag.act_batch(obs, 1.0)
        nxt, r, d, _ = env.step(a)
        ag.memory.add_vector_step(obs, a, r, nxt, d)
        obs = env.reset_done()
    env.close()
    m = ag.memory
    assert m.size == 16_384 and float(m.dones.sum()) > 0
    return tuple(t.clone() for t in (m.states, m.actions, m.rewards, m.next_states, m.dones))


def _load_ring(ag, ring):
    m = ag.memory
    n = ring[0].shape[0]
    for dst, src in zip((m.states, m.actions, m.rewards, m.next_states, m.dones), ring):
        dst[:n].copy_(src)
    m.size, m.ptr = n, n % m.capacity


def _flat(ag, what="param"):
    ps = list(ag.q_net.parameters())
    if what == "grad":
        return np.concatenate([p.grad.detach().double().cpu().numpy().ravel() for p in ps])
    return np.concatenate([p.detach().double().cpu().numpy().ravel() for p in ps])


def _f64_step(torch, ag, batch):
    """Loss and clipped gradient of DQN.train in float64 from the agent's current networks."""
    import torch.nn.functional as F
    q = copy.deepcopy(ag.q_net).double()
    t = copy.deepcopy(ag.q_net_target).double()
    obs, act, rew, nxt, done = (x.double() if x.dtype == torch.float32 else x for x in batch)
    with torch.no_grad():
        y = rew + (1 - done) * ag.gamma * t(nxt).max(dim=1)[0].reshape(-1, 1)
    loss = F.smooth_l1_loss(torch.gather(q(obs), 1, act.long()), y)
    loss.backward()
    norm = float(torch.nn.utils.clip_grad_norm_(q.parameters(), ag.max_grad_norm))
    return float(loss.detach()), np.concatenate([p.grad.cpu().numpy().ravel() for p in q.parameters()]), norm


class _State:
    """Snapshot / restore of a fused agent's whole training state (parameters, target, Adam moments and step)."""

    def __init__(self, ag):
        ft = ag._fused_trainer()
        self.ag, self.t = ag, [x.clone() for x in (ft.local, ft.target, ft.exp_avg, ft.exp_avg_sq, ft.step_dev)]

    def restore(self):
        ft = self.ag._fused
        for d, s in zip((ft.local, ft.target, ft.exp_avg, ft.exp_avg_sq, ft.step_dev), self.t):
            d.copy_(s)
        self.ag._train_path = "hip"      # the device counter is authoritative: the next eager step takes it over
        self.ag.policy.weights_changed()


def _compare_step(torch, ag, idx, state):
    """Fused and eager step on rows `idx` from the same state, both against float64; returns the gradient norm before clipping."""
    m = ag.memory
    batch = tuple(t[idx] for t in (m.states, m.actions, m.rewards, m.next_states, m.dones))
    state.restore()
    loss64, g64, norm = _f64_step(torch, ag, batch)
    loss_f = float(ag.train_fused(idx))
    g_f, p_f = _flat(ag, "grad"), _flat(ag)
    state.restore()
    loss_e = float(ag.train(batch))
    g_e, p_e = _flat(ag, "grad"), _flat(ag)
    ag._enter_train_path("hip")
    lbar = 1.5 * abs(loss_e - loss64) + 1e-6
    assert abs(loss_f - loss64) <= lbar, (loss_f, loss_e, loss64)
    gbar = 1.5 * np.abs(g_e - g64).max() + 1e-6
    assert np.abs(g_f - g64).max() <= gbar, (np.abs(g_f - g64).max(), np.abs(g_e - g64).max())
    big = np.abs(g64) > 100 * gbar
    assert np.abs(p_f - p_e)[big].max(initial=0) <= 2e-6
    assert np.abs(p_f - p_e).max() <= 2 * LR
    return norm


def test_g11_through_the_kernel(torch):
    """G11 (the reference's own DQN.train step, tests/golden/make_golden_dqn.py) with its batch placed in the ring and passed as idx_dev."""
    Z = np.load(os.path.join(G, "g11_dqn_train.npz"))
    ag = _agent(torch, batch=32, buffer_size=64)
    ag.load(os.path.join(G, "pretrained_DQN_seed3", "q_net.npz"))
    ag.q_net_target.load_state_dict({k[len("tgt_"):]: torch.from_numpy(Z[k]) for k in Z.files if k.startswith("tgt_")})
    m = ag.memory
    for dst, k in zip((m.states, m.actions, m.rewards, m.next_states, m.dones), ("observations", "actions", "rewards", "next_observations", "dones")):
        dst[:32].copy_(torch.from_numpy(Z["batch_" + k]).view(32, -1))
    m.size = 32
    idx = torch.arange(32, device="cuda:0")
    batch = tuple(t[idx] for t in (m.states, m.actions, m.rewards, m.next_states, m.dones))
    loss64, g64, _ = _f64_step(torch, ag, batch)
    loss = float(ag.train_fused(idx))
    names = [n for n, _ in ag.q_net.named_parameters()]
    g_ref = np.concatenate([Z["grad_" + n].astype(np.float64).ravel() for n in names])
    p_ref = np.concatenate([Z["after_" + n].astype(np.float64).ravel() for n in names])
    g_k, p_k = _flat(ag, "grad"), _flat(ag)
    # the golden values are float32 eager: the kernel's error against float64 must be of their size
    assert abs(loss - loss64) <= 1.5 * abs(float(Z["loss"]) - loss64) + 1e-6, (loss, float(Z["loss"]), loss64)
    gbar = 1.5 * np.abs(g_ref - g64).max() + 1e-6
    assert np.abs(g_k - g64).max() <= gbar
    big = np.abs(g64) > 100 * gbar
    assert big.sum() > 100
    assert np.abs(p_k - p_ref)[big].max() <= 2e-6
    assert np.abs(p_k - p_ref).max() <= 2 * LR
    assert int(ag._fused.step_dev.item()) == 1 and ag.n_updates == 1


def test_fused_against_eager_any_batch_and_20_steps(torch, ring):
    ag = _agent(torch, batch=32)
    _load_ring(ag, ring)
    gen = torch.Generator(device="cuda:0").manual_seed(11)
    state = _State(ag)
    norms = []
    for B in (1, 5, 16, 17, 32, 64, 100, 256):
        idx = torch.randperm(ring[0].shape[0], device="cuda:0", generator=gen)[:B]
        norms.append(_compare_step(torch, ag, idx, state))
    # a steeper output layer from the same start: gradient norms above max_norm = 10, so the clip acts
    state.restore()
    with torch.no_grad():
        ag.q_net.q_net[4].weight.mul_(100.0)
    steep = _State(ag)
    for B in (17, 256):
        idx = torch.randperm(ring[0].shape[0], device="cuda:0", generator=gen)[:B]
        norms.append(_compare_step(torch, ag, idx, steep))
    assert max(norms) > 10 and min(norms) < 10, norms      # both a clipping and a non-clipping step
    # 20 consecutive steps each way from the same state
    idxs = [torch.randperm(ring[0].shape[0], device="cuda:0", generator=gen)[:64] for _ in range(20)]
    m = ag.memory
    state.restore()
    for idx in idxs:
        ag.train_fused(idx)
    p_f = _flat(ag)
    state.restore()
    for idx in idxs:
        ag.train(tuple(t[idx] for t in (m.states, m.actions, m.rewards, m.next_states, m.dones)))
    p_e = _flat(ag)
    d = np.abs(p_f - p_e)
    assert d.max() <= 6.4e-3 and np.median(d) <= 1e-5, (d.max(), np.median(d))
    assert np.abs(p_f - state.t[0].double().cpu().numpy()).max() > 1e-4      # the steps moved the weights


def test_in_launch_sampling_is_mn_iqn_sample(torch, ring):
    import ctypes as C
    from distributional_rl_navigation_amd import _capi
    ag = _agent(torch, batch=100)
    _load_ring(ag, ring)
    ft = ag._fused_trainer()
    ft.rng_state.copy_(torch.tensor([1234567, 41], dtype=torch.int64))
    st = ft.rng_state.clone()
    want = torch.empty(100, dtype=torch.int64, device="cuda:0")
    rc = _capi.lib().mn_iqn_sample(ring[0].shape[0], 100, C.c_void_p(st.data_ptr()), C.c_void_p(want.data_ptr()), None, 0,
                                   _capi.stream_ptr(torch.device("cuda:0")))
    assert rc == 0
    state = _State(ag)
    ag.train_fused()
    got = ft.last_idx.clone()
    assert torch.equal(got, want) and got.unique().numel() == 100
    assert ft.rng_state.tolist() == [1234567, 42] and st.tolist() == [1234567, 42]
    p_sampled, g_sampled, loss_s = ft.local.clone(), ft.grad.clone(), ft.loss.clone()
    state.restore()
    ag.train_fused(got)
    assert torch.equal(ft.local, p_sampled) and torch.equal(ft.grad, g_sampled) and torch.equal(ft.loss, loss_s)


def test_determinism_200_sampled_steps(torch, ring):
    ags = []
    for _ in range(2):
        ag = _agent(torch, batch=256, seed=7)
        _load_ring(ag, ring)
        for _ in range(200):
            ag.train()
        ags.append(ag._fused)
    a, b = ags
    for x, y in ((a.local, b.local), (a.exp_avg, b.exp_avg), (a.exp_avg_sq, b.exp_avg_sq), (a.step_dev, b.step_dev), (a.rng_state, b.rng_state)):
        assert torch.equal(x, y)
    assert int(a.step_dev.item()) == 200 and int(a.rng_state[1].item()) == 200


def test_one_optimizer_state_and_fresh_act_image(torch, ring):
    gen = torch.Generator(device="cuda:0").manual_seed(5)
    idxs = [torch.randperm(ring[0].shape[0], device="cuda:0", generator=gen)[:32] for _ in range(7)]
    obs = ring[0][:512]
    mixed, eager = _agent(torch, seed=21), _agent(torch, seed=21)
    eager.fused_train = False
    for ag in (mixed, eager):
        _load_ring(ag, ring)
    m = mixed.memory
    q_before = mixed.policy.q_values(obs).clone()      # builds the act kernel's weight image
    for k in range(3):
        mixed.train_fused(idxs[k])
    ft = mixed._fused
    p0 = next(iter(mixed.q_net.parameters()))
    assert mixed.optimizer.state[p0]["exp_avg"].data_ptr() == ft.exp_avg.data_ptr()
    assert float(mixed.optimizer.state[p0]["exp_avg"].abs().sum()) > 0
    # the act path sees the weights the kernel wrote
    with torch.no_grad():
        q_eager = mixed.q_net(obs)
    q_k = mixed.policy.q_values(obs)
    assert (q_eager - q_before).abs().max() > 1e-4
    torch.testing.assert_close(q_k, q_eager, rtol=0, atol=1e-5)
    a = mixed.policy.act_batch(obs)
    top2 = q_eager.sort(dim=1).values
    clear = (top2[:, -1] - top2[:, -2]) > 1e-4
    assert torch.equal(a[clear].long(), q_eager.argmax(dim=1)[clear])
    # fused x3, eager x1 (the optimizer takes the step count over), fused x3  vs  7 eager steps
    mixed.train(tuple(t[idxs[3]] for t in (m.states, m.actions, m.rewards, m.next_states, m.dones)))
    assert float(mixed.optimizer.state[p0]["step"]) == 4
    for k in range(4, 7):
        mixed.train_fused(idxs[k])
    assert int(ft.step_dev.item()) == 7
    me = eager.memory
    for idx in idxs:
        eager.train(tuple(t[idx] for t in (me.states, me.actions, me.rewards, me.next_states, me.dones)))
    d = np.abs(_flat(mixed) - _flat(eager))
    assert d.max() <= 6.4e-3 and np.median(d) <= 1e-5, (d.max(), np.median(d))


def test_learn_vec_fused_and_checkpoint(torch, tmp_path):
    from distributional_rl_navigation_amd.dqn import DQNAgent, DQNPolicy
    from distributional_rl_navigation_amd.marinenav_env.vec_env import VecMarineNavEnv
    env = VecMarineNavEnv(2048, seed=0, device="cuda:0")
    ag = DQNAgent(device="cuda:0", buffer_size=50_000, batch_size=64, learning_starts=4096, train_freq=2, target_update_interval=20480, seed=3,
                  fused_train=True)
    before = [p.detach().clone() for p in ag.q_net.parameters()]
    stats = ag.learn_vec(total_vector_steps=30, train_env=env)
    assert ag._fused is not None and int(ag._fused.step_dev.item()) == 14
    assert stats["n_updates"] == 14 and np.isfinite(stats["mean_loss"])
    assert all(float((p.detach() - q).abs().max()) > 0 for p, q in zip(ag.q_net.parameters(), before))
    ag.save(str(tmp_path))
    pol = DQNPolicy.load(os.path.join(tmp_path, "policy.pth"), device="cuda:0")
    obs = env.reset()
    assert torch.equal(pol.act_batch(obs), ag.policy.act_batch(obs))
    ag2 = DQNAgent(device="cuda:0", buffer_size=64, seed=9)
    ag2.load(os.path.join(tmp_path, "policy.pth"))
    for p, q in zip(ag.q_net_target.parameters(), ag2.q_net_target.parameters()):
        assert torch.equal(p, q)
    big = DQNAgent(device="cuda:0", buffer_size=8192, batch_size=300, learning_starts=2048, train_freq=1, seed=3, fused_train=True)
    st = big.learn_vec(total_vector_steps=3, train_env=env)      # B > 256: the eager step
    assert big._fused is None and st["n_updates"] == 2 and np.isfinite(st["mean_loss"])
    env.close()


def test_train_dqn_end_to_end_tiny(torch, tmp_path):
    from distributional_rl_navigation_amd import train_dqn
    from distributional_rl_navigation_amd.dqn import DQNPolicy
    from distributional_rl_navigation_amd.experiments import run_experiment
    cfg = tmp_path / "config_DQN.json"
    cfg.write_text(json.dumps({"agent": "DQN", "seed": [1], "total_timesteps": 3_000_000, "eval_freq": 10_000, "save_dir": str(tmp_path / "runs")}))
    train_dqn.main(["-C", str(cfg), "--n-envs", "1024", "--total-grad-steps", "300", "--n-evals", "2"])
    (stamp,) = os.listdir(tmp_path / "runs")
    d = tmp_path / "runs" / stamp / "seed_1"
    for f in ("trial_config.json", "training_schedule.json", "evaluations.npz", "latest_model.zip", "best_model.zip"):
        assert (d / f).exists(), f
    tc = json.loads((d / "trial_config.json").read_text())
    assert tc["seed"] == 1 and tc["batched"]["total_grad_steps"] == 300 and tc["batched"]["batch"] == 256
    ev = np.load(d / "evaluations.npz", allow_pickle=True)
    assert set(ev.files) == {"timesteps", "rewards", "times", "energies", "successes", "actions"}
    assert ev["timesteps"].dtype == np.int64 and ev["timesteps"].shape == (2,) and ev["timesteps"][-1] == 3_000_000
    for k in ("rewards", "times", "energies"):
        assert ev[k].dtype == np.float64 and ev[k].shape == (2, 30), k
    assert ev["successes"].dtype == bool and ev["successes"].shape == (2, 30)
    assert ev["actions"].dtype == object and len(ev["actions"]) == 2 and len(ev["actions"][0]) == 30
    assert "policy.pth" in zipfile.ZipFile(d / "best_model.zip").namelist()
    pol = DQNPolicy.load(str(d / "best_model.zip"), device="cuda:0")
    res, _ = run_experiment(None, n_obs=6, n_cores=4, num=8, seed=15, policies=("DQN",), dqn=pol)
    assert len(res["DQN"]["success"]) == 8
