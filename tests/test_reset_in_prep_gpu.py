"""Episode resets INSIDE the next act call's preparation launch (csrc/mn_prep_reset.hip; C-ABI mn_reset_done_next_act -> MN_RESET_OWED -> mn_iqn_act_rng_env;
`VecMarineNavEnv.reset_done(under_next_act=True, eps=...)`, `fused_act(..., late_env=env)`): the resets of vector step t, the draws of act call t + 1 and the pack
of a stale weight image share one launch on the caller's stream.  Everything the loop leaves behind equals, byte for byte, what the same loop through
mn_reset_done + mn_iqn_act_rng leaves: env state of every kind, RNG rows, observations, actions, draws, the act call counter, the listed rows, the replay ring.

n = 256 and 320 envs (320: npad = 512 != n and a partly filled last wavefront), both precisions.  The episode limit makes, within 40 vector steps, steps that
finish no env, steps that finish every env (limit 1: every second step), steps that finish a handful (limit 9 with staggered episode clocks), and at least
six resets per env, so every MT19937 stream crosses the 624-word block boundary more than once."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ALWAYS = 2 ** 31 - 1
T = 40
RAW = ("mt", "mt_pos", "qcx", "qcy", "qcg", "qox", "qoy", "qor")


@pytest.fixture(scope="module")
def torch():
    import torch as t
    if not t.cuda.is_available():
        pytest.skip("no GPU")
    return t


def _env(n, precision, seed=3):
    from distributional_rl_navigation_amd.marinenav_env.vec_env import VecMarineNavEnv
    env = VecMarineNavEnv(n, seed=seed, device=DEV, precision=precision)
    env.params.max_episode_steps = 1
    env.set_attrs(num_cores=8, num_obs=10, min_start_goal_dis=40.0)
    return env


def _everything(torch, env, agent, obs):
    """What a loop leaves behind, as host arrays."""
    torch.cuda.synchronize()
    m = agent.memory
    out = {"obs": obs.cpu().numpy(), "obs_bufs": [b.cpu().numpy() for b in env._obs_bufs], "reward": env.reward.cpu().numpy(), "done": env.done.cpu().numpy(),
           "ring": [x.cpu().numpy() for x in (m.states, m.actions, m.rewards, m.next_states, m.dones)], "ring_ptr": int(m.ptr),
           "rng_state": agent._act_rng.state.cpu().numpy(), "params": torch.cat([p.detach().reshape(-1) for p in agent.qnetwork_local.parameters()]).cpu().numpy()}
    state, ep_t, tot_t = env.get_state()
    out.update(state=state, ep_t=ep_t, tot_t=tot_t, peek=env.peek_next_double())
    out["worlds"] = [(w["cores"], w["obstacles"], w["start"], w["goal"]) for w in env.get_worlds()]
    for k in RAW:
        out[k] = env.debug_read(k)
    return out


def _listed_rows(ctx, n):
    from distributional_rl_navigation_amd import _capi
    lst, cnt = np.zeros(n, np.int32), C.c_int32()
    assert _capi.lib().mn_iqn_last_greedy_rows(ctx.h, _capi.stream_ptr(ctx.device), lst.ctypes.data_as(C.POINTER(C.c_int32)), n, C.byref(cnt)) == 0
    return sorted(lst[:cnt.value].tolist())


def _loop(torch, n, precision, new_path, eps, train=False, owed_max_rows=ALWAYS):
    """T vector steps of IQNAgent.vec_step.  new_path = False: resets in front of the act kernel (mn_reset_done, mn_iqn_act_rng); True: vec_finish hands eps and n
    to reset_done(under_next_act=True, ...) with the rule set to `owed_max_rows`, and act_batch takes the owed reset along."""
    from distributional_rl_navigation_amd import _capi
    from distributional_rl_navigation_amd.iqn.agent import IQNAgent
    from distributional_rl_navigation_amd.iqn.fused_act import act_context
    env = _env(n, precision)
    agent = IQNAgent(26, 9, BATCH_SIZE=64, BUFFER_SIZE=3 * n, device=DEV, seed=11, learning_starts=0, UPDATE_EVERY=2 if train else 10 ** 9)
    agent.reset_under_act = new_path
    if new_path:
        env.set_reset_owed_max_rows(owed_max_rows)
    ctx = act_context(agent.qnetwork_local)
    obs = env.reset()
    steps = []
    for t in range(T):
        if t == 12:      # from here on: limit 9 with the episode clocks staggered -- a handful of envs (n / 9) finishes at every step
            env.params.max_episode_steps = 9
            env.set_attrs(num_cores=8, num_obs=10)
            env.set_state(episode_timesteps=np.arange(n) % 9)
        obs, reward, done, info, loss = agent.vec_step(env, obs, eps)
        owed = bool(_capi.lib().mn_reset_is_owed(env.h))
        under = env.late_rows is not None
        draws = agent._act_rng.draws(n, 32)
        torch.cuda.synchronize()
        u = draws[32 * n:].cpu().numpy()
        rows = _listed_rows(ctx, n) if eps > 0.0 else None
        if rows is not None:
            assert rows == np.nonzero(u > np.float32(eps))[0].tolist()      # the list as a set: the rows whose uniform says "greedy" (agent.py:200)
        steps.append(dict(reward=reward.cpu().numpy(), done=done.cpu().numpy(), info=info.cpu().numpy(), loss=None if loss is None else float(loss),
                          draws=draws.cpu().numpy(), counter=agent._act_rng.state.cpu().numpy(), rows=rows, owed=owed, under=under))
    env.join_reset()
    assert not _capi.lib().mn_reset_is_owed(env.h)
    agent.check_learner()
    out = dict(steps=steps, end=_everything(torch, env, agent, obs), resets_owed=env.resets_owed, launches=list(env.reset_launches))
    env.close()
    return out


_REFERENCE = {}


def _reference(torch, n, precision, eps, train=False):
    key = (n, precision, eps, train)
    if key not in _REFERENCE:
        _REFERENCE[key] = _loop(torch, n, precision, False, eps, train)
    return _REFERENCE[key]


def _equal(x, y, path=""):
    if isinstance(x, dict):
        assert x.keys() == y.keys(), path
        for k in x:
            _equal(x[k], y[k], f"{path}.{k}")
    elif isinstance(x, (list, tuple)):
        assert len(x) == len(y), path
        for i, (a, b) in enumerate(zip(x, y)):
            _equal(a, b, f"{path}[{i}]")
    elif isinstance(x, np.ndarray):
        assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), path      # byte for byte (NaN payloads and signed zeros included)
    else:
        assert x == y, path


def _same_loops(a, b):
    for t, (s0, s1) in enumerate(zip(a["steps"], b["steps"])):
        for k in ("reward", "done", "info", "loss", "draws", "counter", "rows"):
            _equal(s0[k], s1[k], f"step {t} {k}")
    _equal(a["end"], b["end"], "end")


def _episode_ends_are_of_every_kind(ref, n):
    counts = [int(s["done"].sum()) for s in ref["steps"]]
    assert 0 in counts and n in counts and any(0 < c <= n // 4 for c in counts), counts
    assert sum(counts) >= 6 * n      # resets per env: ~300 words of a 624-word block each


@pytest.mark.parametrize("eps", [1.0, 0.999, 0.5, 0.0])
@pytest.mark.parametrize("n,precision", [(256, "f64"), (320, "f64"), (256, "mixed"), (320, "mixed")])
def test_loop_through_the_fused_launch_equals_the_loop_with_resets_in_front(torch, n, precision, eps):
    ref = _reference(torch, n, precision, eps)
    _episode_ends_are_of_every_kind(ref, n)
    if eps > 0.0:
        new = _loop(torch, n, precision, True, eps)
        # every reset was left to the next act call -- except where another call had to settle it (the set_attrs / set_state of step 12 do, by design)
        assert all(s["owed"] and not s["under"] for s in new["steps"]) and new["resets_owed"] == T and new["launches"] == [T, 0]
    else:
        # eps = 0: every row goes through the network, far more than the threshold -> today's path (under the act kernel) as soon as a reset launch has
        # reported its episode count; the very first call, with nothing seen, would have gone in front and is owed instead.  Same results either way.
        new = _loop(torch, n, precision, True, eps, owed_max_rows=n // 8)
        assert new["steps"][0]["owed"] and all(s["under"] and not s["owed"] for s in new["steps"][1:]), [(s["owed"], s["under"]) for s in new["steps"]]
    _same_loops(ref, new)


@pytest.mark.parametrize("precision", ["f64", "mixed"])
def test_stale_weight_image_is_packed_inside_the_fused_launch(torch, precision):
    """A gradient step every second vector step: the act call behind it finds its weight image stale, so the fused launch has pack blocks between its reset and
    its draw blocks.  Losses and learned parameters included in the comparison."""
    ref = _reference(torch, 320, precision, 0.5, train=True)
    new = _loop(torch, 320, precision, True, 0.5, train=True)
    assert sum(s["loss"] is not None for s in ref["steps"]) >= T // 2 - 1 and new["resets_owed"] == T
    _same_loops(ref, new)


@pytest.mark.parametrize("kind", ["join_reset", "get_state", "last_done_count", "step", "reset_done", "act_with_torch_rand"])
def test_an_owed_reset_is_settled_by_whatever_touches_the_env_next(torch, kind):
    """Nothing is launched when a reset is owed; the next entry point that reads or writes the env's state pays the debt with a plain reset launch first."""
    from distributional_rl_navigation_amd import _capi
    from distributional_rl_navigation_amd.iqn.agent import IQNAgent
    L, n = _capi.lib(), 320
    outs = []
    for owe in (False, True):
        env = _env(n, "f64", seed=9)
        env.set_reset_owed_max_rows(ALWAYS)
        agent = IQNAgent(26, 9, device=DEV, seed=4)
        obs = env.reset()
        a = torch.arange(n, dtype=torch.int32, device=DEV) % 9
        env.step(a)
        env.step(a)      # limit 1: every env is done
        assert int(env.done.sum()) == n
        if owe:
            env.reset_done(under_next_act=True, eps=0.9)
            assert env.reset_owed and L.mn_reset_is_owed(env.h) == 1 and env.late_rows is None
        else:
            env.reset_done()
        extra = None
        if kind == "join_reset":
            env.join_reset()
        elif kind == "get_state":
            extra = env.get_state()
        elif kind == "last_done_count":
            extra = env.last_done_count()
        elif kind == "step":
            env.step(a)
            extra = (env.reward.cpu().numpy(), env.done.cpu().numpy())
        elif kind == "reset_done":
            env.reset_done()      # (a second reset of the same queue, as two mn_reset_done calls in a row have always been)
        else:      # an act call that is told about the env but has no preparation launch of the library's (torch.rand draws): the reset first, then the call
            agent.use_library_rng = False
            extra = agent.act_batch(env.obs, 0.3, late_env=env).cpu().numpy()
        assert L.mn_reset_is_owed(env.h) == 0
        torch.cuda.synchronize()
        outs.append(dict(extra=extra, obs=[b.cpu().numpy() for b in env._obs_bufs], state=env.get_state(), peek=env.peek_next_double(),
                         raw=[env.debug_read(k) for k in RAW]))
        env.close()
    _equal(outs[0], outs[1], kind)


def test_two_handles_interleaved(torch):
    """One agent, two envs stepped alternately: each handle's debt is its own, and the act call for one env never runs the other's resets."""
    from distributional_rl_navigation_amd import _capi
    from distributional_rl_navigation_amd.iqn.agent import IQNAgent
    outs = []
    for new_path in (False, True):
        envs = [_env(256, "f64", seed=3), _env(320, "mixed", seed=5)]
        agent = IQNAgent(26, 9, BATCH_SIZE=64, BUFFER_SIZE=4096, device=DEV, seed=11, learning_starts=0, UPDATE_EVERY=10 ** 9)
        agent.reset_under_act = new_path
        obs = []
        for e in envs:
            if new_path:
                e.set_reset_owed_max_rows(ALWAYS)
            obs.append(e.reset())
        for t in range(16):
            for i, e in enumerate(envs):
                obs[i] = agent.vec_step(e, obs[i], 0.7)[0]
            if new_path:
                assert all(_capi.lib().mn_reset_is_owed(e.h) == 1 for e in envs)
        for e in envs:
            e.join_reset()
        outs.append([_everything(torch, e, agent, o) for e, o in zip(envs, obs)])
        for e in envs:
            e.close()
    _equal(outs[0], outs[1], "interleaved")


def test_guard_preflight_still_puts_every_reset_under_the_act_kernel(torch):
    """learn_vec's first 12 vector steps force every reset under the act kernel (UnderActGuard) to test that arrangement on this box: forced-under mode wins over
    the owed rule even when the rule would owe every reset; behind the preflight the rule applies."""
    from distributional_rl_navigation_amd.iqn.agent import IQNAgent
    env = _env(320, "f64")
    env.params.max_episode_steps = 5
    env.set_attrs(num_cores=8, num_obs=10)
    env.set_reset_owed_max_rows(ALWAYS)
    agent = IQNAgent(26, 9, BATCH_SIZE=64, BUFFER_SIZE=4096, device=DEV, seed=5, learning_starts=0, UPDATE_EVERY=2)
    seen = {}

    def on_step(it, st):
        seen[it] = (list(env.reset_launches), env.resets_owed)
    agent.learn_vec(total_vector_steps=16, train_env=env, verbose=False, reset_under_act=True, on_step=on_step)
    assert agent.under_act_fallback is None
    assert seen[11] == ([0, 12], 0), seen      # every reset of the 12 preflight steps went under the act kernel
    assert seen[15] == ([4, 12], 4), seen      # ... and the four behind them rode in the next act call's preparation launch
    env.close()
