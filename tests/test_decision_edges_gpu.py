"""The two discrete decisions every learned policy ends in, held per kernel on hand-built inputs (tests/decision_edges.py): which action is greedy on an
EXACT tie -- the first maximum, like np.argmax -- and which CVaR level an adaptive row acts with when it sits ON one of `adjust_cvar_row`'s thresholds.

A. Output weight zero, bias from the table: Q is the bias bit for bit (a -0.0 bias as +0.0: `decision_edges.expected_q`) and the action np.argmax(bias) on
   every one of 70 rows (DQN: 70 and 37), with and without the Q output, in every form that ends in an argmax: the split kernel (every row, listed rows, late rows),
   the few-rows kernel, the exact-f32 kernel, the launch-shared-tau forms (wavefront per row, env-tiled), act_eval's quantile form, the actor-group
   launch, the IQN episode launches (plain, rows, eval, groups), and for DQN mn_dqn_act, mn_dqn_act_rng, the actor-group launch and the episode launches
   (single, groups).  The zero layer also takes the weight image through pow2_to_2p15's degenerate branch (max |W4| = 0).
B. Output row a copied over row b and both lifted clear of the rest (the lift asserted from a float64 evaluation alone): the two columns of the returned Q
   are bit-equal and the action is a, on every row, in every form.
C. Edge rows in `obs_dev`, one step: the `cvar` trace of the adaptive episode launches equals `decision_edges.cvar_twin` bit for bit, the eval form's
   taus are the twin's draws x that cvar, and actions / Q equal one mn_iqn_act_rng call at eps = 0 with cvar_row = the twin from the same generator state.
Nothing here has a tolerance.  The split kernel's late-rows forms take part in A only: their rows are the env's own (an episode reset runs beside the
act launch), so no hand-made row can be put in front of them."""
import copy
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import decision_edges as E      # noqa: E402
import rng_twin as T            # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F = np.float32
N = E.N_ROWS
SEED = 4242
EPS_LISTED = 1e-9                 # a row explores iff its uniform is <= eps: with this one every row of the seeds used here is listed as greedy
ALWAYS, NEVER = 2 ** 31 - 1, -1
TABLE = E.bias_table()


@pytest.fixture(scope="module")
def torch():
    import torch as t
    if not t.cuda.is_available():
        pytest.skip("no GPU")
    return t


@pytest.fixture(scope="module")
def envs(torch):
    """env(n): a reset VecMarineNavEnv of n rows, made once.  At one step per launch the state behind `obs_dev` is irrelevant; a finished env acts again."""
    from distributional_rl_navigation_amd.marinenav_env.vec_env import VecMarineNavEnv
    made = {}

    def env(n):
        if n not in made:
            made[n] = VecMarineNavEnv(n, seed=4, device=DEV, precision="f64")
            made[n].reset()
        return made[n]
    yield env
    for e in made.values():
        e.close()


def _t(torch, x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _n(x):
    return x.detach().cpu().numpy()


def _rng(torch, seed=SEED, ctr=0):
    from distributional_rl_navigation_amd.iqn.fused_act import ActRng
    rng = ActRng(0, DEV)
    rng.state.copy_(torch.tensor([seed, ctr], dtype=torch.int64))
    return rng


def _seeded_net(seed=5):
    from distributional_rl_navigation_amd.iqn.model import ObsEncoder
    return ObsEncoder(26, 9, seed=seed, device=DEV)


def _lib():
    from distributional_rl_navigation_amd import _capi
    return _capi.lib()


def _stream(torch):
    from distributional_rl_navigation_amd import _capi
    return _capi.stream_ptr(torch.device(DEV))


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


class Inputs:
    """The rows and taus every IQN form of a test acts on: 70 random observations, injected per-row taus, one launch-shared tau row, and the library's
    own draws of call {SEED, 0} (what the listed / few-rows forms, the draw path and every episode launch act with)."""

    def __init__(self, torch, envs, rows=None):
        self.rows = E.random_obs(N) if rows is None else rows
        self.obs = _t(torch, self.rows)
        self.taus_np, self.row_np = E.random_taus((N, 32)), E.random_taus((32,), seed=13)
        self.taus, self.row = _t(torch, self.taus_np), _t(torch, self.row_np)
        draws = T.act_draws(SEED, 0, N, 1.0)
        self.draws_np = draws[:N * 32].reshape(N, 32)
        assert (draws[-N:] > F(EPS_LISTED)).all()
        self.env = envs(N)

    def arm(self):
        self.env.obs.copy_(self.obs)
        return self.env


# ---- the IQN forms: name -> (returns Q?, run(torch, net, S, want_q) -> (actions, Q or None, quantiles or None) as numpy) ------------------------------------
def _fused(torch, net, S, want_q, **kw):
    from distributional_rl_navigation_amd.iqn.fused_act import fused_act
    out = fused_act(net, S.obs, 0.0, 1.0, want_qvals=want_q, **kw)
    if kw.get("want_quantiles"):
        return _n(out[0]), (_n(out[3]) if want_q else None), _n(out[1])
    return (_n(out[0]), _n(out[1]), None) if want_q else (_n(out), None, None)


def _exact(torch, net, S, want_q):
    from distributional_rl_navigation_amd.iqn.fused_act import act_context
    ctx = act_context(net)
    try:
        ctx.set_variant(0)
        return _fused(torch, net, S, want_q, taus=S.taus)
    finally:
        ctx.set_variant(ctx.DEFAULT_VARIANT)


def _listed(torch, net, S, want_q, few):
    from distributional_rl_navigation_amd.iqn.fused_act import act_context, fused_act
    assert not want_q
    ctx = act_context(net)
    ctx.set_few_rows_max(ALWAYS if few else NEVER)
    before = ctx.few_rows_launches()
    try:
        a = fused_act(net, S.obs, EPS_LISTED, 1.0, rng=_rng(torch), greedy_rows=True)
    finally:
        ctx.set_few_rows_max(None)
    assert ctx.few_rows_launches() - before == (1 if few else 0)
    return _n(a), None, None


def _rollout_plain(torch, net, env, rng, cvar, adaptive, names):
    """C-ABI mn_rollout_iqn itself (the Python surface goes through mn_rollout_iqn_rows), one step."""
    from distributional_rl_navigation_amd.episodes import trace_buffers
    from distributional_rl_navigation_amd.iqn.fused_act import act_context
    ctx = act_context(net)
    ctx.set_tau_mode(0)
    tr = trace_buffers(1, env.n_envs, DEV, names)
    p = lambda k: _p(tr[k]) if k in tr else None
    steps = torch.zeros(1, dtype=torch.int32, device=DEV)
    rc = _lib().mn_rollout_iqn(env.h, ctx.h, ctx.weights(net), 1, _p(rng.state), C.c_float(float(cvar)), int(bool(adaptive)), _p(env.obs), p("obs"), p("reward"),
                               p("done"), p("info"), p("action"), p("cvar"), p("q"), _p(steps), env._stream())
    assert rc == 0
    assert int(steps.item()) == 1
    return tr


def _episode(torch, net, S, want_q, kind):
    from distributional_rl_navigation_amd.iqn.fused_act import rollout_iqn
    env = S.arm()
    names = ("action", "cvar") + (("q",) if want_q else ())
    if kind == "plain":
        tr = _rollout_plain(torch, net, env, _rng(torch), 1.0, False, names)
    elif kind == "rows":
        tr = rollout_iqn(net, env, 1, _rng(torch), cvar_rows=torch.ones(N), adaptive_rows=torch.zeros(N, dtype=torch.bool), trace=names)
    else:
        assert want_q
        tr = rollout_iqn(net, env, 1, _rng(torch), trace=names, want_quantiles=True)
    assert tr is not None
    return _n(tr["action"][0]), (_n(tr["q"][0]) if want_q else None), (_n(tr["quantiles"][0]) if "quantiles" in tr else None)


def _eval_without_q(torch, net, S):
    """mn_rollout_iqn_eval with no Q and no quantile trace: the raw call (rollout_iqn always attaches the quantile trace with want_quantiles)."""
    from distributional_rl_navigation_amd.episodes import trace_buffers
    from distributional_rl_navigation_amd.iqn.fused_act import act_context
    env = S.arm()
    ctx = act_context(net)
    ctx.set_tau_mode(0)
    tr = trace_buffers(1, N, DEV, ("action",))
    steps = torch.zeros(1, dtype=torch.int32, device=DEV)
    rng = _rng(torch)
    rc = _lib().mn_rollout_iqn_eval(env.h, ctx.h, ctx.weights(net), 1, _p(rng.state), C.c_float(1.0), 0, None, None, _p(env.obs), None, None, None, None,
                                    _p(tr["action"]), None, None, None, None, _p(steps), env._stream())
    assert rc == 0
    torch.cuda.synchronize()
    assert rng.state.tolist() == [SEED, 1]
    return _n(tr["action"][0]), None, None


IQN_FORMS = {
    "split, injected taus": (True, lambda t, net, S, q: _fused(t, net, S, q, taus=S.taus)),
    "split, library draws": (True, lambda t, net, S, q: _fused(t, net, S, q, rng=_rng(t))),
    "split, listed rows": (False, lambda t, net, S, q: _listed(t, net, S, q, False)),
    "few-rows kernel": (False, lambda t, net, S, q: _listed(t, net, S, q, True)),
    "exact f32": (True, _exact),
    "shared taus, wavefront per row": (True, lambda t, net, S, q: _fused(t, net, S, q, taus=S.row, shared_taus="wave")),
    "shared taus, env-tiled": (True, lambda t, net, S, q: _fused(t, net, S, q, taus=S.row, shared_taus="tiled")),
    "quantiles": (True, lambda t, net, S, q: _fused(t, net, S, q, taus=S.taus, want_quantiles=True)),
    "quantiles, shared taus": (True, lambda t, net, S, q: _fused(t, net, S, q, taus=S.row, want_quantiles=True, shared_taus="wave")),
    "episode launch": (True, lambda t, net, S, q: _episode(t, net, S, q, "plain")),
    "episode launch, rows form": (True, lambda t, net, S, q: _episode(t, net, S, q, "rows")),
    "episode launch, eval form": (True, lambda t, net, S, q: _episode(t, net, S, q, "eval") if q else _eval_without_q(t, net, S)),
}
# the taus each form evaluates the network at (part B's float64 evaluation runs on all three sets)
TAUS_OF = {"split, injected taus": "taus", "exact f32": "taus", "quantiles": "taus", "shared taus, wavefront per row": "row", "shared taus, env-tiled": "row",
           "quantiles, shared taus": "row"}


def _q_bits(q, want):
    return np.array_equal(E.bits(q), np.broadcast_to(E.bits(want), q.shape))


# ---- A: the bias table -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", list(IQN_FORMS))
def test_iqn_form_on_the_bias_table(torch, envs, form):
    has_q, run = IQN_FORMS[form]
    net, S = _seeded_net(), Inputs(torch, envs)
    for name, b in TABLE:
        E.set_output(net.output_layer, None, b)
        want_a, want_q = E.expected_action(b), E.expected_q(b)
        for with_q in ((True, False) if has_q else (False,)):
            a, q, quant = run(torch, net, S, with_q)
            assert a.shape == (N,) and (a == want_a).all(), (form, name, with_q, a)
            if with_q:
                assert q.shape == (N, 9) and _q_bits(q, want_q), (form, name, q[0])
            if quant is not None:      # the bias in all 32 x 9 places
                assert quant.shape == (N, 32, 9) and _q_bits(quant, want_q), (form, name)


def test_iqn_actor_group_on_the_bias_table(torch):
    """mn_iqn_actor_group_act, one pattern per actor, one launch; eps = 0 (every row) and the listed form (eps tiny: every row is listed as greedy)."""
    from distributional_rl_navigation_amd import _capi
    from distributional_rl_navigation_amd.iqn.fused_act import act_context
    G = len(TABLE)
    assert G <= _capi.IQN_MAX_ACTORS
    nets = [_seeded_net() for _ in range(G)]
    want = np.repeat([E.expected_action(b) for _, b in TABLE], N)
    obs = _t(torch, E.random_obs(G * N))
    states = [torch.tensor([SEED, 0], dtype=torch.int64, device=DEV) for _ in range(G)]
    draws = [torch.empty(33 * N, dtype=torch.float32, device=DEV) for _ in range(G)]
    table = (_capi.MnIqnActor * G)()
    for g, row in enumerate(table):
        E.set_output(nets[g].output_layer, None, TABLE[g][1])
        ctx = act_context(nets[g])
        row.ctx, row.weights = ctx.h.value, C.cast(ctx.weights(nets[g]), C.c_void_p).value
        row.rng_state, row.draws = states[g].data_ptr(), draws[g].data_ptr()
    h = C.c_void_p()
    assert _lib().mn_iqn_actor_group_create(table, G, N, C.byref(h)) == 0
    try:
        for call, eps in enumerate((0.0, EPS_LISTED)):
            assert (T.act_draws(SEED, call, N, 1.0)[-N:] > F(eps)).all()
            actions = torch.full((G * N,), -7, dtype=torch.int32, device=DEV)
            assert _lib().mn_iqn_actor_group_act(h, _p(obs), C.c_float(1.0), C.c_float(eps), _p(actions), _stream(torch)) == 0
            a = _n(actions)
            bad = sorted({TABLE[i // N][0] for i in np.nonzero(a != want)[0]})
            assert not bad, (eps, bad)
            assert [int(s[1]) for s in states] == [call + 1] * G
    finally:
        assert _lib().mn_iqn_actor_group_destroy(h) == 0


def test_late_rows_forms_on_the_bias_table(torch):
    """The split kernel's late-rows forms (every row; listed rows): an episode reset of about a sixth of the rows runs beside the act launch, which takes
    those rows last.  Q is the bias whatever a row holds, so the launch acts on the env's own observations."""
    from distributional_rl_navigation_amd.iqn.fused_act import act_context, fused_act, late_rows_possible, late_timeouts
    from distributional_rl_navigation_amd.marinenav_env.vec_env import VecMarineNavEnv
    env = VecMarineNavEnv(N, seed=3, device=DEV, precision="f64")
    env.params.max_episode_steps = 5
    env.set_attrs(num_cores=8, num_obs=10, min_start_goal_dis=40.0)
    env.set_reset_under_act_max(ALWAYS)
    env.reset()
    env.set_state(episode_timesteps=np.arange(N) % 6)      # a sixth of the envs runs out of steps at every step (the step that finds the clock at 5)
    net = _seeded_net()
    ctx = act_context(net)
    ctx.set_few_rows_max(NEVER)      # (the few-rows kernel takes no late rows)
    assert late_rows_possible(net, N)
    rng = _rng(torch)
    a = torch.zeros(N, dtype=torch.int32, device=DEV)
    try:
        for name, b in TABLE:
            E.set_output(net.output_layer, None, b)
            for eps, with_q in ((0.0, True), (0.0, False), (EPS_LISTED, False)):
                env.step(a)
                assert 0 < int(env.done.sum()) < N
                obs = env.reset_done(under_next_act=True)
                assert env.late_rows is not None
                greedy = T.act_draws(SEED, int(rng.state[1]), N, 1.0)[-N:] > F(eps)
                out = fused_act(net, obs, eps, 1.0, rng=rng, want_qvals=with_q, late_env=env, greedy_rows=True)
                assert env.late_rows is None      # the launch took them
                a = out[0] if with_q else out
                assert greedy.sum() >= N - 1 and (_n(a)[greedy] == E.expected_action(b)).all(), (name, eps, with_q, _n(a))
                if with_q:
                    assert _q_bits(_n(out[1]), E.expected_q(b)), name
        env.join_reset()
        assert late_timeouts(net) == 0
    finally:
        ctx.set_few_rows_max(None)
        env.close()


def _iqn_images(torch, net, outputs):
    """One exported acting image per (weight or None, bias) of `outputs`, all from `net` with its output layer overwritten in turn."""
    from distributional_rl_navigation_amd.iqn.fused_act import export_image, image_floats
    img = torch.empty(len(outputs), image_floats(), dtype=torch.int32, device=DEV)
    for j, (w, b) in enumerate(outputs):
        E.set_output(net.output_layer, w, b)
        export_image(net, img[j])
    return img


def _iqn_groups(torch, envs, images, rows, **kw):
    """mn_rollout_iqn_groups, one step: every group acts on the same N rows from the generator state {SEED, 0}."""
    from distributional_rl_navigation_amd.iqn.fused_act import rollout_iqn_groups
    G = images.shape[0]
    env = envs(G * N)
    env.obs.copy_(_t(torch, np.tile(rows, (G, 1))))
    states = torch.tensor([[SEED, 0]] * G, dtype=torch.int64, device=DEV)
    tr = rollout_iqn_groups(images, env, 1, states, N, **kw)
    torch.cuda.synchronize()
    assert not tr["group_words"].any() and states[:, 1].tolist() == [1] * G and tr["steps_run"].tolist() == [1] * G
    return tr


def test_iqn_group_episode_launch_on_the_bias_table(torch, envs):
    net = _seeded_net()
    images = _iqn_images(torch, net, [(None, b) for _, b in TABLE])
    rows = E.random_obs(N)
    for names in (("action", "q"), ("action",)):
        tr = _iqn_groups(torch, envs, images, rows, trace=names)
        a = _n(tr["action"][0]).reshape(len(TABLE), N)
        for g, (name, b) in enumerate(TABLE):
            assert (a[g] == E.expected_action(b)).all(), (name, names, a[g])
            if "q" in names:
                assert _q_bits(_n(tr["q"][0]).reshape(len(TABLE), N, 9)[g], E.expected_q(b)), name


# ---- DQN ---------------------------------------------------------------------------------------------------------------------------------------------
def _dqn(torch):
    from distributional_rl_navigation_amd.dqn import DQNPolicy
    return DQNPolicy.load(os.path.join(E.GOLD, "pretrained_DQN_seed3", "q_net.npz"), device=DEV)


def _dqn_act(torch, pol, obs, env, want_q):
    if want_q:
        q, a = pol._fused(obs, True, True)
        q2 = pol.q_values(obs)
        assert torch.equal(q.view(torch.int32), q2.view(torch.int32))
        return _n(a), _n(q)
    return _n(pol.act_batch(obs)), None


def _dqn_act_rng(torch, pol, obs, env, want_q):
    if want_q:
        a, _, q = pol.act_rng(obs, SEED, 3, 0.0, want_q=True)
        return _n(a), _n(q)
    return _n(pol.act_rng(obs, SEED, 3, 0.0)), None


def _dqn_episode(torch, pol, obs, env, want_q):
    env.obs.copy_(obs)
    tr = pol.rollout(env, 1, trace=("action", "q") if want_q else ("action",))
    assert tr is not None
    return _n(tr["action"][0]), (_n(tr["q"][0]) if want_q else None)


DQN_FORMS = {"mn_dqn_act": _dqn_act, "mn_dqn_act_rng at eps 0": _dqn_act_rng, "episode launch": _dqn_episode}
DQN_ROWS = (N, 37)


@pytest.mark.parametrize("n", DQN_ROWS)
@pytest.mark.parametrize("form", list(DQN_FORMS))
def test_dqn_form_on_the_bias_table(torch, envs, form, n):
    pol = _dqn(torch)
    obs = _t(torch, E.random_obs(n, seed=3))
    for name, b in TABLE:
        E.set_output(pol.q_net.q_net[4], None, b)
        for with_q in (True, False):
            a, q = DQN_FORMS[form](torch, pol, obs, envs(n), with_q)
            assert a.shape == (n,) and (a == E.expected_action(b)).all(), (form, name, with_q, a)
            if with_q:
                assert q.shape == (n, 9) and _q_bits(q, E.expected_q(b)), (form, name, q[0])


def _dqn_group_act(torch, pols, obs, n):
    """mn_dqn_actor_group_act at eps = 0 with every image stale: actions [G n]."""
    from distributional_rl_navigation_amd import _capi
    G = len(pols)
    assert G <= _capi.DQN_MAX_ACTORS
    floats = int(_lib().mn_dqn_image_floats())
    images = [torch.zeros(floats, dtype=torch.float32, device=DEV) for _ in range(G)]
    ptrs = []
    table = (_capi.MnDqnActor * G)()
    for g, row in enumerate(table):
        st, _ = pols[g]._image(torch.device(DEV))
        ptrs.append((C.c_void_p * 18)(*[st["ptrs"][i] for i in range(18)]))
        row.weights, row.image, row.seed = C.cast(ptrs[g], C.c_void_p).value, images[g].data_ptr(), SEED + g
    h = C.c_void_p()
    assert _lib().mn_dqn_actor_group_create(table, G, n, C.byref(h)) == 0
    try:
        actions = torch.full((G * n,), -7, dtype=torch.int32, device=DEV)
        calls = (C.c_uint64 * G)(*range(G))
        assert _lib().mn_dqn_actor_group_act(h, _p(obs), C.c_float(0.0), (1 << G) - 1, calls, _p(actions), _stream(torch)) == 0
        return _n(actions)
    finally:
        assert _lib().mn_dqn_actor_group_destroy(h) == 0


@pytest.mark.parametrize("n", DQN_ROWS)
def test_dqn_actor_group_on_the_bias_table(torch, n):
    pols = []
    for _, b in TABLE:
        pols.append(_dqn(torch))
        E.set_output(pols[-1].q_net.q_net[4], None, b)
    a = _dqn_group_act(torch, pols, _t(torch, E.random_obs(len(TABLE) * n, seed=3)), n)
    want = np.repeat([E.expected_action(b) for _, b in TABLE], n)
    bad = sorted({TABLE[i // n][0] for i in np.nonzero(a != want)[0]})
    assert not bad, bad


def _dqn_images(torch, pol, outputs):
    from distributional_rl_navigation_amd.dqn.policy import image_floats
    img = torch.empty(len(outputs), image_floats(), dtype=torch.float32, device=DEV)
    for j, (w, b) in enumerate(outputs):
        E.set_output(pol.q_net.q_net[4], w, b)
        pol.export_image(img[j])
    return img


def _dqn_groups(torch, envs, images, rows, names):
    from distributional_rl_navigation_amd.dqn.policy import rollout_dqn_groups
    G, n = images.shape[0], len(rows)
    env = envs(G * n)
    env.obs.copy_(_t(torch, np.tile(rows, (G, 1))))
    return rollout_dqn_groups(images, env, 1, n, trace=names)


@pytest.mark.parametrize("n", DQN_ROWS)
def test_dqn_group_episode_launch_on_the_bias_table(torch, envs, n):
    images = _dqn_images(torch, _dqn(torch), [(None, b) for _, b in TABLE])
    rows = E.random_obs(n, seed=3)
    for names in (("action", "q"), ("action",)):
        tr = _dqn_groups(torch, envs, images, rows, names)
        a = _n(tr["action"][0]).reshape(len(TABLE), n)
        for g, (name, b) in enumerate(TABLE):
            assert (a[g] == E.expected_action(b)).all(), (name, names, a[g])
            if "q" in names:
                assert _q_bits(_n(tr["q"][0]).reshape(len(TABLE), n, 9)[g], E.expected_q(b)), name


# ---- B: ties through the real arithmetic ---------------------------------------------------------------------------------------------------------------
def _tied_iqn_net(torch, S, a, b):
    """The seeded network with output row a copied over row b and both lifted; the lift's condition is asserted from float64 alone."""
    net = _seeded_net()
    w0, b0 = _n(net.output_layer.weight).copy(), _n(net.output_layer.bias).copy()
    obs64 = S.obs.double()
    tau_sets = [S.taus.double(), S.row.double().view(1, 32).expand(N, 32), _t(torch, S.draws_np).double()]

    def q64_of():
        net64 = copy.deepcopy(net).double()
        with torch.no_grad():
            return np.concatenate([_n(net64.get_qvals(obs64, 1.0, taus=t)) for t in tau_sets])
    lift, q64 = E.tie_lift(net.output_layer, w0, b0, a, b, q64_of)
    assert q64.shape == (3 * N, 9) and E.clear_of_the_others(q64, a, b) and (q64.argmax(axis=1) == a).all()
    assert lift <= 4.0 * np.abs(q64).max()      # a small power of two: the low bits of Q stay alive
    return net, lift


def _columns_tie(q, a, b):
    return np.array_equal(E.bits(np.ascontiguousarray(q[..., a])), E.bits(np.ascontiguousarray(q[..., b])))


@pytest.mark.parametrize("a,b", E.PAIRS)
def test_iqn_forms_on_duplicated_output_rows(torch, envs, a, b):
    S = Inputs(torch, envs)
    net, lift = _tied_iqn_net(torch, S, a, b)
    with_q = {}
    for form, (has_q, run) in IQN_FORMS.items():
        if not has_q:
            continue
        act, q, quant = run(torch, net, S, True)
        assert not np.array_equal(q[0], q[1]) and np.isfinite(q).all(), form      # (the real arithmetic: Q depends on the row)
        assert _columns_tie(q, a, b), (form, "max |Q[a] - Q[b]|", float(np.abs(q[:, a] - q[:, b]).max()))
        if quant is not None:
            assert _columns_tie(quant, a, b), form
        assert (act == a).all(), (form, act)
        with_q[form] = act
    for form, (has_q, run) in IQN_FORMS.items():      # without the Q output: the actions of the Q-returning run on the same taus
        act, _, _ = run(torch, net, S, False)
        assert (act == a).all() and np.array_equal(act, with_q[form if has_q else "split, library draws"]), (form, act)


def test_iqn_group_launches_on_duplicated_output_rows(torch, envs):
    """One group / actor per pair: the grouped episode launch (Q trace) and the actor-group act launch (actions only)."""
    from distributional_rl_navigation_amd import _capi
    from distributional_rl_navigation_amd.iqn.fused_act import act_context, export_image, image_floats
    S = Inputs(torch, envs)
    nets = [_tied_iqn_net(torch, S, a, b)[0] for a, b in E.PAIRS]
    img = torch.empty(len(nets), image_floats(), dtype=torch.int32, device=DEV)
    for j, net in enumerate(nets):
        export_image(net, img[j])
    tr = _iqn_groups(torch, envs, img, S.rows, trace=("action", "q"))
    act, q = _n(tr["action"][0]).reshape(-1, N), _n(tr["q"][0]).reshape(-1, N, 9)
    tr2 = _iqn_groups(torch, envs, img, S.rows, trace=("action",))
    for g, (a, b) in enumerate(E.PAIRS):
        assert _columns_tie(q[g], a, b) and (act[g] == a).all(), (a, b)
    assert np.array_equal(_n(tr2["action"][0]).reshape(-1, N), act)
    G = len(nets)
    states = [torch.tensor([SEED, 0], dtype=torch.int64, device=DEV) for _ in range(G)]
    draws = [torch.empty(33 * N, dtype=torch.float32, device=DEV) for _ in range(G)]
    table = (_capi.MnIqnActor * G)()
    for g, row in enumerate(table):
        ctx = act_context(nets[g])
        row.ctx, row.weights = ctx.h.value, C.cast(ctx.weights(nets[g]), C.c_void_p).value
        row.rng_state, row.draws = states[g].data_ptr(), draws[g].data_ptr()
    h = C.c_void_p()
    assert _lib().mn_iqn_actor_group_create(table, G, N, C.byref(h)) == 0
    try:
        actions = torch.full((G * N,), -7, dtype=torch.int32, device=DEV)
        assert _lib().mn_iqn_actor_group_act(h, _p(_t(torch, np.tile(S.rows, (G, 1)))), C.c_float(1.0), C.c_float(0.0), _p(actions), _stream(torch)) == 0
        assert np.array_equal(_n(actions).reshape(G, N), act)      # the same rows, the same draws {SEED, 0}: the episode launch's actions
    finally:
        assert _lib().mn_iqn_actor_group_destroy(h) == 0


def _tied_dqn(torch, obs, a, b):
    pol = _dqn(torch)
    layer = pol.q_net.q_net[4]
    w0, b0 = _n(layer.weight).copy(), _n(layer.bias).copy()

    def q64_of():
        with torch.no_grad():
            return _n(copy.deepcopy(pol.q_net).double()(obs.double()))
    lift, q64 = E.tie_lift(layer, w0, b0, a, b, q64_of)
    assert E.clear_of_the_others(q64, a, b) and (q64.argmax(axis=1) == a).all() and lift <= 4.0 * np.abs(q64).max()
    return pol


@pytest.mark.parametrize("n", DQN_ROWS)
def test_dqn_forms_on_duplicated_output_rows(torch, envs, n):
    rows = E.random_obs(n, seed=3)
    obs = _t(torch, rows)
    pols = []
    for a, b in E.PAIRS:
        pol = _tied_dqn(torch, obs, a, b)
        pols.append(pol)
        for form, run in DQN_FORMS.items():
            act, q = run(torch, pol, obs, envs(n), True)
            assert not np.array_equal(q[0], q[1]) and np.isfinite(q).all(), form
            assert _columns_tie(q, a, b), (form, "max |Q[a] - Q[b]|", float(np.abs(q[:, a] - q[:, b]).max()))
            assert (act == a).all(), (form, act)
            act2, _ = run(torch, pol, obs, envs(n), False)
            assert np.array_equal(act2, act), form
    want = np.repeat([a for a, _ in E.PAIRS], n)
    assert np.array_equal(_dqn_group_act(torch, pols, _t(torch, np.tile(rows, (len(pols), 1))), n), want)
    img = torch.empty(len(pols), int(_lib().mn_dqn_image_floats()), dtype=torch.float32, device=DEV)
    for j, pol in enumerate(pols):
        pol.export_image(img[j])
    tr = _dqn_groups(torch, envs, img, rows, ("action", "q"))
    q = _n(tr["q"][0]).reshape(-1, n, 9)
    for g, (a, b) in enumerate(E.PAIRS):
        assert _columns_tie(q[g], a, b), (a, b)
    assert np.array_equal(_n(tr["action"][0]), want)
    assert np.array_equal(_n(_dqn_groups(torch, envs, img, rows, ("action",))["action"][0]), want)


# ---- C: adjust_cvar on its thresholds ------------------------------------------------------------------------------------------------------------------
CTR = 7      # the act call counter the launches start from


@pytest.fixture(scope="module")
def edges(torch):
    rows, names = E.cvar_edge_rows()
    twin = E.cvar_twin(rows)
    skip32, below32 = E.cvar_decisions_f32(rows)
    skip64, below64 = E.cvar_decisions_f64(rows)
    assert np.array_equal(skip32, skip64) and np.array_equal(below32, below64)      # before any kernel runs (also held on the CPU)
    return rows, names, twin


def test_adjust_cvar_batch_on_the_device_equals_the_twin_bitwise(torch, edges):
    """The kernel comment's claim about PyTorch on ROCm: two squares rounded separately, a correctly rounded root, a multiply by 0.1f."""
    from distributional_rl_navigation_amd.iqn.agent import IQNAgent
    rows, names, twin = edges
    got = _n(IQNAgent(26, 9, device=DEV, seed=5).adjust_cvar_batch(_t(torch, rows)))
    bad = [(names[i], got[i], twin[i]) for i in np.nonzero(E.bits(got) != E.bits(twin))[0]]
    assert not bad, bad


def _act_reference(torch, net, rows, cvar, seed, ctr, quantiles=False):
    """One mn_iqn_act_rng call at eps = 0 on `rows` with cvar_row = `cvar` from the generator state {seed, ctr}: (actions, Q[, quantiles]) as numpy."""
    from distributional_rl_navigation_amd.iqn.fused_act import fused_act
    out = fused_act(net, _t(torch, rows), 0.0, _t(torch, cvar), rng=_rng(torch, seed, ctr), want_qvals=True, want_quantiles=quantiles)
    return (_n(out[0]), _n(out[3]), _n(out[1])) if quantiles else (_n(out[0]), _n(out[1]))


def _cvar_bad(names, got, want):
    return [(names[i], got[i], want[i]) for i in np.nonzero(E.bits(got) != E.bits(want))[0]]


@pytest.mark.parametrize("form", ["plain", "rows", "eval"])
def test_adaptive_episode_launch_on_the_cvar_thresholds(torch, envs, edges, form):
    from distributional_rl_navigation_amd.iqn.fused_act import rollout_iqn
    rows, names, twin = edges
    net = _seeded_net()
    env = envs(N)
    env.obs.copy_(_t(torch, rows))
    rng = _rng(torch, SEED, CTR)
    want_cv = twin
    if form == "plain":
        tr = _rollout_plain(torch, net, env, rng, 0.375, True, ("action", "cvar", "q"))      # (the scalar cvar is not used by an adaptive launch)
    elif form == "rows":      # the adaptive flag on the odd rows, a fixed cvar_row on the even ones
        odd = np.arange(N) % 2 == 1
        fixed = np.linspace(0.1, 1.0, N).astype(F)
        want_cv = np.where(odd, twin, fixed)
        assert (want_cv[odd] != fixed[odd]).any()
        tr = rollout_iqn(net, env, 1, rng, cvar_rows=_t(torch, fixed), adaptive_rows=_t(torch, odd), trace=("action", "cvar", "q"))
    else:
        tr = rollout_iqn(net, env, 1, rng, adaptive=True, trace=("action", "cvar", "q"), want_quantiles=True)
    assert tr is not None and rng.state.tolist() == [SEED, CTR + 1]
    assert not _cvar_bad(names, _n(tr["cvar"][0]), want_cv), _cvar_bad(names, _n(tr["cvar"][0]), want_cv)
    ref = _act_reference(torch, net, rows, want_cv, SEED, CTR, quantiles=form == "eval")
    assert np.array_equal(_n(tr["action"][0]), ref[0])
    assert np.array_equal(E.bits(_n(tr["q"][0])), E.bits(ref[1]))
    if form == "eval":
        draws = T.act_draws(SEED, CTR, N, want_cv)[:N * 32].reshape(N, 32)
        assert np.array_equal(E.bits(_n(tr["taus"][0])), E.bits(draws))
        assert np.array_equal(E.bits(_n(tr["quantiles"][0])), E.bits(ref[2]))
    assert len(np.unique(ref[0])) > 1      # (the seeded network does choose among actions on these rows)


def test_adaptive_group_episode_launch_on_the_cvar_thresholds(torch, envs, edges):
    """mn_rollout_iqn_groups, two groups of 35 rows with a network, a seed and a counter each."""
    from distributional_rl_navigation_amd.iqn.fused_act import export_image, image_floats, rollout_iqn_groups
    rows, names, twin = edges
    R = N // 2
    nets, seeds, ctrs = [_seeded_net(5), _seeded_net(6)], [SEED, SEED + 1], [CTR, CTR + 4]
    img = torch.empty(2, image_floats(), dtype=torch.int32, device=DEV)
    for j, net in enumerate(nets):
        export_image(net, img[j])
    env = envs(N)
    env.obs.copy_(_t(torch, rows))
    states = torch.tensor(list(zip(seeds, ctrs)), dtype=torch.int64, device=DEV)
    tr = rollout_iqn_groups(img, env, 1, states, R, adaptive_rows=torch.ones(N, dtype=torch.bool), trace=("action", "cvar", "q"))
    torch.cuda.synchronize()
    assert states.tolist() == [[seeds[0], ctrs[0] + 1], [seeds[1], ctrs[1] + 1]] and not tr["group_words"].any()
    assert not _cvar_bad(names, _n(tr["cvar"][0]), twin), _cvar_bad(names, _n(tr["cvar"][0]), twin)
    for g in range(2):
        sl = slice(g * R, (g + 1) * R)
        a, q = _act_reference(torch, nets[g], rows[sl], twin[sl], seeds[g], ctrs[g])
        assert np.array_equal(_n(tr["action"][0])[sl], a), g
        assert np.array_equal(E.bits(_n(tr["q"][0])[sl]), E.bits(q)), g
