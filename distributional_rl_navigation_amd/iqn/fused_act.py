"""Python side of the fused IQN act kernel (csrc/iqn_act.hip, `mn_iqn_act` / `mn_iqn_act_rng`).

Every network that acts through the kernel owns one `ActContext` (C-ABI `mn_iqn_ctx`): the permuted weight image
the kernel stages into LDS is cached there and rebuilt only after the weights changed.  Changes made through
PyTorch (optimizer.step, load_state_dict, copy_) are detected from the parameters' version counters; writers that
bypass PyTorch (the fused HIP Adam step, csrc/iqn_train.hip) call `weights_changed(net)`.
"""
import ctypes as C
import weakref

import torch

from .. import _capi
from ..episodes import EPISODE_TRACES, trace_buffers

_ORDER = ("velocity_encoder", "goal_encoder", "sensor_encoder", "cos_embedding", "hidden_layer", "hidden_layer_2", "output_layer")


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _params(net):
    # (through the module / parameter dicts: nn.Module.__getattr__ is a Python-level fallback lookup, 28 of them per act call were 15 us of a 90-us vector step at 4 096 envs)
    mods = net._modules
    out = []
    for name in _ORDER:
        ps = mods[name]._parameters
        out.append(ps["weight"]); out.append(ps["bias"])
    return out


class ActContext:
    """`mn_iqn_ctx` of one network on one device."""

    def __init__(self, device):
        self.device = torch.device(device)
        h = C.c_void_p()
        with torch.cuda.device(self.device):
            rc = _capi.lib().mn_iqn_create(C.byref(h))
        if rc:
            raise _capi.MarineNavHipError(f"mn_iqn_create failed ({rc})")
        self.h = h
        self._sig = None
        self.variant = self.DEFAULT_VARIANT
        self.tau_mode = 0
        self.greedy_rows = True
        self.few_rows_max = self.FEW_ROWS_MAX_DEFAULT
        self._ptrs = (C.c_void_p * 14)()
        self._fin = weakref.finalize(self, _capi.lib().mn_iqn_destroy, h)

    def __deepcopy__(self, memo):      # a copied network gets its own context lazily (act_context)
        return None

    def __reduce__(self):
        return (type(None), ())

    def weights(self, net):
        """HOST array of the 14 device pointers; marks the cached image stale when a parameter was re-allocated or
        written through PyTorch since the last call."""
        ps = _params(net)
        sig = tuple((t.data_ptr(), t._version) for t in ps)
        if sig != self._sig:
            for i, t in enumerate(ps):
                assert t.is_cuda and t.is_contiguous() and t.dtype == torch.float32
                self._ptrs[i] = t.data_ptr()
            self._sig = sig
            self.invalidate()
        return self._ptrs

    def invalidate(self):
        _capi.lib().mn_iqn_weights_changed(self.h)

    DEFAULT_VARIANT = 2

    def set_variant(self, variant):
        """2 = the split-f16 kernel (default: three f16 MFMA products per float32 product, float32-class accuracy, ~3x faster),
        0 = the exact-f32 16x16x4 MFMA kernel (A / B measurements, tests)."""
        rc = _capi.lib().mn_iqn_set_variant(self.h, int(variant))
        if rc:
            raise _capi.MarineNavHipError(f"mn_iqn_set_variant failed ({rc})")
        self.variant = int(variant)

    def set_greedy_rows(self, on):
        """True (default): an act call that returns nothing but actions runs the network only on the rows that do not explore -- the preparation
        launch writes the exploring rows' actions and lists the others (C-ABI mn_iqn_set_greedy_rows).  False: every row is evaluated.  Same
        actions, draws and call counter either way."""
        if bool(on) == self.greedy_rows:
            return
        rc = _capi.lib().mn_iqn_set_greedy_rows(self.h, int(bool(on)))
        if rc:
            raise _capi.MarineNavHipError(f"mn_iqn_set_greedy_rows failed ({rc})")
        self.greedy_rows = bool(on)

    FEW_ROWS_MAX_DEFAULT = 256      # = MN_IQN_FEW_ROWS_MAX_DEFAULT (include/marinenav_hip.h)
    FEW_ROWS_ALWAYS = 2 ** 31 - 1

    def set_few_rows_max(self, rows=None):
        """The act launch of the listed rows runs as the few-rows kernel (csrc/iqn_act_few.h: no LDS weight image, two wavefronts per row) while the
        list is expected to hold at most `rows` rows, (1 - eps) n (C-ABI mn_iqn_set_few_rows_max).  None: the library's default; negative: never;
        FEW_ROWS_ALWAYS: always.  Same actions, draws and call counter either way."""
        rows = self.FEW_ROWS_MAX_DEFAULT if rows is None else int(rows)
        rc = _capi.lib().mn_iqn_set_few_rows_max(self.h, rows)
        if rc:
            raise _capi.MarineNavHipError(f"mn_iqn_set_few_rows_max failed ({rc})")
        self.few_rows_max = rows

    def few_rows_launches(self):
        """Act launches of this context that ran as the few-rows kernel so far (C-ABI mn_iqn_few_rows_launches)."""
        out = C.c_int64()
        rc = _capi.lib().mn_iqn_few_rows_launches(self.h, C.byref(out))
        if rc:
            raise _capi.MarineNavHipError(f"mn_iqn_few_rows_launches failed ({rc})")
        return out.value

    def set_tau_mode(self, mode):
        """0 = every observation row its own 32 taus (default, the reference's per-call draw); 1 = one set of 32 taus per launch:
        layer 1 of the network becomes a constant of the launch (C-ABI mn_iqn_set_tau_mode; split-f16 kernel only); 2 = the same
        with the wavefront-per-row kernel for every batch size (1 switches to the environment-tiled kernel for large batches); 3 = the
        environment-tiled kernel for every batch size."""
        if int(mode) == self.tau_mode:
            return
        rc = _capi.lib().mn_iqn_set_tau_mode(self.h, int(mode))
        if rc:
            raise _capi.MarineNavHipError(f"mn_iqn_set_tau_mode failed ({rc})")
        self.tau_mode = int(mode)

    def set_grid(self, max_workgroups):
        """0 = one persistent workgroup per CU (default); > 0 = up to that many shorter workgroups, so that other streams'
        kernels get CUs while an act launch is in flight (C-ABI mn_iqn_set_grid)."""
        rc = _capi.lib().mn_iqn_set_grid(self.h, int(max_workgroups))
        if rc:
            raise _capi.MarineNavHipError(f"mn_iqn_set_grid failed ({rc})")
        self.__dict__.pop("_late_ok", None)      # (late_rows_possible: rows per wavefront follow the grid)

    def refresh(self, net):
        """Rebuild the cached weight image now (current stream) if it is stale -- see mn_iqn_refresh."""
        stream = _capi.stream_ptr(self.device)
        rc = _capi.lib().mn_iqn_refresh(self.h, self.weights(net), stream)
        if rc:
            raise _capi.MarineNavHipError(f"mn_iqn_refresh failed ({rc})")

    def profile_begin(self, max_launches):
        rc = _capi.lib().mn_iqn_profile_begin(self.h, int(max_launches))
        if rc:
            raise _capi.MarineNavHipError(f"mn_iqn_profile_begin failed ({rc})")

    def profile_end(self):
        ms, nl = C.c_double(), C.c_int32()
        stream = _capi.stream_ptr(self.device)
        rc = _capi.lib().mn_iqn_profile_end(self.h, stream, C.byref(ms), C.byref(nl))
        if rc:
            raise _capi.MarineNavHipError(f"mn_iqn_profile_end failed ({rc})")
        return ms.value, nl.value


def act_context(net):
    """The network's own act context (created on first use, on the device its parameters live on)."""
    dev = net.output_layer.weight.device
    ctx = getattr(net, "_act_ctx", None)
    if ctx is None or ctx.device != dev:
        ctx = ActContext(dev)
        object.__setattr__(net, "_act_ctx", ctx)      # not a Module / Parameter: keep it out of state_dict
    return ctx


def weights_changed(net):
    """Tell the act path that `net`'s weights were written outside PyTorch's version tracking (HIP kernels)."""
    ctx = getattr(net, "_act_ctx", None)
    if ctx is not None:
        ctx.invalidate()


def _taus(net, n, device, cvar, taus, generator):
    if taus is None:
        taus = torch.rand(n, net.K, device=device, generator=generator)
    taus = taus.to(device=device, dtype=torch.float32)
    if torch.is_tensor(cvar):
        taus = taus * cvar.to(device).view(-1, 1)
    elif cvar != 1.0:
        taus = taus * cvar
    return taus.contiguous()


class ActRng:
    """State of the library's own tau / exploration draws for `fused_act(..., rng=...)`: {seed, call counter} on the
    device plus the [33 n] scratch buffer the draws of a call are written to."""

    def __init__(self, seed, device):
        self.state = torch.tensor([int(seed) & 0x7FFFFFFFFFFFFFFF, 0], dtype=torch.int64, device=device)
        self._draws = {}

    def draws(self, n, K):
        buf = self._draws.get(n)
        if buf is None:
            buf = self._draws[n] = torch.empty(n * (K + 1), dtype=torch.float32, device=self.state.device)
        return buf


def _arm_late_rows(ctx, late_env, n, want_quantiles):
    """`late_env`: a VecMarineNavEnv whose `reset_done(under_next_act=True)` is still running on its own stream while `states` (its
    observation buffer) goes into this act launch.  The launch is told which rows are being rewritten (mn_iqn_set_late_rows) and takes them
    last; a kernel form that cannot do that waits for the reset instead.  Returns True if the launch that follows must be joined afterwards."""
    if late_env is None:
        return False
    lr = late_env.take_late_rows()
    if lr is None:
        return False
    mask, ready, tick = lr
    rc = 1 if want_quantiles else _capi.lib().mn_iqn_set_late_rows(ctx.h, _p(mask), C.c_void_p(ready), C.c_uint32(tick), n)
    if rc == 1:
        late_env.join_reset()
        return False
    if rc:
        raise _capi.MarineNavHipError(f"mn_iqn_set_late_rows failed ({rc})")
    return True


def late_rows_possible(net, n, shared_taus=False):
    """Whether an act launch of `n` rows of `net` takes late rows (the split-f16 kernel with per-row taus, at most 64 rows per wavefront): what
    `IQNAgent.vec_step` asks before it puts an episode reset under the next act kernel -- for any other form the reset stays in front."""
    if shared_taus:
        return False
    ctx = act_context(net)
    key = (int(n), ctx.variant)
    cache = ctx.__dict__.setdefault("_late_ok", {})
    if key not in cache:
        probe = torch.zeros(1, dtype=torch.int32, device=ctx.device)      # (pointers are not dereferenced by the query)
        mode, ctx.tau_mode = ctx.tau_mode, None
        ctx.set_tau_mode(0)
        rc = _capi.lib().mn_iqn_set_late_rows(ctx.h, _p(probe), _p(probe), C.c_uint32(0), int(n))
        _capi.lib().mn_iqn_set_late_rows(ctx.h, None, None, C.c_uint32(0), 0)
        if mode is not None:
            ctx.set_tau_mode(mode)
        cache[key] = rc == 0
    return cache[key]


def late_timeouts(net):
    """Waits of late rows that ran out in `net`'s act context (0 in a healthy run): C-ABI mn_iqn_late_timeouts.  Synchronises the stream."""
    ctx = act_context(net)
    out = C.c_uint32()
    dev = next(net.parameters()).device
    rc = _capi.lib().mn_iqn_late_timeouts(ctx.h, _capi.stream_ptr(dev), C.byref(out))
    if rc:
        raise _capi.MarineNavHipError(f"mn_iqn_late_timeouts failed ({rc})")
    return out.value


def late_timeouts_peek(net):
    """The same count WITHOUT synchronising (mn_iqn_late_timeouts_peek: what the launches executed so far have reported through a host-mapped word)."""
    out = C.c_uint32()
    rc = _capi.lib().mn_iqn_late_timeouts_peek(act_context(net).h, C.byref(out))
    if rc:
        raise _capi.MarineNavHipError(f"mn_iqn_late_timeouts_peek failed ({rc})")
    return out.value


def set_late_bound_ms(net, ms):
    """Bound of a late row's wait for its reset (mn_iqn_set_late_bound_ms; default 500 ms)."""
    rc = _capi.lib().mn_iqn_set_late_bound_ms(act_context(net).h, C.c_double(ms))
    if rc:
        raise _capi.MarineNavHipError(f"mn_iqn_set_late_bound_ms failed ({rc})")


@torch.no_grad()
def fused_act(net, states, eps=0.0, cvar=1.0, taus=None, generator=None, want_qvals=False, rng=None, want_quantiles=False,
              shared_taus=False, late_env=None, greedy_rows=None):
    """IQNAgent.act for states [n, 26] on the GPU in ONE kernel: encoders, cosine embedding, Hadamard
    product, hidden layers, mean over K = 32 taus, argmax and epsilon-greedy.
    Returns actions [n] int32; with want_qvals (actions, Q [n, 9]); with want_quantiles -- the batched
    IQNAgent.act_eval (agent.py:217-236) -- (actions, quantiles [n, 32, 9], taus [n, 32, 1]) (+ Q if want_qvals).
    `taus` [n, 32] may be injected; otherwise, with `rng` (an ActRng) the library draws taus and exploration uniforms
    in its own preparation launch (no torch.rand kernels), and without it they come from torch.rand on `generator`.
    `shared_taus` (opt-in): ONE set of 32 taus (x the scalar `cvar`) for all n rows of the call instead of 32 per row -- layer 1 of
    the network becomes a constant of the launch (mn_iqn_set_tau_mode; 216 instead of 372 matrix instructions per row).  Injected
    `taus` are then [32]; a per-row `cvar` tensor (adaptive policies) needs per-row taus and keeps the default mode.
    `greedy_rows` (None: as the network's context is set, on by default): with `rng`, `eps` > 0 and nothing but actions asked for, only the rows
    that do not explore go through the network (ActContext.set_greedy_rows); False evaluates every row.  Same results."""
    assert states.is_cuda and states.dtype == torch.float32 and states.is_contiguous()
    n = states.shape[0]
    dev = states.device
    ctx = act_context(net)
    shared = bool(shared_taus) and not torch.is_tensor(cvar) and ctx.variant == 2
    # mode 1: the library picks the kernel form (from 65 536 rows up the MFMA columns are environments, iqn_act_tiled.h; below, one
    # wavefront per row); shared_taus="wave" / "tiled" pin a form (modes 2 / 3: A / B measurements, tests)
    ctx.set_tau_mode({"wave": 2, "tiled": 3}.get(shared_taus, 1) if shared else 0)
    actions = torch.empty(n, dtype=torch.int32, device=dev)
    q = torch.empty(n, net.action_size, dtype=torch.float32, device=dev) if want_qvals else None
    quant = torch.empty(n, net.K, net.action_size, dtype=torch.float32, device=dev) if want_quantiles else None
    stream = _capi.stream_ptr(dev)
    if greedy_rows is not None:
        ctx.set_greedy_rows(greedy_rows)
    joined_after = _arm_late_rows(ctx, late_env, n, want_quantiles)      # (after set_tau_mode: the form of THIS launch decides)
    # an env that left its resets to this call (reset_done(under_next_act=True, eps=...)): the library's own draws have a preparation launch that runs them;
    # every other path reads `states` behind a plain reset launch
    owed = late_env is not None and hasattr(late_env, "take_owed_reset") and late_env.take_owed_reset()
    if owed and not (taus is None and rng is not None):
        late_env.join_reset()
        owed = False
    if taus is None and rng is not None:
        cv_row = cvar.to(device=dev, dtype=torch.float32).contiguous() if torch.is_tensor(cvar) else None
        draws = rng.draws(n, net.K)
        args = (_p(states), ctx.weights(net), _p(rng.state), _p(draws), _p(cv_row), C.c_float(1.0 if cv_row is not None else float(cvar)), C.c_float(float(eps)),
                _p(actions), _p(q), _p(quant), n, net.K, stream)
        rc = _capi.lib().mn_iqn_act_rng_env(ctx.h, late_env.h, *args) if owed else _capi.lib().mn_iqn_act_rng(ctx.h, *args)
        if rc:
            raise _capi.MarineNavHipError(f"mn_iqn_act_rng{'_env' if owed else ''} failed ({rc})")
        t = draws[:net.K].view(1, net.K).expand(n, net.K) if shared else draws[:n * net.K].view(n, net.K)
    elif shared:
        t1 = (torch.rand(net.K, device=dev, generator=generator) if taus is None else taus.to(device=dev, dtype=torch.float32).reshape(-1))
        assert t1.numel() == net.K, "shared_taus: one row of K taus"
        t1 = (t1 * cvar if cvar != 1.0 else t1).contiguous()
        u = torch.rand(n, device=dev, generator=generator) if eps > 0.0 else None
        rc = _capi.lib().mn_iqn_act(ctx.h, _p(states), _p(t1), ctx.weights(net), _p(q), _p(u), C.c_float(float(eps)),
                                    _p(actions), _p(quant), n, net.K, stream)
        if rc:
            raise _capi.MarineNavHipError(f"mn_iqn_act failed ({rc})")
        t = t1.view(1, net.K).expand(n, net.K)
    else:
        if taus is None and eps > 0.0:      # one RNG launch for the n x K taus and the n exploration uniforms
            buf = torch.rand(n * (net.K + 1), device=dev, generator=generator)
            t = _taus(net, n, dev, cvar, buf[:n * net.K].view(n, net.K), None)
            u = buf[n * net.K:]
        else:
            t = _taus(net, n, dev, cvar, taus, generator)
            u = torch.rand(n, device=dev, generator=generator) if eps > 0.0 else None
        rc = _capi.lib().mn_iqn_act(ctx.h, _p(states), _p(t), ctx.weights(net), _p(q), _p(u), C.c_float(float(eps)),
                                    _p(actions), _p(quant), n, net.K, stream)
        if rc:
            raise _capi.MarineNavHipError(f"mn_iqn_act failed ({rc})")
    if joined_after:      # later work on this stream (the next step reads every row) comes after the reset launch's end
        late_env.join_reset()
    out = (actions,)
    if want_quantiles:
        out += (quant, t.clone().view(n, net.K, 1))       # (.clone(): the library's draw buffer is reused by the next call)
    if want_qvals:
        out += (q,)
    return out if len(out) > 1 else actions


@torch.no_grad()
def rollout_iqn(net, env, n_steps, rng, cvar=1.0, adaptive=False, shared_taus=False,
                trace=("reward", "done", "info", "action", "cvar", "q"), cvar_rows=None, adaptive_rows=None, want_quantiles=False):
    """Every env's CURRENT episode of `env` (a VecMarineNavEnv) under the IQN policy of `net` for up to `n_steps` steps in ONE launch (C-ABI
    mn_rollout_iqn): per step what `fused_act(net, env.obs, 0.0, cvar, rng=rng, shared_taus=shared_taus)` would choose -- `cvar` a float, or with
    `adaptive` IQNAgent.adjust_cvar_batch of each row -- then the env step.  No resets: a finished env idles (reward 0, done 1, terminal info,
    action -1 in the traces; its cvar / Q / obs entries stay NaN / 0).  `rng` (an ActRng) advances as that loop would advance it.
    `cvar_rows` ([n] float tensor) / `adaptive_rows` ([n] bool tensor): per-env cvar and adaptive flag (C-ABI mn_rollout_iqn_rows) -- what a loop of
    `fused_act(net, env.obs, 0.0, torch.where(adaptive_rows, adjust_cvar_batch(env.obs), cvar_rows), rng=rng)` would choose; a per-row cvar tensor
    keeps fused_act on per-row taus whatever `shared_taus` says, and so does this call.
    `want_quantiles`: the batched IQNAgent.act_eval instead (C-ABI mn_rollout_iqn_eval) -- per step what `fused_act(..., want_quantiles=True)` chooses (Q =
    the mean of the per-tau outputs; can differ from the acting form in the last bit) -- with the traces "quantiles" [n_steps][n][32][9] and "taus"
    [n_steps][n][32] of what it chose from (NaN behind an env's end).  "traj" among the traces (f64 envs): [n_steps][n][N][2], every step's sub-step
    positions while the env is alive -- the loop's `env.get_trajectory()`.
    Returns the requested traces ([n_steps][n], Q [n_steps][n][9]), `final_obs` and `steps_run` (the longest episode), or None when the
    library refuses the form (the exact-f32 variant, launch-shared taus: the caller runs the loop instead)."""
    T, n, dev = int(n_steps), env.n_envs, env.device
    ctx = act_context(net)
    per_row = cvar_rows is not None or adaptive_rows is not None
    ctx.set_tau_mode(1 if (shared_taus and not adaptive and not per_row and ctx.variant == 2) else 0)      # the form fused_act would pick for the loop
    cv_rows = cvar_rows.to(device=dev, dtype=torch.float32).contiguous() if cvar_rows is not None else None
    ad_rows = adaptive_rows.to(device=dev, dtype=torch.uint8).contiguous() if adaptive_rows is not None else None
    assert cv_rows is None or cv_rows.numel() == n
    assert ad_rows is None or ad_rows.numel() == n
    if want_quantiles:
        trace = tuple(trace) + tuple(k for k in ("quantiles", "taus") if k not in trace)
    else:
        assert "quantiles" not in trace and "taus" not in trace, "the quantile / tau traces need want_quantiles=True"
    tr = trace_buffers(T, n, dev, trace, n_actions=net.action_size, n_taus=net.K, n_substeps=int(env.params.N))
    p = lambda k: _p(tr[k]) if k in tr else None
    steps = torch.zeros(1, dtype=torch.int32, device=dev)
    args = (env.h, ctx.h, ctx.weights(net), T, _p(rng.state), C.c_float(float(cvar)), int(bool(adaptive)), _p(cv_rows), _p(ad_rows), _p(env.obs),
            p("obs"), p("reward"), p("done"), p("info"), p("action"), p("cvar"), p("q"))
    env.set_trajectory_trace(tr.get("traj"))      # last before the launch, which consumes it whatever it returns
    if want_quantiles:
        rc = _capi.lib().mn_rollout_iqn_eval(*args, p("quantiles"), p("taus"), _p(steps), env._stream())
    else:
        rc = _capi.lib().mn_rollout_iqn_rows(*args, _p(steps), env._stream())
    if rc == -1:      # MN_ERR_INVALID: a form the rollout does not reproduce
        noise = getattr(env, "obs_noise", None)
        if want_quantiles and noise is not None and not noise.is_off:      # not a form to fall back from: the caller asked for noise and would lose it silently
            raise _capi.MarineNavHipError("rollout_iqn(want_quantiles=True): the capture form (mn_rollout_iqn_eval) has no observation-noise instantiation -- "
                                          f"detach it (env.set_obs_noise(None)) or run the loop with env.perturb: {_capi.lib().mn_last_error(env.h).decode()}")
        return None
    if rc:
        raise _capi.MarineNavHipError(f"mn_rollout_iqn_{'eval' if want_quantiles else 'rows'} failed ({rc})")
    out = dict(tr)
    out["final_obs"] = env.obs
    out["steps_run"] = int(steps.item())
    return out


def image_floats():
    """32-bit words of one acting weight image (C-ABI mn_iqn_image_floats): the row length of `rollout_iqn_groups`' `images`."""
    return int(_capi.lib().mn_iqn_image_floats())


@torch.no_grad()
def export_image(net, out):
    """A copy of `net`'s acting weight image -- what `rollout_iqn` would act with now -- in `out`, an [image_floats()] uint32 (or int32) tensor on the
    net's device (C-ABI mn_iqn_export_image): rebuilt first if the weights changed, then one device copy on the current stream, no host synchronisation.
    Raises for the forms the episode launches do not reproduce (the exact-f32 variant, launch-shared taus)."""
    ctx = act_context(net)
    assert out.is_cuda and out.device == ctx.device and out.is_contiguous() and out.element_size() == 4 and out.numel() == image_floats()
    rc = _capi.lib().mn_iqn_export_image(ctx.h, ctx.weights(net), _p(out), _capi.stream_ptr(ctx.device))
    if rc:
        raise _capi.MarineNavHipError(f"mn_iqn_export_image failed ({rc})")
    return out


@torch.no_grad()
def rollout_iqn_groups(images, env, n_steps, rng_states, rows_per_group, cvar_rows=None, adaptive_rows=None, trace=EPISODE_TRACES):
    """`rollout_iqn` for MANY networks in ONE launch (C-ABI mn_rollout_iqn_groups): rows [g * rows_per_group, (g + 1) * rows_per_group) of `env` act
    with `images[g]` (a [G][>= image_floats()] 4-byte tensor of `export_image` rows) and `rng_states[g]` ([G][2] int64: {seed, counter}, the state of
    an ActRng; each counter advances by its group's longest episode), their taus keyed by the row's index inside the group.  Group g gets, bit for bit, what
    `rollout_iqn(net_g, env_g, n_steps, ActRng(seed_g), cvar_rows=..., adaptive_rows=...)` gets on an env of its own with the group's worlds.
    `cvar_rows` / `adaptive_rows`: [n] over ALL rows (None: cvar 1 / not adaptive).  Returns the requested traces ([n_steps][n] ...), `final_obs`
    and `steps_run`, an int32 [G] DEVICE tensor (nothing here synchronises with the host)."""
    T, n, dev, R = int(n_steps), env.n_envs, env.device, int(rows_per_group)
    assert images.is_cuda and images.dim() == 2 and images.element_size() == 4 and images.stride(1) == 1
    assert rng_states.is_cuda and rng_states.dtype == torch.int64 and rng_states.is_contiguous() and rng_states.shape == (images.shape[0], 2)
    G = images.shape[0]
    cv_rows = cvar_rows.to(device=dev, dtype=torch.float32).contiguous() if cvar_rows is not None else None
    ad_rows = adaptive_rows.to(device=dev, dtype=torch.uint8).contiguous() if adaptive_rows is not None else None
    assert cv_rows is None or cv_rows.numel() == n
    assert ad_rows is None or ad_rows.numel() == n
    assert "quantiles" not in trace and "taus" not in trace and "traj" not in trace, "the grouped launch records no quantile / tau / trajectory traces"
    tr = trace_buffers(T, n, dev, trace)
    p = lambda k: _p(tr[k]) if k in tr else None
    steps = torch.zeros(G, dtype=torch.int32, device=dev)
    words = env.__dict__.get("_group_words")      # the launch's tickets: zeroed once, left zero by every launch
    if words is None or words.shape[0] < G:
        words = env._group_words = torch.zeros(G, 2, dtype=torch.int32, device=dev)
    rc = _capi.lib().mn_rollout_iqn_groups(env.h, _p(images), images.stride(0), G, R, T, _p(rng_states), _p(cv_rows), _p(ad_rows), _p(env.obs), p("obs"),
                                           p("reward"), p("done"), p("info"), p("action"), p("cvar"), p("q"), _p(words), _p(steps), env._stream())
    if rc:
        raise _capi.MarineNavHipError(f"mn_rollout_iqn_groups failed ({rc}): {_capi.lib().mn_last_error(env.h).decode()}")
    out = dict(tr)
    out["final_obs"] = env.obs
    out["steps_run"] = steps
    out["group_words"] = words[:G]
    return out


@torch.no_grad()
def fused_qvals(net, states, cvar=1.0, taus=None, generator=None):
    """Q(s, .) = mean over K = 32 quantile samples (model.py:188-191) for states [n, 26] on the GPU."""
    assert states.is_cuda and states.dtype == torch.float32
    states = states.contiguous()
    n = states.shape[0]
    ctx = act_context(net)
    ctx.set_tau_mode(0)
    t = _taus(net, n, states.device, cvar, taus, generator)
    q = torch.empty(n, net.action_size, dtype=torch.float32, device=states.device)
    stream = _capi.stream_ptr(states.device)
    rc = _capi.lib().mn_iqn_act(ctx.h, _p(states), _p(t), ctx.weights(net), _p(q), None, C.c_float(0.0), None, None, n, net.K,
                                stream)
    if rc:
        raise _capi.MarineNavHipError(f"mn_iqn_act failed ({rc})")
    return q
