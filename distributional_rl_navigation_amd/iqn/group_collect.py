"""Many IQN actors per launch: the host side of `mn_iqn_actor_group_*` (csrc/iqn_act.hip, csrc/iqn_act_group.h, csrc/replay.hip).

`CollectorGroup(agents, stacked_env)` is the collect phase of G agents in lockstep -- the seeds of one config -- whose envs are STACKED in one
`VecMarineNavEnv` of G n rows, agent g owning rows [g n, (g + 1) n): per vector step one `act` (one preparation launch that rebuilds the stale weight
images and makes every agent's draws, one act launch with the agent as the second grid dimension) and one `append` (every agent's transitions into its own
replay ring) instead of G of each; the env step and the episode resets are the stacked env's own single launches.  The grouped kernels run the single
calls' bodies, so every agent's actions, draws, generator state, weight image and ring are bit for bit what `agent.act_batch` and
`train_env.step_append` leave for that agent alone, and grouped and single calls (an inline evaluation's `act_batch`) interleave freely.  What a launch has
in common must be equal among the agents: the rows per agent, the exploration rate and cvar of the call, the greedy-rows switch, the ring's capacity and
write position.
"""
import ctypes as C

import torch

from .. import _capi

MAX_ACTORS = _capi.IQN_MAX_ACTORS


def _p(t):
    return C.c_void_p(t.data_ptr())


def check_agents(agents, n_rows_total=None):
    """ValueError, in words that name the difference, unless `agents` can collect through one stacked env (of `n_rows_total` rows, if given).  Reads
    attributes only: nothing touches a device."""
    agents = list(agents)
    if not 1 <= len(agents) <= MAX_ACTORS:
        raise ValueError(f"a collector group holds 1..{MAX_ACTORS} agents, not {len(agents)}")
    if len({id(a) for a in agents}) != len(agents):
        raise ValueError("a collector group cannot hold the same agent twice: its two actors would write the same buffers")
    first = agents[0]
    for i, a in enumerate(agents):
        dev = torch.device(a.device)
        if dev.type != "cuda":
            raise ValueError(f"collector group: agent {i} is on device {dev}; the agents must be on one GPU")
        if dev != torch.device(first.device):
            raise ValueError(f"collector group: agent {i} is on device {dev} and agent 0 on {torch.device(first.device)}; the agents must be on one GPU")
    for i, a in enumerate(agents):
        if not (a.use_fused_act and a.use_library_rng):
            raise ValueError(f"collector group: agent {i} does not act through the fused act kernel with the library's generator (use_fused_act, "
                             "use_library_rng): the grouped act launch has no other form")
        if a.n_step != 1:
            raise ValueError(f"collector group: agent {i} has n_step = {a.n_step}; the grouped append stores 1-step transitions (n_step must be 1)")
        if a.shared_taus:
            raise ValueError(f"collector group: agent {i} acts with launch-shared taus (shared_taus): the grouped act launch draws per-row taus")
        ctx = getattr(a.qnetwork_local, "_act_ctx", None)      # (a network without a context yet gets the default variant)
        if ctx is not None and ctx.variant != 2:
            raise ValueError(f"collector group: agent {i} acts with variant {ctx.variant} of the act kernel; the grouped act launch is the split-f16 form (variant 2)")
        if a.distributed:
            raise ValueError(f"collector group: agent {i} is a distributed (shared) learner: its ranks collect in separate processes")
    common = (("greedy-rows switch (act_greedy_rows_only)", lambda a: bool(a.act_greedy_rows_only)), ("ring capacity", lambda a: a.memory.capacity),
              ("ring write position (ptr)", lambda a: a.memory.ptr))
    for what, get in common:
        for i, a in enumerate(agents[1:], 1):
            if get(a) != get(first):
                raise ValueError(f"collector group: agent {i} differs from agent 0 in {what} ({get(a)!r} against {get(first)!r}); a grouped launch has one {what}")
    if n_rows_total is not None and (n_rows_total < len(agents) or n_rows_total % len(agents)):
        raise ValueError(f"collector group: a stacked env of {n_rows_total} rows does not divide into {len(agents)} equal groups of rows")
    return agents


class CollectorGroup:
    def __init__(self, agents, stacked_env):
        self.agents = check_agents(agents, int(stacked_env.n_envs))
        from .fused_act import ActRng, act_context
        self.env = stacked_env
        self.device = torch.device(self.agents[0].device)
        G = len(self.agents)
        self.n = n = int(stacked_env.n_envs) // G
        self._handle = None
        self.ctxs, self._sigs = [], []
        table = (_capi.MnIqnActor * G)()
        for row, ag in zip(table, self.agents):
            net, m = ag.qnetwork_local, ag.memory
            ctx = act_context(net)
            ctx.set_tau_mode(0)
            ctx.set_greedy_rows(ag.act_greedy_rows_only)
            if ag._act_rng is None:      # (as act_batch makes it)
                ag._act_rng = ActRng(ag.gen.initial_seed(), self.device)
            for t in (m.states, m.actions, m.rewards, m.next_states, m.dones):
                assert t.is_cuda and t.is_contiguous()
            assert m.states.dtype == torch.float32 and m.actions.dtype == torch.int64 and m.dones.dtype == torch.float32
            ptrs = ctx.weights(net)
            self.ctxs.append(ctx)
            self._sigs.append(tuple(ptrs))
            row.ctx, row.weights = ctx.h.value, C.cast(ptrs, C.c_void_p).value
            row.rng_state, row.draws = ag._act_rng.state.data_ptr(), ag._act_rng.draws(n, net.K).data_ptr()
            row.ring_states, row.ring_next_states, row.ring_actions = m.states.data_ptr(), m.next_states.data_ptr(), m.actions.data_ptr()
            row.ring_rewards, row.ring_dones = m.rewards.data_ptr(), m.dones.data_ptr()
        h = C.c_void_p()
        with torch.cuda.device(self.device):
            rc = _capi.lib().mn_iqn_actor_group_create(table, G, n, C.byref(h))
        if rc:
            raise _capi.MarineNavHipError(f"mn_iqn_actor_group_create failed ({rc}): the actors' contexts, draws, generator states and rings must be their own")
        self._handle = h

    def __len__(self):
        return len(self.agents)

    def close(self):
        if getattr(self, "_handle", None):
            _capi.lib().mn_iqn_actor_group_destroy(self._handle)
            self._handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @torch.no_grad()
    def act(self, obs, eps, cvar=1.0):
        """`agent.act_batch(obs[g n : (g + 1) n], eps, cvar)` of every agent g: actions [G n] int32 (device)."""
        assert obs.is_cuda and obs.dtype == torch.float32 and obs.is_contiguous() and obs.shape[0] == len(self.agents) * self.n
        for i, (ag, ctx, sig) in enumerate(zip(self.agents, self.ctxs, self._sigs)):
            if getattr(ag.qnetwork_local, "_act_ctx", None) is not ctx or tuple(ctx.weights(ag.qnetwork_local)) != sig:      # (weights: marks the image stale after a PyTorch write)
                raise ValueError(f"collector group: the network of agent {i} was replaced or re-allocated since the group was built; build a new group")
            ctx.set_tau_mode(0)
            ctx.set_greedy_rows(ag.act_greedy_rows_only)
        actions = torch.empty(obs.shape[0], dtype=torch.int32, device=obs.device)
        rc = _capi.lib().mn_iqn_actor_group_act(self._handle, _p(obs), C.c_float(float(cvar)), C.c_float(float(eps)), _p(actions), _capi.stream_ptr(self.device))
        if rc:
            raise _capi.MarineNavHipError(f"mn_iqn_actor_group_act failed ({rc}): the contexts must agree on the greedy-rows switch and have no late rows armed")
        return actions

    def append(self, obs, actions, reward, next_obs, done):
        """Every agent's rows of one vector step (device tensors as the stacked env returns them) into its own replay ring: `memory.add_vector_step` per agent."""
        first = self.agents[0].memory
        for i, ag in enumerate(self.agents[1:], 1):
            if ag.memory.ptr != first.ptr or ag.memory.capacity != first.capacity:
                raise ValueError(f"collector group: the ring of agent {i} is at row {ag.memory.ptr} of {ag.memory.capacity} and that of agent 0 at {first.ptr} of "
                                 f"{first.capacity}; a grouped append has one write position")
        for t in (obs, actions, reward, next_obs, done):
            assert t.is_cuda and t.is_contiguous() and t.shape[0] == len(self.agents) * self.n
        assert actions.dtype == torch.int32 and done.dtype == torch.uint8 and obs.dtype == torch.float32 and reward.dtype == torch.float32
        assert obs.data_ptr() != next_obs.data_ptr()
        rc = _capi.lib().mn_iqn_actor_group_append(self._handle, _p(obs), _p(actions), _p(reward), _p(next_obs), _p(done), int(first.ptr), int(first.capacity),
                                                   _capi.stream_ptr(self.device))
        if rc:
            raise _capi.MarineNavHipError(f"mn_iqn_actor_group_append failed ({rc})")
        for ag in self.agents:
            ag.memory.advance(self.n)
