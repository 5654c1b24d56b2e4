"""Many DQN actors per launch: the host side of `mn_dqn_actor_group_*` (csrc/dqn_collect.hip, csrc/replay.hip).

`CollectorGroup(agents, stacked_env)` is the collect phase of G agents in lockstep -- the seeds of one config -- whose envs are STACKED in one
`VecMarineNavEnv` of G n rows, agent g owning rows [g n, (g + 1) n): per vector step one `act` (at most two launches: the weight images that are stale,
then the exploring act with the agent as the second grid dimension) and one `append` (every agent's transitions into its own replay ring) instead of G of
each; the env step and the episode resets are the stacked env's own single launches.  Every agent's actions, call counter, weight image and ring are bit
for bit what `agent.act_batch` and `memory.add_vector_step` leave for that agent alone (`DQNAgent(fused_collect=True)`), and since the library keeps no
state of its own, grouped and single calls (an inline evaluation's `policy.act_batch`) interleave freely.  What a launch has in common must be equal among
the agents: the rows per agent, the exploration rate of the call, the ring's capacity and write position.
"""
import ctypes as C

import torch

from .. import _capi

MAX_ACTORS = _capi.DQN_MAX_ACTORS


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
        if not (a.fused_collect and a.policy.use_fused_act):
            raise ValueError(f"collector group: agent {i} does not collect on the device with the library's generator (fused_collect, policy.use_fused_act): "
                             "the grouped act launch has no other form")
    common = (("ring capacity", lambda a: a.memory.capacity), ("ring write position (ptr)", lambda a: a.memory.ptr))
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
        self.env = stacked_env
        self.device = torch.device(self.agents[0].device)
        G = len(self.agents)
        self.n = n = int(stacked_env.n_envs) // G
        self._handle = None
        self._states, self._ptrs = [], []
        self._calls = (C.c_uint64 * G)()
        table = (_capi.MnDqnActor * G)()
        for row, ag in zip(table, self.agents):
            m = ag.memory
            st, _ = ag.policy._image(self.device)      # (brings the pointer table up to date; whether the image is stale is asked again at every act)
            st["sig"] = None
            for t in (m.states, m.actions, m.rewards, m.next_states, m.dones):
                assert t.is_cuda and t.is_contiguous()
            assert m.states.dtype == torch.float32 and m.actions.dtype == torch.int64 and m.dones.dtype == torch.float32
            self._states.append(st)
            self._ptrs.append(tuple(st["ptrs"]))
            row.weights, row.image, row.seed = C.cast(st["ptrs"], C.c_void_p).value, st["image"].data_ptr(), int(ag.act_seed) & ((1 << 64) - 1)
            row.ring_states, row.ring_next_states, row.ring_actions = m.states.data_ptr(), m.next_states.data_ptr(), m.actions.data_ptr()
            row.ring_rewards, row.ring_dones = m.rewards.data_ptr(), m.dones.data_ptr()
        h = C.c_void_p()
        with torch.cuda.device(self.device):
            rc = _capi.lib().mn_dqn_actor_group_create(table, G, n, C.byref(h))
        if rc:
            raise _capi.MarineNavHipError(f"mn_dqn_actor_group_create failed ({rc}): the actors' weight images and rings must be their own")
        self._handle = h

    def __len__(self):
        return len(self.agents)

    def close(self):
        if getattr(self, "_handle", None):
            _capi.lib().mn_dqn_actor_group_destroy(self._handle)
            self._handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_grid(self, workgroups_per_group):
        """Workgroups per agent of the act launch instead of the default share of the CUs (0: the default again); results do not depend on it."""
        rc = _capi.lib().mn_dqn_actor_group_set_grid(self._handle, int(workgroups_per_group))
        if rc:
            raise _capi.MarineNavHipError(f"mn_dqn_actor_group_set_grid failed ({rc})")

    @torch.no_grad()
    def act(self, obs, eps):
        """`agent.act_batch(obs[g n : (g + 1) n], eps)` of every agent g: actions [G n] int32 (device); every agent's `act_calls` advances."""
        assert obs.is_cuda and obs.dtype == torch.float32 and obs.is_contiguous() and obs.shape[0] == len(self.agents) * self.n
        stale = 0
        for i, (ag, st0, ptrs) in enumerate(zip(self.agents, self._states, self._ptrs)):
            st, repack = ag.policy._image(self.device)
            if st is not st0 or tuple(st["ptrs"]) != ptrs:
                raise ValueError(f"collector group: the network of agent {i} was replaced or re-allocated since the group was built; build a new group")
            stale |= int(repack) << i
            self._calls[i] = int(ag.act_calls) & ((1 << 64) - 1)
        actions = torch.empty(obs.shape[0], dtype=torch.int32, device=obs.device)
        with torch.cuda.device(self.device):
            rc = _capi.lib().mn_dqn_actor_group_act(self._handle, _p(obs), C.c_float(float(eps)), stale, self._calls, _p(actions), _capi.stream_ptr(self.device))
        if rc:
            for st in self._states:      # (nothing was launched: every image is as stale as it was)
                st["sig"] = None
            raise _capi.MarineNavHipError(f"mn_dqn_actor_group_act failed ({rc})")
        for ag in self.agents:
            ag.act_calls += 1
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
        rc = _capi.lib().mn_dqn_actor_group_append(self._handle, _p(obs), _p(actions), _p(reward), _p(next_obs), _p(done), int(first.ptr), int(first.capacity),
                                                   _capi.stream_ptr(self.device))
        if rc:
            raise _capi.MarineNavHipError(f"mn_dqn_actor_group_append failed ({rc})")
        for ag in self.agents:
            ag.memory.advance(self.n)
