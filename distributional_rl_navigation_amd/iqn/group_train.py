"""Many IQN learners per launch: the host side of `mn_iqn_group_train_step` (csrc/iqn_train.hip, "many learners per launch").

`LearnerGroup(agents)` steps every agent's fused learner -- the seeds of one config -- in THREE launches per gradient step (forward / backward, reduction,
clip + Adam, the learner being a grid dimension of each) instead of one to three per agent.  The grouped kernels are the forms of the single step in which
no workgroup waits for another, so a group may be larger than the device; they inline the single kernels' bodies, and every learner is bit for bit what
`agent.train_from_memory()` / `agent.train()` leave.  The group takes each agent's own `FusedTrainer` buffers (iqn/fused_train.py) and that trainer's
workspace of the batch size -- epoch word, generator state and Adam counter live in the agent's own memory -- so an agent can be stepped by the group and
by itself in any interleaving.  What a launch has in common -- batch size, the ring's fill, gamma ** n_step, the learning rate, the number of taus -- must
be equal among the agents.  `use_fused_graph`, `one_launch_step`, `two_launch_step` and `mn_iqn_train_set_mode` select among the single forms only: the
grouped form is always the one above.
"""
import ctypes as C

import torch

from .. import _capi

MAX_LEARNERS = _capi.IQN_MAX_LEARNERS


def _p(t):
    return C.c_void_p(t.data_ptr())


def check_agents(agents):
    """ValueError, in words that name the difference, unless `agents` can share a launch.  Reads attributes only: nothing touches a device."""
    agents = list(agents)
    if not 1 <= len(agents) <= MAX_LEARNERS:
        raise ValueError(f"a learner group holds 1..{MAX_LEARNERS} agents, not {len(agents)}")
    if len({id(a) for a in agents}) != len(agents):
        raise ValueError("a learner group cannot hold the same agent twice: its two learners would write the same buffers")
    first = agents[0]
    common = (("batch size", lambda a: a.BATCH_SIZE), ("ring capacity", lambda a: a.memory.capacity), ("ring fill", lambda a: a.memory.size),
              ("gamma", lambda a: a.GAMMA ** a.n_step), ("learning rate", lambda a: a.LR), ("number of taus", lambda a: a.N))
    for what, get in common:
        for i, a in enumerate(agents[1:], 1):
            if get(a) != get(first):
                raise ValueError(f"learner group: agent {i} differs from agent 0 in {what} ({get(a)!r} against {get(first)!r}); a grouped launch has one {what}")
    for i, a in enumerate(agents):
        dev = torch.device(a.device)
        if dev.type != "cuda":
            raise ValueError(f"learner group: agent {i} is on device {dev}; the agents must be on one GPU")
        if dev != torch.device(first.device):
            raise ValueError(f"learner group: agent {i} is on device {dev} and agent 0 on {torch.device(first.device)}; the agents must be on one GPU")
    for i, a in enumerate(agents):
        if not a.use_fused_train:
            raise ValueError(f"learner group: agent {i} does not use the fused gradient step (use_fused_train): there is no grouped form of the PyTorch step")
        if a.distributed:
            raise ValueError(f"learner group: agent {i} is a distributed (shared) learner: its gradient exchange has no grouped form")
        if getattr(a, "per", False):
            raise ValueError(f"learner group: agent {i} uses prioritized replay (per=True): the grouped launches draw uniformly inside the launch and have no "
                             "prioritized form")
        if getattr(a, "munchausen", False):
            raise ValueError(f"learner group: agent {i} uses the Munchausen target (munchausen=True): the grouped launches run one target forward per "
                             "element and have no Munchausen form")
        if getattr(a, "target_rule", "max") != "max":
            raise ValueError(f"learner group: agent {i} uses target_rule={a.target_rule!r}: the grouped launches take the per-sample max and have no "
                             "greedy-on-mean form")
    if first.BATCH_SIZE % 2 or not 2 <= first.BATCH_SIZE <= 1024:
        raise ValueError(f"learner group: batch size {first.BATCH_SIZE}; the fused gradient step takes even batch sizes up to 1024")
    return agents


class LearnerGroup:
    def __init__(self, agents):
        self.agents = check_agents(agents)
        self.device = torch.device(self.agents[0].device)
        self.batch = int(self.agents[0].BATCH_SIZE)
        self.trainers = [a._fused_trainer() for a in self.agents]
        G, B, N = len(self.agents), self.batch, int(self.agents[0].N)
        self._workspaces = []
        table = (_capi.MnIqnLearner * G)()
        for row, ag, ft in zip(table, self.agents, self.trainers):
            m = ag.memory
            for t in (m.states, m.actions, m.rewards, m.next_states, m.dones):
                assert t.is_cuda and t.is_contiguous()
            assert m.states.dtype == torch.float32 and m.actions.dtype == torch.int64 and m.dones.dtype == torch.float32
            if B not in ft._idx:      # (as FusedTrainer.step_sampled makes them)
                ft._idx[B] = torch.empty(B, dtype=torch.int64, device=self.device)
                ft._taus[B] = torch.empty(2, B, N, dtype=torch.float32, device=self.device)
            ws = ft._workspace(B)
            self._workspaces.append(ws)
            row.ring_states, row.ring_next_states, row.ring_actions = m.states.data_ptr(), m.next_states.data_ptr(), m.actions.data_ptr()
            row.ring_rewards, row.ring_dones, row.rng_state = m.rewards.data_ptr(), m.dones.data_ptr(), ft.rng_state.data_ptr()
            row.params_local, row.params_target, row.workspace = ft.local.data_ptr(), ft.target.data_ptr(), ws.data_ptr()
            row.grad, row.loss, row.exp_avg, row.exp_avg_sq = ft.grad.data_ptr(), ft.loss.data_ptr(), ft.exp_avg.data_ptr(), ft.exp_avg_sq.data_ptr()
            row.step, row.idx_out, row.taus_out = ft.step_dev.data_ptr(), ft._idx[B].data_ptr(), ft._taus[B].data_ptr()
        self._handle = C.c_void_p()
        rc = _capi.lib().mn_iqn_group_create(table, G, B, C.byref(self._handle))
        if rc:
            self._handle = None
            raise _capi.MarineNavHipError(f"mn_iqn_group_create failed ({rc}): the learners' buffers must not overlap")
        self._losses = torch.zeros(G, dtype=torch.float32, device=self.device)

    def __len__(self):
        return len(self.agents)

    def close(self):
        if getattr(self, "_handle", None):
            _capi.lib().mn_iqn_group_destroy(self._handle)
            self._handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- what the launch has in common, read from the agents at every call -----------------------------------------------------------------------------
    def _ring_size(self):
        sizes = {int(a.memory.size) for a in self.agents}
        if len(sizes) != 1:
            raise ValueError(f"learner group: the agents' rings are not equally full ({sorted(sizes)} rows); a grouped launch has one ring fill")
        for ag, ft, ws in zip(self.agents, self.trainers, self._workspaces):
            if not ft.owns(ag) or ag._fused is not ft:
                raise ValueError("learner group: an agent's networks were replaced since the group was built; build a new group")
            if ft._workspace(self.batch) is not ws:
                raise ValueError("learner group: an agent's workspace was replaced since the group was built; build a new group")
        return sizes.pop()

    def _entered(self):
        for ag in self.agents:
            ag._enter_train_path("hip")

    def _left(self, n_steps):
        from .fused_act import weights_changed
        for ag, ft in zip(self.agents, self.trainers):
            ag.grad_steps += n_steps
            ft._staged_key = None      # the grouped reduction stages nothing and says so in the workspace
            weights_changed(ag.qnetwork_local)      # the kernel wrote the weights outside PyTorch's version counters: the act image is stale

    def _call(self, ring_size, idx, tt, tl):
        ag = self.agents[0]
        q = lambda t: _p(t) if t is not None else None
        rc = _capi.lib().mn_iqn_group_train_step(self._handle, int(ring_size), q(idx), q(tt), q(tl), C.c_float(ag.GAMMA ** ag.n_step), C.c_double(ag.LR),
                                                 C.c_double(0.9), C.c_double(0.999), C.c_double(1e-8), C.c_double(0.5), _capi.stream_ptr(self.device))
        if rc:
            raise _capi.MarineNavHipError(f"mn_iqn_group_train_step failed ({rc}): need ring_size >= batch, and idx / taus_target / taus_local all given or all None")

    def _gather_losses(self):
        torch.stack([ft.loss[0] for ft in self.trainers], out=self._losses)
        return self._losses.clone()

    # ---- the calls -------------------------------------------------------------------------------------------------------------------------------------
    def train(self, idx=None, taus_target=None, taus_local=None):
        """One gradient step of every agent in three launches: each on a batch drawn from its own ring with its own generator state, or -- all three
        given -- on rows `idx` [G][batch] with taus `taus_target` / `taus_local` [G][batch][N].  Returns the losses [G] (a copy); every agent's own
        loss word, `last` rows and taus are where its single step leaves them."""
        given = [x is not None for x in (idx, taus_target, taus_local)]
        if any(given) and not all(given):
            raise ValueError("learner group: idx, taus_target and taus_local are given together or not at all")
        G, B, N = len(self.agents), self.batch, int(self.agents[0].N)
        ring_size = self._ring_size()
        if all(given):
            idx = idx.to(self.device, torch.int64).contiguous()
            taus_target = taus_target.to(self.device, torch.float32).contiguous()
            taus_local = taus_local.to(self.device, torch.float32).contiguous()
            assert idx.shape == (G, B) and taus_target.numel() == G * B * N and taus_local.numel() == G * B * N, (idx.shape, taus_target.shape, taus_local.shape)
        self._entered()
        self._call(ring_size, idx, taus_target, taus_local)
        self._left(1)
        return self._gather_losses()

    def train_many(self, n_steps):
        """`n_steps` drawn gradient steps of every agent: the loop of grouped steps (3 * n_steps launches).  The target networks must not change among
        the steps.  Returns the losses [G] of the last step (None for n_steps <= 0)."""
        if n_steps <= 0:
            return None
        ring_size = self._ring_size()
        self._entered()
        for _ in range(n_steps):
            self._call(ring_size, None, None, None)
        self._left(n_steps)
        return self._gather_losses()

    def sync_target(self):
        """Every learner's hard target copy, with the mark its own cadence counts from."""
        for ag in self.agents:
            ag._sync_target()
