"""Many DQN learners per launch: the host side of `mn_dqn_group_train_step` / `mn_dqn_group_train_steps` (csrc/dqn_train.hip).

`LearnerGroup(agents)` steps every agent's fused learner -- the seeds of one config -- in ONE launch per gradient step, or one multi-step call per stretch,
instead of one per agent.  It takes each agent's own `FusedTrainer` buffers (dqn/fused_train.py), so an agent can be stepped by the group and by itself in
any interleaving, and every learner is bit for bit what `agent.train()` / `agent.train_many()` leave: the grouped kernels inline the single kernels' bodies
with the learner as a grid dimension.  What a launch has in common -- batch size, the ring's fill, gamma, the learning rate, the clip norm -- must be equal
among the agents; everything else (ring contents, networks, Adam state, step and draw counters) is each agent's own.
"""
import ctypes as C

import torch

from .. import _capi
from .fused_train import MAX_BATCH, MULTI_MAX_BATCH, MULTI_MAX_STEPS, _p

MAX_LEARNERS = _capi.DQN_MAX_LEARNERS


def check_agents(agents):
    """ValueError, in words that name the difference, unless `agents` can share a launch.  Reads attributes only: nothing touches a device."""
    agents = list(agents)
    if not 1 <= len(agents) <= MAX_LEARNERS:
        raise ValueError(f"a learner group holds 1..{MAX_LEARNERS} agents, not {len(agents)}")
    if len({id(a) for a in agents}) != len(agents):
        raise ValueError("a learner group cannot hold the same agent twice: its two learners would write the same buffers")
    first = agents[0]
    common = (("batch size", lambda a: a.batch_size), ("ring capacity", lambda a: a.memory.capacity), ("ring fill", lambda a: a.memory.size),
              ("gamma", lambda a: a.gamma), ("learning rate", lambda a: a.learning_rate), ("max_grad_norm", lambda a: a.max_grad_norm))
    for what, get in common:
        for i, a in enumerate(agents[1:], 1):
            if get(a) != get(first):
                raise ValueError(f"learner group: agent {i} differs from agent 0 in {what} ({get(a)!r} against {get(first)!r}); a grouped launch has one {what}")
    for i, a in enumerate(agents):
        dev = torch.device(a.device)
        if dev.type != "cuda":
            raise ValueError(f"learner group: agent {i} is on {dev}; the agents must be on one GPU")
        if dev != torch.device(first.device):
            raise ValueError(f"learner group: agent {i} is on {dev} and agent 0 on {torch.device(first.device)}; the agents must be on one GPU")
    for i, a in enumerate(agents):
        if not a._uses_fused():
            raise ValueError(f"learner group: agent {i} does not use the fused path (fused_train=True and batch size <= {MAX_BATCH}): there is no grouped "
                             "form of the eager gradient step")
    return agents


class LearnerGroup:
    def __init__(self, agents):
        self.agents = check_agents(agents)
        self.device = torch.device(self.agents[0].device)
        self.batch = int(self.agents[0].batch_size)
        self.trainers = [a._fused_trainer() for a in self.agents]
        table = (_capi.MnDqnLearner * len(self.agents))()
        for row, ag, ft in zip(table, self.agents, self.trainers):
            m = ag.memory
            for t in (m.states, m.actions, m.rewards, m.next_states, m.dones):
                assert t.is_cuda and t.is_contiguous()
            assert m.states.dtype == torch.float32 and m.actions.dtype == torch.int64 and m.dones.dtype == torch.float32
            row.ring_states, row.ring_next_states, row.ring_actions = m.states.data_ptr(), m.next_states.data_ptr(), m.actions.data_ptr()
            row.ring_rewards, row.ring_dones, row.rng_state = m.rewards.data_ptr(), m.dones.data_ptr(), ft.rng_state.data_ptr()
            row.params_local, row.params_target, row.grad = ft.local.data_ptr(), ft.target.data_ptr(), ft.grad.data_ptr()
            row.exp_avg, row.exp_avg_sq, row.step = ft.exp_avg.data_ptr(), ft.exp_avg_sq.data_ptr(), ft.step_dev.data_ptr()
        self._handle = C.c_void_p()
        rc = _capi.lib().mn_dqn_group_create(table, len(self.agents), C.byref(self._handle))
        if rc:
            self._handle = None
            raise _capi.MarineNavHipError(f"mn_dqn_group_create failed ({rc}): the learners' buffers must not overlap")
        self._bufs = {}      # n_steps (0: the single step) -> (workspace [G][stride], losses [G][n_steps], rows [G][n_steps][batch])

    def __len__(self):
        return len(self.agents)

    def close(self):
        if getattr(self, "_handle", None):
            _capi.lib().mn_dqn_group_destroy(self._handle)
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
        for ag, ft in zip(self.agents, self.trainers):
            if not ft.owns(ag) or ag._fused is not ft:
                raise ValueError("learner group: an agent's networks were replaced since the group was built; build a new group")
        return sizes.pop()

    def _buffers(self, n_steps):
        buf = self._bufs.get(n_steps)
        if buf is None:
            L, G = _capi.lib(), len(self.agents)
            n = L.mn_dqn_train_steps_workspace_floats(self.batch, n_steps) if n_steps else L.mn_dqn_train_workspace_floats(self.batch)
            if n < 0:
                raise ValueError(f"grouped DQN gradient call: batch {self.batch} or n_steps {n_steps} outside the single calls' limits")
            stride = (n + 3) // 4 * 4
            k = max(n_steps, 1)
            buf = self._bufs[n_steps] = (torch.zeros(G * stride, dtype=torch.float32, device=self.device),      # (the tickets start, and stay, at 0)
                                         torch.zeros((G, k), dtype=torch.float32, device=self.device),
                                         torch.empty((G, k, self.batch), dtype=torch.int64, device=self.device))
        return buf

    def _entered(self):
        for ag in self.agents:
            ag._enter_train_path("hip")

    def _left(self, n_steps):
        for ag in self.agents:
            ag.n_updates += n_steps
            ag.policy.weights_changed()      # the kernel wrote the weights outside PyTorch's version counters: the act image is stale

    def _hyper(self):
        ag = self.agents[0]
        return (C.c_float(ag.gamma), C.c_double(ag.learning_rate), C.c_double(0.9), C.c_double(0.999), C.c_double(1e-8), C.c_double(ag.max_grad_norm))

    # ---- the calls -------------------------------------------------------------------------------------------------------------------------------------
    def train(self, idx=None):
        """One gradient step of every agent as ONE launch: each on a batch drawn from its own ring with its own draw state, or on rows `idx` [G][batch].
        Returns the losses [G] (a copy); the rows are in `last_idx` [G][batch]."""
        ring_size = self._ring_size()
        ws, losses, rows = self._buffers(0)
        if idx is not None:
            idx = idx.to(self.device, torch.int64).contiguous()
            assert idx.shape == (len(self.agents), self.batch), idx.shape
        self._entered()
        rc = _capi.lib().mn_dqn_group_train_step(self._handle, ring_size, _p(idx) if idx is not None else None, _p(rows), _p(ws), _p(losses), self.batch,
                                                 *self._hyper(), _capi.stream_ptr(self.device))
        if rc:
            raise _capi.MarineNavHipError(f"mn_dqn_group_train_step failed ({rc}): need batch in 1..{MAX_BATCH} and ring_size >= batch")
        self._left(1)
        self.last_idx = rows[:, 0]
        return losses[:, 0].clone()

    def train_many(self, n_steps, idx=None):
        """`n_steps` gradient steps of every agent: at batch <= 32 ONE grouped multi-step call (two launches; requests above MN_DQN_MAX_STEPS are split as
        `FusedTrainer.steps` splits them), otherwise the loop of grouped steps.  `idx` [G][n_steps][batch]: the rows; None: drawn.  The target networks must
        not change among the steps (`split_at_target_sync`).  Returns the losses [G][n_steps]; the rows are in `last_idx` [G][n_steps][batch]."""
        G = len(self.agents)
        if n_steps <= 0:
            return torch.zeros((G, 0), device=self.device)
        if idx is not None:
            idx = idx.to(self.device, torch.int64).contiguous()
            assert idx.shape == (G, n_steps, self.batch), idx.shape
        if self.batch > MULTI_MAX_BATCH:
            losses, rows = [], []
            for k in range(n_steps):
                losses.append(self.train(None if idx is None else idx[:, k]))
                rows.append(self.last_idx.clone())
            self.last_idx = torch.stack(rows, dim=1)
            return torch.stack(losses, dim=1)
        if n_steps > MULTI_MAX_STEPS:
            losses, rows = [], []
            for k0 in range(0, n_steps, MULTI_MAX_STEPS):
                k1 = min(n_steps, k0 + MULTI_MAX_STEPS)
                losses.append(self.train_many(k1 - k0, None if idx is None else idx[:, k0:k1]))
                rows.append(self.last_idx.clone())
            self.last_idx = torch.cat(rows, dim=1)
            return torch.cat(losses, dim=1)
        ring_size = self._ring_size()
        ws, losses, rows = self._buffers(n_steps)
        self._entered()
        rc = _capi.lib().mn_dqn_group_train_steps(self._handle, ring_size, _p(idx) if idx is not None else None, _p(rows), _p(ws), _p(losses), self.batch,
                                                  n_steps, *self._hyper(), _capi.stream_ptr(self.device))
        if rc:
            raise _capi.MarineNavHipError(f"mn_dqn_group_train_steps failed ({rc}): need batch in 1..{MULTI_MAX_BATCH}, n_steps >= 1 and ring_size >= batch")
        self._left(n_steps)
        self.last_idx = rows
        return losses.clone()

    def sync_target(self):
        """Every learner's hard target copy."""
        for ag in self.agents:
            ag.sync_target()
