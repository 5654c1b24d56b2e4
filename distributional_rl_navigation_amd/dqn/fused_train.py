"""Host side of the DQN baseline's fused HIP gradient step (csrc/dqn_train.hip): DQNAgent.train (sb3 DQN.train, dqn/dqn.py:188-230)
as ONE launch behind `mn_dqn_train_step` -- batch draw, target and local forward, smooth-L1 loss, backward, clip_grad_norm_ and Adam.

The kernel works on FLAT parameter vectors (27 650 floats, `q_net.named_parameters()` order).  `FusedTrainer` allocates one flat
buffer per network and re-points every `nn.Parameter` at a view of it, so the PyTorch modules (checkpoints, the target copy, the act
kernel, eager evaluation) and the HIP step always see the same memory; `p.grad` are views of the clipped gradient the step writes.
The Adam moments live in two more flat buffers that are ALSO `agent.optimizer`'s `exp_avg` / `exp_avg_sq` state (views), and the step
counter is copied between the device counter of the HIP step and the optimizer's per-parameter `step` whenever the agent switches
between the HIP and the PyTorch gradient step (`sync_to_optimizer` / `sync_from_optimizer`): one optimizer state, whichever path runs.
"""
import ctypes as C

import torch

from .. import _capi

P_TOTAL = 27650
MAX_BATCH = 256
MULTI_MAX_BATCH = 32      # mn_dqn_train_steps: both 16-sample tiles of a batch in one workgroup
MULTI_MAX_STEPS = 1024    # MN_DQN_MAX_STEPS (include/marinenav_hip.h); `FusedTrainer.steps` splits longer requests
_ORDER = tuple(f"features_extractor.{m}" for m in ("velocity_encoder", "goal_encoder", "sensor_encoder", "hidden_layer", "hidden_layer_2",
                                                   "output_layer")) + ("q_net.0", "q_net.2", "q_net.4")
PARAM_NAMES = tuple(f"{m}.{s}" for m in _ORDER for s in ("weight", "bias"))


def _p(t):
    return C.c_void_p(t.data_ptr())


def flatten_network(net):
    """One contiguous float32 buffer holding all parameters of `net` (a DQNPolicy.q_net); the parameters become views of it."""
    names = tuple(n for n, _ in net.named_parameters())
    assert names == PARAM_NAMES, names
    params = list(net.parameters())
    dev = params[0].device
    assert dev.type == "cuda", "the fused gradient step is a HIP kernel: parameters must live on the GPU"
    flat = torch.empty(sum(p.numel() for p in params), dtype=torch.float32, device=dev)
    assert flat.numel() == P_TOTAL
    off = 0
    with torch.no_grad():
        for p in params:
            n = p.numel()
            flat[off:off + n].copy_(p.detach().reshape(-1))
            p.data = flat[off:off + n].view(p.shape)
            off += n
    return flat


class FusedTrainer:
    def __init__(self, agent):
        self.agent = agent
        self.device = agent.device
        self.local = flatten_network(agent.q_net)
        self.target = flatten_network(agent.q_net_target)
        z = lambda: torch.zeros(P_TOTAL, dtype=torch.float32, device=self.device)
        self.grad, self.exp_avg, self.exp_avg_sq = z(), z(), z()
        self.step_dev = torch.zeros(1, dtype=torch.int32, device=self.device)
        self.loss = torch.zeros(1, dtype=torch.float32, device=self.device)
        self._ws = {}
        self._idx_out = {}
        self._multi = {}      # (batch, n_steps) -> (workspace, losses [n_steps], rows [n_steps][batch]) of the multi-step call
        # {seed, call counter} of the in-launch batch draw (mn_iqn_sample's permutation), seeded from the replay memory's generator
        self.rng_state = torch.tensor([int(agent.memory.gen.initial_seed()) & 0x7FFFFFFFFFFFFFFF, 0], dtype=torch.int64, device=self.device)
        self._nets = (agent.q_net, agent.q_net_target)
        self.point_grads()
        self._adopt_optimizer_state(agent.optimizer)

    def point_grads(self):
        """p.grad = views of the clipped gradient of the last fused step (the eager step's zero_grad drops them)."""
        off = 0
        for p in self.agent.q_net.parameters():
            p.grad = self.grad[off:off + p.numel()].view(p.shape)
            off += p.numel()

    # ---- one Adam state for both gradient-step paths ---------------------------------------------------------------
    def _adopt_optimizer_state(self, opt):
        """Make `opt.state[p]['exp_avg' / 'exp_avg_sq']` views of the flat moment buffers (keeping what the optimizer had
        accumulated so far) and take over its step count."""
        step, off = 0, 0
        for p in self.agent.q_net.parameters():
            n = p.numel()
            st = opt.state.get(p, None)
            m_view = self.exp_avg[off:off + n].view(p.shape)
            v_view = self.exp_avg_sq[off:off + n].view(p.shape)
            if st is not None and "exp_avg" in st:
                m_view.copy_(st["exp_avg"]); v_view.copy_(st["exp_avg_sq"])
                step = int(float(st["step"]))
            else:
                st = opt.state[p]
                on_dev = any(g.get("fused") or g.get("capturable") for g in opt.param_groups)
                st["step"] = torch.zeros((), dtype=torch.float32, device=p.device if on_dev else "cpu")
            st["exp_avg"], st["exp_avg_sq"] = m_view, v_view
            off += n
        self.step_dev.fill_(step)

    def sync_to_optimizer(self, opt):
        """HIP path -> PyTorch path: hand the step count to torch.optim.Adam (the moments are shared memory)."""
        t = float(int(self.step_dev.item()))
        for p in self.agent.q_net.parameters():
            opt.state[p]["step"].fill_(t)

    def sync_from_optimizer(self, opt):
        """PyTorch path -> HIP path."""
        p0 = next(iter(self.agent.q_net.parameters()))
        self.step_dev.fill_(int(float(opt.state[p0]["step"])))

    def owns(self, agent):
        return self._nets == (agent.q_net, agent.q_net_target)

    def _workspace(self, batch):
        ws = self._ws.get(batch)
        if ws is None:
            n = _capi.lib().mn_dqn_train_workspace_floats(batch)
            if n < 0:
                raise ValueError(f"fused DQN gradient step: batch {batch} outside 1..{MAX_BATCH}")
            ws = self._ws[batch] = torch.zeros(n, dtype=torch.float32, device=self.device)      # the ticket starts (and stays) at 0
        return ws

    def sync_target(self):
        """The hard target copy (tau = 1) as one copy of the flat buffer."""
        self.target.copy_(self.local)

    def step(self, ring, ring_size, batch, idx=None):
        """One optimizer step on the ring `(states, actions, rewards, next_states, dones)` (ReplayBuffer layout).  `idx` [batch] i64: the
        rows; None: the batch is drawn inside the launch from this trainer's generator state (uniform without replacement over the
        first `ring_size` rows; rows -> self.last_idx).  Returns the loss (a device view that the next step overwrites)."""
        ag = self.agent
        states, actions, rewards, next_states, dones = ring
        for t in ring:
            assert t.is_cuda and t.is_contiguous()
        assert states.dtype == torch.float32 and actions.dtype == torch.int64 and dones.dtype == torch.float32
        if idx is not None:
            idx = idx.to(self.device, torch.int64).contiguous()
            batch = idx.shape[0]
        out = self._idx_out.get(batch)
        if out is None:
            out = self._idx_out[batch] = torch.empty(batch, dtype=torch.int64, device=self.device)
        rc = _capi.lib().mn_dqn_train_step(
            _p(states), _p(next_states), _p(actions), _p(rewards), _p(dones), int(ring_size),
            None if idx is not None else _p(self.rng_state), _p(idx) if idx is not None else None, _p(out),
            _p(self.local), _p(self.target), _p(self._workspace(batch)), _p(self.grad), _p(self.loss), _p(self.exp_avg), _p(self.exp_avg_sq),
            _p(self.step_dev), batch, C.c_float(ag.gamma), C.c_double(ag.learning_rate), C.c_double(0.9), C.c_double(0.999), C.c_double(1e-8),
            C.c_double(ag.max_grad_norm), _capi.stream_ptr(self.device))
        if rc:
            raise _capi.MarineNavHipError(f"mn_dqn_train_step failed ({rc}): need batch in 1..{MAX_BATCH} and ring_size >= batch")
        self.last_idx = out
        ag.policy.weights_changed()      # the kernel wrote the weights outside PyTorch's version counters: the act image is stale
        return self.loss[0]

    def _multi_buffers(self, batch, n_steps):
        buf = self._multi.get((batch, n_steps))
        if buf is None:
            n = _capi.lib().mn_dqn_train_steps_workspace_floats(batch, n_steps)
            if n < 0:
                raise ValueError(f"multi-step DQN gradient call: batch {batch} outside 1..{MULTI_MAX_BATCH} or n_steps {n_steps} outside 1..{MULTI_MAX_STEPS}")
            buf = self._multi[(batch, n_steps)] = (torch.zeros(n, dtype=torch.float32, device=self.device),
                                                   torch.zeros(n_steps, dtype=torch.float32, device=self.device),
                                                   torch.empty((n_steps, batch), dtype=torch.int64, device=self.device))
        return buf

    def steps(self, ring, ring_size, batch, n_steps, idx=None, parts=3):
        """`n_steps` consecutive optimizer steps as ONE call of `mn_dqn_train_steps` (batch <= 32; two launches, no launch per step): bit for bit what
        `n_steps` calls of `step` leave.  `idx` [n_steps][batch] i64: the rows of every step; None: drawn as `step` draws them.  The target network must
        not change among the steps: cut a run at its target copies (`split_at_target_sync`).  Requests above MN_DQN_MAX_STEPS are split.  Returns the
        [n_steps] losses (a device view that the next call of the same shape overwrites) and sets `last_idx` [n_steps][batch].
        `parts` (measurements): 1 the TD-target launch only, 2 the chain only, 3 both."""
        ag = self.agent
        states, actions, rewards, next_states, dones = ring
        for t in ring:
            assert t.is_cuda and t.is_contiguous()
        assert states.dtype == torch.float32 and actions.dtype == torch.int64 and dones.dtype == torch.float32
        if idx is not None:
            idx = idx.to(self.device, torch.int64).contiguous()
            n_steps, batch = idx.shape
        if n_steps > MULTI_MAX_STEPS:
            losses, rows = [], []
            for k0 in range(0, n_steps, MULTI_MAX_STEPS):
                k1 = min(n_steps, k0 + MULTI_MAX_STEPS)
                losses.append(self.steps(ring, ring_size, batch, k1 - k0, None if idx is None else idx[k0:k1], parts).clone())
                rows.append(self.last_idx.clone())
            self.last_idx = torch.cat(rows)
            return torch.cat(losses)
        ws, losses, out = self._multi_buffers(batch, n_steps)
        rc = _capi.lib().mn_dqn_train_steps_parts(
            _p(states), _p(next_states), _p(actions), _p(rewards), _p(dones), int(ring_size),
            None if idx is not None else _p(self.rng_state), _p(idx) if idx is not None else None, _p(out),
            _p(self.local), _p(self.target), _p(ws), _p(self.grad), _p(losses), _p(self.exp_avg), _p(self.exp_avg_sq),
            _p(self.step_dev), batch, n_steps, C.c_float(ag.gamma), C.c_double(ag.learning_rate), C.c_double(0.9), C.c_double(0.999), C.c_double(1e-8),
            C.c_double(ag.max_grad_norm), parts, _capi.stream_ptr(self.device))
        if rc:
            raise _capi.MarineNavHipError(f"mn_dqn_train_steps failed ({rc}): need batch in 1..{MULTI_MAX_BATCH}, n_steps >= 1 and ring_size >= batch")
        self.last_idx = out
        ag.policy.weights_changed()      # once per call: the act image is rebuilt on the next act, not per step
        return losses
