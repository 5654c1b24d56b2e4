"""Inference-side counterpart of the reference's DQN baseline (run_experiments.py:74-98, 367-376).

The reference's DQN agent is its modified stable-baselines3 `ObsEncoderPolicy`: the features extractor is the
whole 26 -> (16 | 16 | 176) -> 64 -> 64 -> 9 observation network WITHOUT activations on the three encoders
(thirdparty/stable_baselines3/common/torch_layers.py:96-135), followed by sb3's default 9 -> 64 -> 64 -> 9 Q head
(dqn/policies.py:48-58, torch_layers.py:137-174).  Only the greedy policy is needed on the batched path (the
experiment sweep and evaluation); training is `dqn.agent.DQNAgent` (eager, or the fused HIP step of csrc/dqn_train.hip).

Module / parameter names mirror sb3's (`q_net.features_extractor.*`, `q_net.q_net.{0,2,4}.*`) so that the
`policy.pth` inside an sb3 checkpoint zip loads unchanged.
"""
import io
import zipfile

import numpy as np
import torch
import torch.nn as nn


def image_floats():
    """Floats of one weight image (C-ABI mn_dqn_image_floats): the row length of `rollout_dqn_groups`' `images`."""
    from .. import _capi
    return int(_capi.lib().mn_dqn_image_floats())


@torch.no_grad()
def rollout_dqn_groups(images, env, n_steps, rows_per_group, trace=("reward", "done", "info", "action")):
    """`DQNPolicy.rollout` for MANY networks in ONE launch (C-ABI mn_rollout_dqn_groups): rows [g * rows_per_group, (g + 1) * rows_per_group) of `env`
    act with `images[g]` (a [G][>= image_floats()] float32 tensor of `DQNPolicy.export_image` rows).  Group g gets, bit for bit, what
    `policy_g.rollout(env_g, n_steps)` gets on an env of its own with the group's worlds.  Returns the requested traces ([n_steps][n] ...; "obs"
    [n_steps][n][26], "q" [n_steps][n][9]; no "traj") and `final_obs`.  Nothing here synchronises with the host; the longest episode of a group is
    `episodes.steps_run` of its columns of the done trace."""
    import ctypes as C
    from .. import _capi
    from ..episodes import trace_buffers
    T, n, dev, R = int(n_steps), env.n_envs, env.device, int(rows_per_group)
    assert images.is_cuda and images.dim() == 2 and images.dtype == torch.float32 and images.stride(1) == 1
    assert "traj" not in trace, "the grouped launch records no trajectory trace"
    G = images.shape[0]
    tr = trace_buffers(T, n, dev, trace)
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    rc = _capi.lib().mn_rollout_dqn_groups(env.h, p(images), images.stride(0), G, R, T, p(env.obs), p(tr.get("obs")), p(tr.get("reward")), p(tr.get("done")),
                                           p(tr.get("info")), p(tr.get("action")), p(tr.get("q")), env._stream())
    if rc:
        raise _capi.MarineNavHipError(f"mn_rollout_dqn_groups failed ({rc}): {_capi.lib().mn_last_error(env.h).decode()}")
    out = dict(tr)
    out["final_obs"] = env.obs
    return out


class _Extractor(nn.Module):
    def __init__(self, state_size=26, action_size=9):
        super().__init__()
        assert state_size == 26, "observation dimension needs to be 26 (velocity, goal, measurements)"
        self.velocity_encoder = nn.Linear(2, 16)
        self.goal_encoder = nn.Linear(2, 16)
        self.sensor_encoder = nn.Linear(22, 176)
        self.hidden_layer = nn.Linear(208, 64)
        self.hidden_layer_2 = nn.Linear(64, 64)
        self.output_layer = nn.Linear(64, action_size)

    def forward(self, x):
        f = torch.cat((self.velocity_encoder(x[:, :2]), self.goal_encoder(x[:, 2:4]), self.sensor_encoder(x[:, 4:])), 1)
        return self.output_layer(torch.relu(self.hidden_layer_2(torch.relu(self.hidden_layer(f)))))


class _QNet(nn.Module):
    def __init__(self, state_size, action_size, net_arch):
        super().__init__()
        self.features_extractor = _Extractor(state_size, action_size)
        layers, d = [], action_size
        for h in net_arch:
            layers += [nn.Linear(d, h), nn.ReLU()]
            d = h
        layers.append(nn.Linear(d, action_size))
        self.q_net = nn.Sequential(*layers)

    def forward(self, x):
        return self.q_net(self.features_extractor(x))


class DQNPolicy(nn.Module):
    """Greedy DQN policy over device-resident observation batches."""

    def __init__(self, state_size=26, action_size=9, net_arch=(64, 64), device="cuda:0"):
        super().__init__()
        self.state_size, self.action_size = state_size, action_size
        self.q_net = _QNet(state_size, action_size, list(net_arch))
        self.device = torch.device(device)
        self.to(self.device)
        self.eval()

    @classmethod
    def load(cls, path, device="cuda:0"):
        """`path`: an sb3 checkpoint .zip (its policy.pth is read), a bare policy.pth, or an .npz of the q_net.*
        tensors (tests/golden/pretrained_DQN_seed3/q_net.npz)."""
        if path.endswith(".npz"):
            sd = {k: torch.from_numpy(v) for k, v in np.load(path).items()}
        elif zipfile.is_zipfile(path) and "policy.pth" in zipfile.ZipFile(path).namelist():
            with zipfile.ZipFile(path) as z:
                sd = torch.load(io.BytesIO(z.read("policy.pth")), map_location="cpu")
        else:
            sd = torch.load(path, map_location="cpu")
        sd = {k: v for k, v in sd.items() if k.startswith("q_net.")}      # q_net_target.* is training state
        pol = cls(device=device)
        pol.load_state_dict(sd, strict=True)
        return pol

    use_fused_act = True      # GPU tensors: the whole network + argmax as ONE HIP launch (csrc/dqn_act.hip); False = eager PyTorch

    def _image(self, device):
        """The permuted weight image of the HIP kernels on `device` and whether it must be rebuilt in front of the next launch: when a parameter
        was written (PyTorch version counters), re-allocated, or `weights_changed()` was called.  Returns (state dict, repack)."""
        import ctypes as C
        from .. import _capi
        L = _capi.lib()
        ex, qn = self.q_net.features_extractor, self.q_net.q_net
        mods = (ex.velocity_encoder, ex.goal_encoder, ex.sensor_encoder, ex.hidden_layer, ex.hidden_layer_2, ex.output_layer, qn[0], qn[2], qn[4])
        ps = [t for m in mods for t in (m.weight, m.bias)]
        sig = tuple((t.data_ptr(), t._version) for t in ps)
        st = getattr(self, "_fused_state", None)
        if st is None or st["image"].device != device:
            st = dict(image=torch.empty(L.mn_dqn_image_floats(), dtype=torch.float32, device=device), sig=None, ptrs=(C.c_void_p * 18)())
            object.__setattr__(self, "_fused_state", st)
        repack = sig != st["sig"]
        if repack:
            for i, t in enumerate(ps):
                assert t.is_cuda and t.is_contiguous() and t.dtype == torch.float32
                st["ptrs"][i] = t.data_ptr()
            st["sig"] = sig
        return st, repack

    def _fused(self, obs, want_q, want_a):
        """C-ABI mn_dqn_act on a contiguous float32 device batch; the permuted weight image is rebuilt when a parameter was written
        (PyTorch version counters) or re-allocated."""
        import ctypes as C
        from .. import _capi
        L = _capi.lib()
        st, repack = self._image(obs.device)
        n = obs.shape[0]
        q = torch.empty(n, self.action_size, dtype=torch.float32, device=obs.device) if want_q else None
        a = torch.empty(n, dtype=torch.int32, device=obs.device) if want_a else None
        p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
        rc = L.mn_dqn_act(p(obs), st["ptrs"], p(st["image"]), int(repack), p(q), p(a), n, C.c_void_p(torch.cuda.current_stream(obs.device).cuda_stream))
        if rc:
            raise _capi.MarineNavHipError(f"mn_dqn_act failed ({rc})")
        return q, a

    @torch.no_grad()
    def act_rng(self, obs, seed, call_index, eps, want_u=False, want_q=False):
        """Epsilon-greedy actions of a contiguous float32 device batch in ONE launch (C-ABI mn_dqn_act_rng): row e explores iff its uniform
        u01(e, draw_keys(seed, call_index)) is <= eps.  Returns the int32 actions, or (actions, uniforms or None, Q-values or None) with `want_u` / `want_q`."""
        import ctypes as C
        from .. import _capi
        st, repack = self._image(obs.device)
        n = obs.shape[0]
        a = torch.empty(n, dtype=torch.int32, device=obs.device)
        u = torch.empty(n, dtype=torch.float32, device=obs.device) if want_u else None
        q = torch.empty(n, self.action_size, dtype=torch.float32, device=obs.device) if want_q else None
        p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
        mask = (1 << 64) - 1
        rc = _capi.lib().mn_dqn_act_rng(p(obs), st["ptrs"], p(st["image"]), int(repack), int(seed) & mask, int(call_index) & mask, C.c_float(float(eps)),
                                        p(u), p(q), p(a), n, _capi.stream_ptr(obs.device))
        if rc:
            raise _capi.MarineNavHipError(f"mn_dqn_act_rng failed ({rc})")
        return (a, u, q) if want_u or want_q else a

    @torch.no_grad()
    def export_image(self, out):
        """The weight image the HIP kernels would act with NOW, packed into `out` -- an [image_floats()] float32 tensor on the policy's device, 16-byte
        aligned -- on the current stream (C-ABI mn_dqn_export_image): a snapshot `rollout_dqn_groups` can act with later, whatever happens to the
        weights meanwhile.  The weights are read through the pointer table `_image()` maintains, i.e. from the parameters' current storage: correct
        after a fused gradient step too.  No host synchronisation."""
        import ctypes as C
        from .. import _capi
        assert out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and out.numel() == image_floats()
        st, repack = self._image(out.device)
        if repack:
            st["sig"] = None      # only the pointer table was brought up to date: the policy's own image is still to be rebuilt by its next launch
        rc = _capi.lib().mn_dqn_export_image(st["ptrs"], C.c_void_p(out.data_ptr()), _capi.stream_ptr(out.device))
        if rc:
            raise _capi.MarineNavHipError(f"mn_dqn_export_image failed ({rc})")
        return out

    def weights_changed(self):
        """The weights were written outside PyTorch's version counters (the fused gradient step, dqn/fused_train.py): repack the
        act kernel's weight image before its next launch."""
        st = getattr(self, "_fused_state", None)
        if st is not None:
            st["sig"] = None

    def _fusable(self, obs):
        return (self.use_fused_act and obs.is_cuda and not torch.is_grad_enabled() and len(self.q_net.q_net) == 5
                and self.q_net.q_net[0].out_features == 64 and self.q_net.q_net[2].out_features == 64 and obs.shape[0] > 0)

    @torch.no_grad()
    def rollout(self, env, n_steps, trace=("reward", "done", "info", "action")):
        """Every env's CURRENT episode of `env` (a VecMarineNavEnv) under this greedy policy for up to `n_steps` steps in ONE launch (C-ABI
        mn_rollout_dqn): per step what `act_batch(env.obs)` chooses, then the env step -- bit-identical to that loop.  No resets: a finished env idles
        (reward 0, done 1, terminal info, action -1 in the traces; its obs / Q entries stay 0 / NaN); an env still alive afterwards continues with the
        next call.  Returns the requested traces ([n_steps][n]; "obs" [n_steps][n][26], "q" [n_steps][n][9], "traj" [n_steps][n][N][2] float64: the sub-step
        positions of every step while the env is alive, f64 envs) and `final_obs`, or None where the fused
        act kernel would not run either (CPU, another net_arch, use_fused_act = False): the caller runs the loop instead."""
        import ctypes as C
        from .. import _capi
        from ..episodes import trace_buffers
        if not (hasattr(env, "h") and self._fusable(env.obs)):
            return None
        T, n, dev = int(n_steps), env.n_envs, env.device
        st, repack = self._image(dev)
        tr = trace_buffers(T, n, dev, trace, obs_dim=self.state_size, n_actions=self.action_size, n_substeps=int(env.params.N))
        p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
        env.set_trajectory_trace(tr.get("traj"))
        rc = _capi.lib().mn_rollout_dqn(env.h, st["ptrs"], p(st["image"]), int(repack), T, p(env.obs), p(tr.get("obs")), p(tr.get("reward")),
                                        p(tr.get("done")), p(tr.get("info")), p(tr.get("action")), p(tr.get("q")), env._stream())
        if rc:
            raise _capi.MarineNavHipError(f"mn_rollout_dqn failed ({rc})")
        out = dict(tr)
        out["final_obs"] = env.obs
        return out

    @torch.no_grad()
    def q_values(self, obs):
        obs = obs.to(self.device, torch.float32).view(-1, self.state_size)
        if self._fusable(obs):
            return self._fused(obs.contiguous(), True, False)[0]
        return self.q_net(obs)

    @torch.no_grad()
    def act_batch(self, obs):
        """QNetwork._predict (dqn/policies.py:69-73): argmax_a Q(obs, a), one int32 per row."""
        obs = obs.to(self.device, torch.float32).view(-1, self.state_size)
        if self._fusable(obs):
            return self._fused(obs.contiguous(), False, True)[1]
        return self.q_net(obs).argmax(dim=1).to(torch.int32)

    exploration_rate = 0.05      # sb3 DQN's value after its exploration schedule (exploration_final_eps, dqn/dqn.py:82)

    def predict(self, observation, deterministic=True):
        """sb3 surface used by run_experiments.py:86: `action, _ = agent.predict(obs, deterministic=True)`.  With
        deterministic=False, DQN.predict's epsilon-greedy (dqn/dqn.py:249-257): ONE `np.random.rand()` draw per call decides whether
        the whole (vector of) observation(s) gets uniformly random actions instead of the greedy ones."""
        obs = torch.as_tensor(np.asarray(observation), dtype=torch.float32)
        single = obs.dim() == 1
        if not deterministic and np.random.rand() < self.exploration_rate:
            n = 1 if single else obs.view(-1, self.state_size).shape[0]
            a = np.array([np.random.randint(self.action_size) for _ in range(n)], dtype=np.int64)
            return (a[0] if single else a), None
        a = self.act_batch(obs.view(-1, self.state_size)).cpu().numpy().astype(np.int64)
        return (a[0] if single else a), None
