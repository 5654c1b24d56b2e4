"""Device-resident replay memory (counterpart of thirdparty/IQN/replay_buffer.py:6-59).

The reference keeps a deque of python tuples and stacks a batch on every sample; here the
transitions live in HBM as a ring of tensors and a whole vector step (n_envs transitions) is
appended with one indexed copy.

n_step > 1 (replay_buffer.py:26-41; never used by the reference's scripts, part of the constructor surface): every
environment stream keeps its last n_step transitions; once it holds n_step of them each further add emits
(s_{t-n+1}, a_{t-n+1}, sum_i gamma^i r_{t-n+1+i}, s'_t, done_t) -- the reference's sliding window, which (as there) does
not restart at episode ends.  That is nstep_mode "reference" (default).  nstep_mode "episode" is the standard n-step
transition: the window is cut at its first episode end (return over the steps up to it, that step's next state, done = 1),
so nothing of the next episode enters a transition; every step still heads exactly one emitted window.  The rule, operation
by operation: include/marinenav_hip.h, "n-step window".

The fused `mn_step_append` path stores 1-step transitions only, so the agent uses step + `add_vector_step` when n_step > 1:
on a CUDA ring with 2 <= n_step <= 16 that is ONE launch (`mn_replay_append_nstep`, csrc/replay.hip; `use_nstep_kernel`),
otherwise -- the CPU, n_step > 16, `add_batch` -- the torch ops of `_nstep_window`, which the kernel equals bit for bit.

prioritized = True (opt-in): a `PriorityStore` (iqn/priority.py) rides next to the ring -- every row the ring writes, by whichever of the paths above, gets the
largest mass assigned so far (one small launch in stream order behind the write; with n_step > 1 only when rows were emitted).  `sample()` stays the uniform
draw; the prioritized draw is `priority.sample` (IQNAgent.train_from_memory with per = True).
"""
import torch

NSTEP_MODES = ("reference", "episode")


class ReplayBuffer:
    def __init__(self, buffer_size, batch_size, device, seed, gamma, n_step=1, state_size=26, nstep_mode="reference", prioritized=False):
        if int(n_step) < 1:
            raise ValueError("n_step must be >= 1")
        if nstep_mode not in NSTEP_MODES:
            raise ValueError(f"nstep_mode must be one of {NSTEP_MODES}, not {nstep_mode!r}")
        self.device = torch.device(device)
        self.capacity = int(buffer_size)
        self.batch_size = int(batch_size)
        self.gamma = gamma
        self.n_step = n_step
        self.nstep_mode = nstep_mode
        self.use_nstep_kernel = True     # add_vector_step, CUDA ring, 2 <= n_step <= 16: the window append as one HIP launch; False: the torch ops (same bits)
        self.gen = torch.Generator(device=self.device)
        self.gen.manual_seed(int(seed))
        c = self.capacity
        self.states = torch.zeros(c, state_size, dtype=torch.float32, device=self.device)
        self.next_states = torch.zeros(c, state_size, dtype=torch.float32, device=self.device)
        self.actions = torch.zeros(c, 1, dtype=torch.int64, device=self.device)
        self.rewards = torch.zeros(c, 1, dtype=torch.float32, device=self.device)
        self.dones = torch.zeros(c, 1, dtype=torch.float32, device=self.device)
        self.size = 0
        self.ptr = 0
        self._hist = None     # n_step > 1: per-stream window of the last n_step transitions
        self._gamma_pow = None   # the kernel's table of float32(gamma ** i), built at its first call
        self.priority = None  # prioritized: the rows' masses, block sums and sampling state (iqn/priority.py)
        if prioritized:
            from .priority import PriorityStore
            self.priority = PriorityStore(self.capacity, self.device, seed)
        self.version = 0      # bumped by every write to the ring (a batch the gradient kernels staged from it is then stale)

    def add(self, state, action, reward, next_state, done):
        """One transition (replay_buffer.py:26-34)."""
        as_t = lambda x, dt: torch.as_tensor(x, dtype=dt, device=self.device)
        self.add_batch(as_t(state, torch.float32).view(1, -1), as_t([action], torch.int64),
                       as_t([reward], torch.float32), as_t(next_state, torch.float32).view(1, -1),
                       as_t([float(done)], torch.float32))

    def _nstep_window(self, states, actions, rewards, next_states, dones):
        """replay_buffer.py:26-41 for `k` parallel streams (row i of every call belongs to stream i): returns the k n-step
        transitions this add completes, or None while the windows are still filling.  nstep_mode "episode": the window cut at its first done (the module
        docstring; include/marinenav_hip.h, "n-step window").  The yardstick of `mn_replay_append_nstep`, which leaves the same bits."""
        k = states.shape[0]
        n = self.n_step
        episode = self.nstep_mode == "episode"
        h = self._window(k, states.shape[1])
        slot = h["count"] % n
        h["s"][slot].copy_(states); h["a"][slot].copy_(actions.view(-1)); h["r"][slot].copy_(rewards.view(-1))
        if episode:
            h["ns"][slot].copy_(next_states); h["d"][slot].copy_(dones.view(-1) != 0)
        h["count"] += 1
        if h["count"] < n:
            return None
        oldest = h["count"] % n                     # the slot the NEXT add overwrites = the window's first transition
        ret = torch.zeros(k, dtype=torch.float32, device=self.device)
        if not episode:
            for i in range(n):                      # Return += gamma**idx * reward_idx, in the reference's order
                ret = ret + (self.gamma ** i) * h["r"][(oldest + i) % n]
            return h["s"][oldest].clone(), h["a"][oldest].clone(), ret, next_states, dones
        # the window cut at its first done: slot j (age order) is the last one the transition takes in
        open_ = torch.ones(k, dtype=torch.bool, device=self.device)       # no done in the slots in front of slot i
        j = torch.full((k,), n - 1, dtype=torch.int64, device=self.device)
        for i in range(n):
            at = (oldest + i) % n
            ret = torch.where(open_, ret + (self.gamma ** i) * h["r"][at], ret)
            d = h["d"][at] != 0
            j = torch.where(open_ & d, torch.full_like(j, i), j)
            open_ = open_ & ~d
        rows = torch.arange(k, device=self.device)
        return h["s"][oldest].clone(), h["a"][oldest].clone(), ret, h["ns"][(oldest + j) % n, rows], (~open_).to(torch.float32)

    def _window(self, k, state_size):
        """The per-stream window of `k` streams (made, or made anew for another k): s [n][k][state] f32, a [n][k] i64, r [n][k] f32, count = adds so far; episode
        mode: ns [n][k][state] f32 and d [n][k] u8 as well."""
        h, n = self._hist, self.n_step
        if h is None or h["s"].shape[1] != k:
            z = lambda *shape, dt=torch.float32: torch.zeros(*shape, dtype=dt, device=self.device)
            h = self._hist = dict(s=z(n, k, state_size), a=z(n, k, dt=torch.int64), r=z(n, k), count=0)
            if self.nstep_mode == "episode":
                h.update(ns=z(n, k, state_size), d=z(n, k, dt=torch.uint8))
        return h

    def _append_nstep_kernel(self, obs, actions_i32, reward, next_obs, done_u8):
        """`add_batch` of one vector step with n_step > 1 as ONE launch (mn_replay_append_nstep): the window slot written, the head emitted once the window
        is full -- the tensors `_nstep_window` + `add_batch` leave, bit for bit."""
        import ctypes as C
        from .. import _capi
        k, n = obs.shape[0], int(self.n_step)
        for t in (obs, actions_i32, reward, next_obs, done_u8):
            assert t.is_cuda and t.is_contiguous()
        assert actions_i32.dtype == torch.int32 and done_u8.dtype == torch.uint8 and obs.dtype == torch.float32 and obs.shape[1] == 26
        h = self._window(k, obs.shape[1])
        if self._gamma_pow is None:
            self._gamma_pow = _capi.MnNstepGamma()
            for i in range(n):
                self._gamma_pow.g[i] = self.gamma ** i      # (rounded to float32 once, as torch rounds the scalar of `gamma ** i * r`)
        p = lambda t: C.c_void_p(t.data_ptr())
        episode = self.nstep_mode == "episode"
        rc = _capi.lib().mn_replay_append_nstep(p(obs), p(actions_i32), p(reward), p(next_obs), p(done_u8), p(h["s"]), p(h["a"]), p(h["r"]),
                                                p(h["ns"]) if episode else None, p(h["d"]) if episode else None, h["count"], n, self._gamma_pow,
                                                _capi.NSTEP_EPISODE if episode else _capi.NSTEP_REFERENCE, p(self.states), p(self.next_states),
                                                p(self.actions), p(self.rewards), p(self.dones), k, self.ptr, self.capacity, _capi.stream_ptr(self.device))
        if rc:
            raise _capi.MarineNavHipError(f"mn_replay_append_nstep failed ({rc})")
        h["count"] += 1
        if h["count"] >= n:
            self.advance(k)

    def add_vector_step(self, obs, actions_i32, reward, next_obs, done_u8):
        """One vector step of the HIP env (device tensors exactly as VecMarineNavEnv returns them:
        obs / next_obs [n,26] f32, actions [n] i32, reward [n] f32, done [n] u8) appended by ONE kernel
        (csrc/replay.hip); same FIFO semantics as add_batch.  n_step > 1: one launch too (`_append_nstep_kernel`) for 2 <= n_step <= 16 on a CUDA ring
        unless `use_nstep_kernel` is off; else the torch window."""
        if self.n_step > 1:
            if self.use_nstep_kernel and self.device.type == "cuda" and self.n_step <= 16:      # (MN_NSTEP_MAX)
                return self._append_nstep_kernel(obs, actions_i32, reward, next_obs, done_u8)
            return self.add_batch(obs, actions_i32.long(), reward, next_obs, done_u8.float())
        import ctypes as C
        from .. import _capi
        n = obs.shape[0]
        p = lambda t: C.c_void_p(t.data_ptr())
        for t in (obs, actions_i32, reward, next_obs, done_u8):
            assert t.is_cuda and t.is_contiguous()
        assert actions_i32.dtype == torch.int32 and done_u8.dtype == torch.uint8 and obs.dtype == torch.float32
        stream = _capi.stream_ptr(self.device)
        rc = _capi.lib().mn_replay_append(p(obs), p(actions_i32), p(reward), p(next_obs), p(done_u8), p(self.states),
                                          p(self.next_states), p(self.actions), p(self.rewards), p(self.dones),
                                          n, self.ptr, self.capacity, stream)
        if rc:
            raise _capi.MarineNavHipError(f"mn_replay_append failed ({rc})")
        m = min(n, self.capacity)
        if self.priority is not None:
            self.priority.append(self.ptr, m)
        self.ptr = (self.ptr + m) % self.capacity
        self.size = min(self.capacity, self.size + m)
        self.version += 1

    def add_batch(self, states, actions, rewards, next_states, dones):
        """n transitions at once; FIFO eviction like deque(maxlen).  With n_step > 1 row i is the next transition of stream i."""
        if self.n_step > 1:
            out = self._nstep_window(states, actions, rewards, next_states, dones)
            if out is None:
                return
            states, actions, rewards, next_states, dones = out
        n = states.shape[0]
        if n > self.capacity:   # only the newest `capacity` survive
            states, actions, rewards, next_states, dones = (t[-self.capacity:] for t in (states, actions, rewards, next_states, dones))
            n = self.capacity
        end = self.ptr + n
        if end <= self.capacity:
            sl = slice(self.ptr, end)
            self.states[sl].copy_(states); self.next_states[sl].copy_(next_states)
            self.actions[sl, 0].copy_(actions.view(-1)); self.rewards[sl, 0].copy_(rewards.view(-1))
            self.dones[sl, 0].copy_(dones.view(-1))
        else:
            k = self.capacity - self.ptr
            n_step, self.n_step = self.n_step, 1      # the two halves are already n-step transitions
            try:
                self.add_batch(states[:k], actions[:k], rewards[:k], next_states[:k], dones[:k])
                self.add_batch(states[k:], actions[k:], rewards[k:], next_states[k:], dones[k:])
            finally:
                self.n_step = n_step
            return
        if self.priority is not None:
            self.priority.append(self.ptr, n)
        self.ptr = end % self.capacity
        self.size = min(self.capacity, self.size + n)
        self.version += 1

    def advance(self, n):
        """Ring bookkeeping after `n` transitions were written at `ptr` by a kernel (mn_step_append)."""
        m = min(int(n), self.capacity)
        if self.priority is not None:
            self.priority.append(self.ptr, m)
        self.ptr = (self.ptr + m) % self.capacity
        self.size = min(self.capacity, self.size + m)
        self.version += 1

    def sample_indices(self, b):
        """`b` distinct uniform row indices in [0, size) (random.sample, replay_buffer.py:47) without a full
        permutation of the ring: draw with replacement, keep first occurrences, top up until b are distinct (each
        accepted index is uniform over what the earlier ones left, i.e. sequential sampling without replacement)."""
        assert self.size >= b
        if self.size <= 4 * b:      # dense case: a permutation is the cheap way
            return torch.randperm(self.size, device=self.device, generator=self.gen)[:b]
        chosen = torch.empty(0, dtype=torch.int64, device=self.device)
        while chosen.numel() < b:
            cand = torch.randint(0, self.size, (2 * b,), device=self.device, generator=self.gen)
            allv = torch.cat([chosen, cand])
            # stable first-occurrence filter
            srt, order = torch.sort(allv, stable=True)
            first = torch.ones_like(srt, dtype=torch.bool)
            first[1:] = srt[1:] != srt[:-1]
            keep = torch.zeros_like(first)
            keep[order] = first
            chosen = allv[keep][:b]
        return chosen

    def sample(self, batch_size=None):
        """Uniform without replacement (random.sample, replay_buffer.py:47) -> float32 / int64 tensors."""
        b = self.batch_size if batch_size is None else batch_size
        idx = self.sample_indices(b)
        return (self.states[idx], self.actions[idx], self.rewards[idx], self.next_states[idx], self.dones[idx])

    # ---- checkpoints ---------------------------------------------------------------------------
    def state_dict(self):
        """The ring as CPU tensors and plain numbers: rows [0, size) only (a young run fills a fraction of its capacity), `ptr`, `size`, `version`, the
        sampling generator's state and -- n_step > 1 -- the per-stream window.  `load_state_dict` into a ring of the same capacity continues bit for bit:
        the same rows, the same next `sample()`, the same next n-step transition."""
        s = self.size
        sd = dict(capacity=self.capacity, n_step=int(self.n_step), size=int(s), ptr=int(self.ptr), version=int(self.version), gen=self.gen.get_state(),
                  states=self.states[:s].cpu(), next_states=self.next_states[:s].cpu(), actions=self.actions[:s].cpu(), rewards=self.rewards[:s].cpu(),
                  dones=self.dones[:s].cpu(), hist=None, nstep_mode=self.nstep_mode)
        if self._hist is not None:
            h = self._hist
            sd["hist"] = dict({k: v.cpu() for k, v in h.items() if k != "count"}, count=int(h["count"]))      # (s, a, r; episode mode: ns, d)
        if self.priority is not None:      # (a uniform ring's state has no such key, as before there were priorities)
            sd["priority"] = self.priority.state_dict(s)
        return sd

    def load_state_dict(self, sd):
        if int(sd["capacity"]) != self.capacity or int(sd["n_step"]) != int(self.n_step):
            raise ValueError(f"ReplayBuffer.load_state_dict: the state is of a ring of {sd['capacity']} rows with n_step {sd['n_step']}, this one has "
                             f"{self.capacity} rows and n_step {self.n_step}")
        mode = sd.get("nstep_mode", "reference")      # (absent: a state written before there were modes)
        if mode != self.nstep_mode:
            raise ValueError(f"ReplayBuffer.load_state_dict: the state is of a ring with nstep_mode {mode!r}, this one has nstep_mode {self.nstep_mode!r}")
        s = int(sd["size"])
        for name in ("states", "next_states", "actions", "rewards", "dones"):
            getattr(self, name)[:s].copy_(sd[name])
        self.size, self.ptr, self.version = s, int(sd["ptr"]), int(sd["version"])
        self.gen.set_state(sd["gen"])
        h = sd.get("hist")
        self._hist = None if h is None else dict({k: v.to(self.device).contiguous() for k, v in h.items() if k != "count"}, count=int(h["count"]))
        if self.priority is not None:      # a state saved by a uniform ring loads as uniform: every row mass 1.0
            self.priority.load_state_dict(sd.get("priority"), s)

    def __len__(self):
        return self.size
