"""DQN learner on the vector env: the batched counterpart of the reference's DQN baseline training
(train_sb3_model.py:100-122 -> its modified stable-baselines3 `DQN`, thirdparty/stable_baselines3/dqn/dqn.py).

Same network (`ObsEncoderPolicy`, dqn/policies.py:212-240 = `dqn.policy.DQNPolicy` here), same update rule
(`DQN.train`, dqn.py:188-230: 1-step TD target from the target network, smooth-L1 loss, clip_grad_norm_(10), Adam 1e-4),
same schedules (`_on_step`, dqn.py:169-186: hard target copy every `target_update_interval` env steps, linear
exploration over the first `exploration_fraction` of training), driven by `VecMarineNavEnv` and the device replay ring
instead of DummyVecEnv (common/vec_env/dummy_vec_env.py:38-55: auto-reset, terminal observation kept for the
transition).

Acting runs on the DQN act kernel (csrc/dqn_act.hip via DQNPolicy).  The gradient step is eager PyTorch by default; with
`fused_train=True` (GPU, batch <= 256) every step drawn from the replay ring -- `train()` without an explicit batch, hence `learn_vec`
-- is ONE launch of the fused HIP step (csrc/dqn_train.hip, dqn/fused_train.py) on the same parameters and the same Adam state.

`fused_collect=True` (GPU, `policy.use_fused_act`) moves the collect phase onto the device: `act_batch(obs, eps)` is ONE launch that also draws the
exploration (csrc/dqn_collect.hip, C-ABI mn_dqn_act_rng) from the library's counter-based generator under the seed `seed + 4321` and the call counter
`act_calls` -- pinned to the host twin tests/dqn_rng_twin.py -- and the env step writes the transitions into the replay ring itself
(`train_env.step_append`).  The draws differ from the torch.Generator's, so it is opt-in.
"""
import copy
import os

import numpy as np
import torch
import torch.nn.functional as F

from ..iqn.replay_buffer import ReplayBuffer
from .policy import DQNPolicy


def split_at_target_sync(done, n_steps, sync_every):
    """Cut a run of `n_steps` gradient steps, `done` steps into the run, at the hard target copies that fall every `sync_every` steps: a list of
    `(steps, sync_after)` segments in order, `sync_after` True where a copy follows the segment's last step.  The target network is constant inside a
    segment, which is what a multi-step call (`DQNAgent.train_many`) needs.  `sync_every` None or 0: no copies among these steps."""
    if n_steps <= 0:
        return []
    if not sync_every:
        return [(n_steps, False)]
    segments = []
    while n_steps > 0:
        steps = min(n_steps, sync_every - done % sync_every)
        done += steps
        n_steps -= steps
        segments.append((steps, done % sync_every == 0))
    return segments


class DQNAgent:
    def __init__(self, state_size=26, action_size=9, learning_rate=1e-4, buffer_size=1_000_000, learning_starts=50000,
                 batch_size=32, tau=1.0, gamma=0.99, train_freq=4, gradient_steps=1, target_update_interval=10000,
                 exploration_fraction=0.1, exploration_initial_eps=1.0, exploration_final_eps=0.05, max_grad_norm=10,
                 device="cuda:0", seed=0, fused_train=False, fused_collect=False):
        self.device = torch.device(device)
        torch.manual_seed(seed)                                    # sb3 set_random_seed (base_class.py) before the policy is built
        self.policy = DQNPolicy(state_size, action_size, device=device)
        self.q_net = self.policy.q_net
        self.q_net_target = copy.deepcopy(self.q_net)              # dqn/policies.py:150-156: target starts as a copy
        self.q_net_target.eval()
        self.optimizer = torch.optim.Adam(self.q_net.parameters(), lr=learning_rate)
        self.memory = ReplayBuffer(buffer_size, batch_size, device, seed, gamma, 1, state_size)
        self.batch_size, self.tau, self.gamma = batch_size, tau, gamma
        self.learning_starts, self.train_freq, self.gradient_steps = learning_starts, train_freq, gradient_steps
        self.target_update_interval, self.max_grad_norm = target_update_interval, max_grad_norm
        self.exploration_fraction = exploration_fraction
        self.exploration_initial_eps, self.exploration_final_eps = exploration_initial_eps, exploration_final_eps
        self.action_size = action_size
        self.gen = torch.Generator(device=self.device)
        self.gen.manual_seed(int(seed) + 4321)
        self.num_timesteps = 0
        self.n_updates = 0
        self.learning_rate = learning_rate
        self.fused_train = fused_train      # True: steps drawn from the ring run csrc/dqn_train.hip (GPU, batch <= 256)
        self._fused, self._train_path = None, "torch"
        self.fused_collect = fused_collect      # True: act_batch is ONE mn_dqn_act_rng launch with the library's draws (GPU, policy.use_fused_act)
        self.act_seed, self.act_calls = int(seed) + 4321, 0      # ... keyed by this seed and the number of act_batch calls so far

    # ---- the fused HIP gradient step -------------------------------------------------------------------------------
    def _fused_trainer(self):
        from .fused_train import FusedTrainer
        if self._fused is None or not self._fused.owns(self):
            self._fused = FusedTrainer(self)
        return self._fused

    def _uses_fused(self):
        from .fused_train import MAX_BATCH
        return self.fused_train and self.device.type == "cuda" and self.batch_size <= MAX_BATCH

    def _enter_train_path(self, path):
        """Both gradient-step paths update ONE Adam state (the moments are shared memory, dqn/fused_train.py); the step count is
        handed over whenever the path changes."""
        if self._train_path == path:
            return
        if self._fused is not None and self._fused.owns(self):
            if path == "torch" and self._train_path == "hip":
                self._fused.sync_to_optimizer(self.optimizer)
            elif path == "hip" and self._train_path == "torch":
                self._fused.sync_from_optimizer(self.optimizer)
                self._fused.point_grads()
        self._train_path = path

    def train_fused(self, idx=None):
        """One fused HIP gradient step on the replay ring: on rows `idx` [B] (i64), or (None) on a batch of `batch_size` rows drawn inside
        the launch.  Returns the loss (device scalar)."""
        m = self.memory
        ft = self._fused_trainer()
        self._enter_train_path("hip")
        loss = ft.step((m.states, m.actions, m.rewards, m.next_states, m.dones), m.size, self.batch_size, idx)
        self.n_updates += 1
        return loss.clone()

    def _uses_multi_step(self):
        from .fused_train import MULTI_MAX_BATCH
        return self._uses_fused() and self.batch_size <= MULTI_MAX_BATCH

    def train_many(self, n_steps, idx=None):
        """`n_steps` gradient steps on fresh samples of the replay ring (or on rows `idx` [n_steps][B]); returns the [n_steps] losses and raises
        `n_updates` by `n_steps`.  With `fused_train` and batch <= 32 they are ONE multi-step HIP call (`FusedTrainer.steps`), bit for bit the loop of
        `train()`; anywhere else they ARE that loop.  The target network must not be copied among the steps (`split_at_target_sync`)."""
        if n_steps <= 0:
            return torch.zeros(0, device=self.device)
        m = self.memory
        if self._uses_multi_step():
            ft = self._fused_trainer()
            self._enter_train_path("hip")
            losses = ft.steps((m.states, m.actions, m.rewards, m.next_states, m.dones), m.size, self.batch_size, n_steps, idx)
            self.n_updates += n_steps
            return losses.clone()
        if idx is None:
            return torch.stack([self.train() for _ in range(n_steps)])
        if self._uses_fused():
            return torch.stack([self.train_fused(rows) for rows in idx])
        return torch.stack([self.train(tuple(t[rows] for t in (m.states, m.actions, m.rewards, m.next_states, m.dones))) for rows in idx])

    # ---- update rule -----------------------------------------------------------------------------------------------
    def train(self, experiences=None):
        """One gradient step of DQN.train (dqn.py:196-224) on `experiences` = (obs, actions [B,1] i64, rewards [B,1],
        next_obs, dones [B,1] f32) or on a fresh sample of the replay ring.  Returns the loss (device scalar).
        With `fused_train` a fresh sample is drawn and trained on inside one HIP launch (`train_fused`); an explicit batch stays eager."""
        if experiences is None and self._uses_fused():
            return self.train_fused()
        self._enter_train_path("torch")
        obs, actions, rewards, next_obs, dones = experiences if experiences is not None else self.memory.sample()
        with torch.no_grad():
            next_q = self.q_net_target(next_obs).max(dim=1)[0].reshape(-1, 1)
            target_q = rewards + (1 - dones) * self.gamma * next_q
        current_q = torch.gather(self.q_net(obs), dim=1, index=actions.long())
        loss = F.smooth_l1_loss(current_q, target_q)
        self.optimizer.zero_grad()
        loss.backward()
        torch.nn.utils.clip_grad_norm_(self.q_net.parameters(), self.max_grad_norm)
        self.optimizer.step()
        self.n_updates += 1
        return loss.detach()

    def exploration_rate(self, total_timesteps):
        """get_linear_fn(initial, final, fraction) of the progress (common/utils.py), as dqn.py:120-124,183."""
        progress = self.num_timesteps / max(1, total_timesteps)
        if progress > self.exploration_fraction:
            return self.exploration_final_eps
        return self.exploration_initial_eps + progress * (self.exploration_final_eps - self.exploration_initial_eps) / self.exploration_fraction

    @torch.no_grad()
    def act_batch(self, obs, eps):
        """dqn.py:232-262 per env: a uniform random action with probability eps, else argmax_a Q.  With `fused_collect` one launch whose draws are
        `tests/dqn_rng_twin.dqn_actions(act_seed, act_calls, eps, greedy)`; `act_calls` advances by one per call, whatever eps is."""
        if self.uses_fused_collect():
            obs = obs.to(self.device, torch.float32).view(-1, self.policy.state_size).contiguous()
            if not self.policy._fusable(obs):
                raise RuntimeError("fused_collect: the policy cannot act through the fused kernel on this batch (empty, or another net_arch); there is no other form")
            actions = self.policy.act_rng(obs, self.act_seed, self.act_calls, eps)
            self.act_calls += 1
            return actions
        greedy = self.policy.act_batch(obs)
        if eps <= 0.0:
            return greedy
        n = obs.shape[0]
        u = torch.rand(n, device=obs.device, generator=self.gen)
        rnd = torch.randint(0, self.action_size, (n,), device=obs.device, dtype=torch.int32, generator=self.gen)
        return torch.where(u < eps, rnd, greedy)

    def uses_fused_collect(self):
        return self.fused_collect and self.device.type == "cuda" and self.policy.use_fused_act

    # ---- vector loop -----------------------------------------------------------------------------------------------
    def learn_vec(self, total_vector_steps, train_env, total_timesteps=None, callback=None):
        """off_policy_algorithm.py:collect_rollouts / train cadence on n envs at once: every vector step adds n
        transitions; after `learning_starts` env steps, `gradient_steps` updates every `train_freq` VECTOR steps;
        target network copied every `target_update_interval` env steps (rounded to vector steps)."""
        n = train_env.n_envs
        total_timesteps = total_timesteps or total_vector_steps * n
        obs = train_env.reset()
        tgt_every = max(1, int(round(self.target_update_interval / n)))
        losses = []
        for it in range(total_vector_steps):
            eps = self.exploration_rate(total_timesteps)
            a = self.act_batch(obs, eps)
            if self.uses_fused_collect():      # the step kernel appends the transitions itself
                nxt, reward, done, info = train_env.step_append(a, obs, self.memory)
            else:
                nxt, reward, done, info = train_env.step(a)
                self.memory.add_vector_step(obs, a, reward, nxt, done)
            obs = train_env.reset_done()
            self.num_timesteps += n
            if (it + 1) % tgt_every == 0:                                       # dqn.py:175-176, tau = 1 -> hard copy
                self.sync_target()
            if self.num_timesteps > self.learning_starts and (it + 1) % self.train_freq == 0 and len(self.memory) >= self.batch_size:
                # (the target copy above falls between vector steps, never among these gradient steps: one segment)
                for steps, _ in split_at_target_sync(self.n_updates, self.gradient_steps, None):
                    losses.extend(self.train_many(steps))
            if callback is not None:
                callback(self, it)
        return dict(vector_steps=total_vector_steps, n_updates=self.n_updates,
                    mean_loss=float(torch.stack(losses).mean()) if losses else float("nan"))

    @torch.no_grad()
    def sync_target(self):
        """Polyak update of the target network (tau = 1: the hard copy, one copy of the flat buffer on the fused path)."""
        if self.tau == 1.0 and self._fused is not None and self._fused.owns(self):
            self._fused.sync_target()
            return
        for tp, lp in zip(self.q_net_target.parameters(), self.q_net.parameters()):
            tp.mul_(1 - self.tau).add_(lp, alpha=self.tau)

    # ---- checkpoints: the `policy.pth` of an sb3 zip (q_net.* and q_net_target.* keys) -----------------------------
    def state_dict(self):
        sd = {k: v.detach().clone() for k, v in self.policy.state_dict().items()}
        sd.update({"q_net_target." + k: v.detach().clone() for k, v in self.q_net_target.state_dict().items()})
        return sd

    # ---- checkpoints of a training run (train_dqn --checkpoint-every / --stop-after / --resume) --------------------
    def _owned_trainer(self):
        return self._fused if self._fused is not None and self._fused.owns(self) else None

    def _adam_state(self):
        """(exp_avg [P], exp_avg_sq [P], step) of the ONE Adam state both gradient-step paths update, from whichever path holds it: the fused trainer's
        flat buffers and device counter, or torch.optim.Adam's per-parameter state (zeros and 0 before the first step)."""
        params = list(self.q_net.parameters())
        ft = self._owned_trainer()
        st0 = self.optimizer.state.get(params[0], None)
        opt_step = int(float(st0["step"])) if st0 is not None and "step" in st0 else 0
        if ft is not None:      # (the optimizer's moments are views of these)
            return ft.exp_avg.detach().cpu().clone(), ft.exp_avg_sq.detach().cpu().clone(), int(ft.step_dev.item()) if self._train_path == "hip" else opt_step
        flat = lambda key: torch.cat([(self.optimizer.state[p][key] if key in self.optimizer.state.get(p, {}) else torch.zeros_like(p)).detach().reshape(-1).cpu()
                                      for p in params])
        return flat("exp_avg"), flat("exp_avg_sq"), opt_step

    def _load_adam_state(self, exp_avg, exp_avg_sq, step):
        """The reverse, IN PLACE: into the fused trainer's flat buffers where there is one (the optimizer's views of them follow), into the optimizer's own
        tensors otherwise, and the step count into both -- whichever path runs next finds what the saving agent's path left."""
        ft = self._owned_trainer()
        if ft is not None:
            ft.exp_avg.copy_(exp_avg); ft.exp_avg_sq.copy_(exp_avg_sq)
            ft.step_dev.fill_(int(step))
        opt = self.optimizer
        on_dev = any(g.get("fused") or g.get("capturable") for g in opt.param_groups)
        off = 0
        with torch.no_grad():
            for p in self.q_net.parameters():
                n = p.numel()
                st = opt.state[p]
                if "exp_avg" not in st:
                    st["exp_avg"], st["exp_avg_sq"] = torch.zeros_like(p), torch.zeros_like(p)
                if "step" not in st:
                    st["step"] = torch.zeros((), dtype=torch.float32, device=p.device if on_dev else "cpu")
                if ft is None:
                    st["exp_avg"].copy_(exp_avg[off:off + n].view(p.shape)); st["exp_avg_sq"].copy_(exp_avg_sq[off:off + n].view(p.shape))
                st["step"].fill_(float(int(step)))
                off += n
        self._train_path = None      # both paths hold the same state now: nothing to hand over at the next step

    def global_rng_state(self):
        """torch's CPU and device global generator states and python's: the agent's constructor seeds them, nothing in the training loop draws from them."""
        import random
        return dict(torch_cpu_rng=torch.get_rng_state(), torch_device_rng=torch.cuda.get_rng_state(self.device) if self.device.type == "cuda" else None,
                    py_random=random.getstate())

    def train_state_dict(self):
        """Everything of the learner a continued training run depends on, as CPU tensors and plain values (`state_dict()` is the policy.pth of the sb3-style
        zips and keeps its keys; the replay ring has its own `memory.state_dict()`): both networks, the ONE Adam state from whichever gradient-step path
        holds it, the fused step's {seed, draw counter} (what a trainer made now would start from, where there is none yet), the update and timestep
        counts, the fused collect's {seed, calls}, the eager collect's generator, and torch's CPU and device generators and python's.  Not state: the act
        kernel's weight image, the workspaces, the multi-step buffers and `last_idx` -- the next call that needs them rebuilds them."""
        ft = self._owned_trainer()
        m, v, step = self._adam_state()
        cpu = lambda net: {k: t.detach().cpu().clone() for k, t in net.state_dict().items()}
        train_rng = (ft.rng_state.cpu() if ft is not None
                     else torch.tensor([int(self.memory.gen.initial_seed()) & 0x7FFFFFFFFFFFFFFF, 0], dtype=torch.int64))
        return dict(q_net=cpu(self.q_net), q_net_target=cpu(self.q_net_target), exp_avg=m, exp_avg_sq=v, adam_step=int(step), train_rng=train_rng,
                    n_updates=int(self.n_updates), num_timesteps=int(self.num_timesteps), act_seed=int(self.act_seed), act_calls=int(self.act_calls),
                    gen=self.gen.get_state(), **self.global_rng_state())

    def load_train_state_dict(self, sd):
        """Continue where `train_state_dict()` was taken, on either gradient-step path.  Everything is written IN PLACE: where the fused path is in use its
        trainer is made first, and the networks, the moments, the step and the draw counter go into its existing flat buffers -- their addresses are what a
        `LearnerGroup`'s device table holds.  Load the agent LAST: the state holds torch's generator states, which nothing behind it may move."""
        import random
        if self._uses_fused():
            self._fused_trainer()
        ft = self._owned_trainer()
        with torch.no_grad():
            for net, key in ((self.q_net, "q_net"), (self.q_net_target, "q_net_target")):
                own = net.state_dict()
                if own.keys() != sd[key].keys():
                    raise ValueError(f"DQNAgent.load_train_state_dict: the saved {key} has other parameters ({sorted(set(own) ^ set(sd[key]))})")
                for k, t in own.items():
                    t.copy_(sd[key][k])
        self._load_adam_state(sd["exp_avg"], sd["exp_avg_sq"], sd["adam_step"])
        if ft is not None:
            ft.rng_state.copy_(sd["train_rng"])
            ft.point_grads()
            ft._ws, ft._idx_out, ft._multi = {}, {}, {}      # caches: rebuilt by the next call of their shape
            ft.__dict__.pop("last_idx", None)
        self.n_updates, self.num_timesteps = int(sd["n_updates"]), int(sd["num_timesteps"])
        self.act_seed, self.act_calls = int(sd["act_seed"]), int(sd["act_calls"])
        self.policy.weights_changed()      # the act kernel's weight image repacks on the next act
        self.gen.set_state(sd["gen"])
        torch.set_rng_state(sd["torch_cpu_rng"])
        if sd["torch_device_rng"] is not None and self.device.type == "cuda":
            torch.cuda.set_rng_state(sd["torch_device_rng"], self.device)
        random.setstate(sd["py_random"])

    def save(self, directory):
        os.makedirs(directory, exist_ok=True)
        torch.save(self.state_dict(), os.path.join(directory, "policy.pth"))

    def load(self, path):
        """`path`: an sb3 checkpoint zip, a policy.pth or the q_net npz fixture (target := q_net if absent)."""
        import io, zipfile
        if path.endswith(".npz"):
            sd = {k: torch.from_numpy(v) for k, v in np.load(path).items()}
        elif zipfile.is_zipfile(path) and "policy.pth" in zipfile.ZipFile(path).namelist():
            with zipfile.ZipFile(path) as z:
                sd = torch.load(io.BytesIO(z.read("policy.pth")), map_location="cpu")
        else:
            sd = torch.load(path, map_location="cpu")
        self.policy.load_state_dict({k: v for k, v in sd.items() if k.startswith("q_net.")}, strict=True)
        tgt = {k[len("q_net_target."):]: v for k, v in sd.items() if k.startswith("q_net_target.")}
        self.q_net_target.load_state_dict(tgt if tgt else self.q_net.state_dict())
