"""IQN agent: batched act / learn around the HIP vector env.

Keeps the reference's `IQNAgent` surface (thirdparty/IQN/agent.py:10-407): the constructor keywords, `train`,
`soft_update`, `load_model` here; the reference-shaped single-env methods (`learn`, `evaluation`, `act`, `act_eval`,
`act_adaptive`, `adjust_cvar`, `linear_eps`) are the boundary layer and live in `iqn/compat.py` (`ReferenceLoopMixin`).
This file is the batched code the MI355X path actually runs: `act_batch`, `vec_step`, `learn_vec`, `evaluation_vec`,
the fused / pipelined gradient step.  Optional data-parallel training over RCCL:
one flat 35 785-float gradient bucket, one all_reduce per grad step.
"""
import json
import math
import os
import random
import sys
from collections import namedtuple

import numpy as np
import torch
import torch.optim as optim

from ..episodes import EPISODE_TRACES, energy_table, host_traces, loop_episodes, tally
from .cadence import cadence_tick
from .compat import ReferenceLoopMixin
from .model import ObsEncoder
from .replay_buffer import ReplayBuffer


def calculate_huber_loss(td_errors, k=1.0):
    """agent.py:401-407, element-wise Huber with threshold k."""
    return torch.where(td_errors.abs() <= k, 0.5 * td_errors.pow(2), k * (td_errors.abs() - 0.5 * k))


def first_argmax(q):
    """The LOWEST index that attains each row's maximum of q [B, A] -> [B] i64 (torch.argmax does not promise which of several equal maxima it returns)."""
    A = q.shape[1]
    idx = torch.arange(A, device=q.device).expand_as(q)
    return torch.where(q == q.max(1, keepdim=True)[0], idx, torch.full_like(idx, A)).min(1)[0]


class UnderActGuard:
    """Keeps `IQNAgent.reset_under_act` honest on the box the loop actually runs on.

    Episode resets under the next act kernel (mn_reset_done_async) need the reset launch to run BESIDE that kernel: a hardware queue of its own and room
    on the CUs next to the act workgroups.  HIP promises neither (another ROCm release, a partitioned or shared GPU).  When it does not happen, every late
    row waits out its bound and is then taken as it is.  So the first `preflight` vector steps of a loop run with EVERY reset forced under the act kernel
    (whatever the library's episode-count rule would decide), the late-row waits that ran out are read after step 2 and after the last preflight step,
    and -- if there were any -- the loop goes back to resets in front of the act kernel with one line on stderr instead of failing at its first evaluation
    point.  After that the count is looked at every `poll_every` steps without synchronising (mn_iqn_late_timeouts_peek).  Call `after_step(i)` behind
    vector step i = 0, 1, ...; `close()` restores the library's rule if the loop ends inside the preflight.
    The preflight steps ARE steps of the run: with the resets served in time their results are those of resets in front, bit for bit; if not, a dozen
    vector steps at the start of a run chose some actions from unfinished observation rows (at eps ~ 1, where the choice is random anyway)."""

    def __init__(self, agent, env, preflight=12, poll_every=64, log=None):
        self.agent, self.env = agent, env
        self.preflight, self.poll_every = int(preflight), int(poll_every)
        self.log = log
        self.fallback = None      # dict(step=, timeouts=) once the loop has gone back to resets in front
        self.active = bool(agent.reset_under_act) and agent.device.type == "cuda" and agent.use_fused_act and hasattr(env, "set_reset_under_act_max")
        self._restore = None
        if self.active:
            self._seen0 = agent._late_acknowledged      # (time-outs an earlier loop of this agent has already answered with its fallback do not count again)
            if self.preflight > 0:
                self._restore = env.reset_under_act_max
                env.set_reset_under_act_max(2 ** 31 - 1)

    def _end_preflight(self):
        if self._restore is not None:
            self.env.set_reset_under_act_max(self._restore)
            self._restore = None

    def _fall_back(self, step, k):
        self.agent.reset_under_act = False
        self.agent.reset_fallback = True      # (vec_step: from here on the resets may still ride in the next act call's preparation launch, never under the act kernel)
        self.env.join_reset()
        self._end_preflight()
        self.fallback = dict(step=int(step), timeouts=int(k))
        self.agent._late_acknowledged = self._seen0 + int(k)
        self.active = False
        msg = (f"reset_under_act: {k} act rows were taken before their episode reset had finished (by vector step {step}): the reset launch does not run beside the act "
               "kernel on this device -- episode resets go in front of the act kernel from here on (mn_reset_done)")
        (self.log or (lambda m: print(m, file=sys.stderr, flush=True)))(msg)

    def after_step(self, i):
        if not self.active:
            return
        from .fused_act import late_timeouts, late_timeouts_peek
        if i < self.preflight:
            if i == 1 or i == self.preflight - 1:
                self.env.join_reset()
                k = late_timeouts(self.agent.qnetwork_local) - self._seen0      # (synchronises: twice per loop)
                if k > 0:
                    return self._fall_back(i, k)
                if i == self.preflight - 1:
                    self._end_preflight()
        elif self.poll_every > 0 and (i - self.preflight) % self.poll_every == self.poll_every - 1:
            k = late_timeouts_peek(self.agent.qnetwork_local) - self._seen0
            if k > 0:
                self._fall_back(i, k)

    def close(self):
        self._end_preflight()

    def state_dict(self):
        """The verdict so far: still watching or not, the fallback if there was one, and the env threshold the end of the preflight restores (None behind it)."""
        return dict(active=bool(self.active), fallback=None if self.fallback is None else dict(self.fallback), restore=self._restore,
                    reset_under_act=bool(self.agent.reset_under_act), reset_fallback=bool(self.agent.reset_fallback))

    def load_state_dict(self, sd):
        """Into the guard of a fresh loop whose env has ALREADY been given its saved state (the handle's threshold came with it): the resumed loop neither
        repeats a preflight that has ended nor forgets a fallback.  The late-row time-outs of the saving process are not carried: this process's act context
        counts its own from zero, and a loop that fell back no longer looks at them."""
        self.active, self.fallback, self._restore = bool(sd["active"]), None if sd["fallback"] is None else dict(sd["fallback"]), sd["restore"]
        self.agent.reset_under_act, self.agent.reset_fallback = bool(sd["reset_under_act"]), bool(sd["reset_fallback"])


def evaluation_from_traces(reward, done, info, action, discount, energy_tab, dt, N):
    """The evaluation lists of IQNAgent.evaluation_vec from the traces (numpy [T][n]) of its episodes, whichever way they were produced:
    `episodes.tally`'s numbers as (action_data, reward_data, success_data, time_data, energy_data)."""
    tl = tally(reward, done, info, action, discount, energy_tab)
    return (tl["actions"], [float(x) for x in tl["ret"]], [bool(x) for x in (tl["last_info"] == 4)], [float(dt * N * l) for l in tl["length"]],
            [float(x) for x in tl["energy"]])


VecStepState = namedtuple("VecStepState", "obs reward done info due under_act eps fallback", defaults=(None, False))      # IQNAgent.vec_collect -> vec_finish


class VecLoop:
    """`IQNAgent.learn_vec`'s loop in the parts a driver can interleave with other agents' (train_iqn.run_trials_together): per vector step `collect(it)` (act,
    step + append, resets in front; returns the cadence's tick), the gradient steps the tick asks for -- the caller's: the agent's own
    `train_steps_from_memory(grad_steps_per_update)` or a `LearnerGroup` for all agents at once -- and `finish(it, loss)` (target copy, resets under the next
    act, counters, guard, episode log, evaluation points, hook); `end()` behind the last step, `close()` in any case.  `learn_vec` is this loop for one agent."""

    def __init__(self, agent, total_vector_steps, train_env, eval_env=None, eval_config=None, eval_freq=None, eval_log_path=None, total_timesteps=None,
                 world_size=1, cvar=1.0, verbose=True, train_every=None, on_step=None, report_timestep_scale=1.0, eval_adaptive=True, reset_under_act=True,
                 eval_one_launch=False, eval_deferred=False, episode_log=None, eval_points=None, max_eval_steps=1000):
        self.agent, self.train_env, self.eval_env, self.eval_config = agent, train_env, eval_env, eval_config
        self.eval_freq, self.eval_log_path, self.cvar, self.verbose, self.on_step = eval_freq, eval_log_path, cvar, verbose, on_step
        self.eval_adaptive, self.eval_one_launch, self.episode_log, self.eval_points, self.max_eval_steps = eval_adaptive, eval_one_launch, episode_log, eval_points, max_eval_steps
        n = train_env.n_envs
        self.per_iter = n * world_size
        # evaluation npz `timesteps` are reported as current_timestep * report_timestep_scale (train_iqn: reference-
        # equivalent timesteps, so scripts/plot_eval_returns.py keeps its x axis)
        agent._report_scale = float(report_timestep_scale)
        self.total_timesteps = total_vector_steps * self.per_iter if total_timesteps is None else total_timesteps
        self.train_every = agent.UPDATE_EVERY if train_every is None else train_every
        self.obs = train_env.reset()
        self.ep_ret = torch.zeros(n, device=agent.device)
        self.ep_len = torch.zeros(n, device=agent.device)
        self.stats = dict(episodes=0, successes=0, collisions=0, timeouts=0, loss=None)
        # this loop never looks at `obs` between two vector steps, so the resets can run under the next step's act kernel (see `reset_under_act`) -- checked on this
        # device by the loop's first steps (UnderActGuard: falls back to resets in front with one log line if the reset launch does not run beside the act kernel)
        self.was_under_act, agent.reset_under_act = agent.reset_under_act, bool(reset_under_act)
        self.guard = UnderActGuard(agent, train_env)
        agent.under_act_fallback = None
        self.deferred = (agent._deferred_evaluations(eval_deferred, eval_env, eval_config, eval_adaptive, eval_log_path)
                         if eval_deferred and eval_env is not None else None)
        self._state = self._eps = None
        self._points, self._evaluate_now = (), False

    def eps_now(self):
        """The exploration rate of the vector step that comes next."""
        return self.agent.linear_eps(self.total_timesteps)

    def _begin(self, it):
        """What a vector step settles before it collects: its exploration rate and its evaluation points."""
        agent = self.agent
        self._eps = eps = self.eps_now()
        if self.eval_points is None:
            self._evaluate_now = self.eval_env is not None and cadence_tick(agent, self.train_every, self.eval_freq).evaluate      # (the state vec_collect's own tick sees)
            self._points = (None,) if self._evaluate_now else ()
        else:
            self._points = tuple(self.eval_points.get(it, ()))
            self._evaluate_now = self.eval_env is not None and len(self._points) > 0
        return eps

    def collect(self, it):
        eps = self._begin(it)
        self._state = self.agent.vec_collect(self.train_env, self.obs, eps, self.cvar, self.train_every)
        return self._state.due

    def collect_given(self, it, obs, reward, done, info):
        """`collect` for a vector step whose collect phase was done for this agent (iqn/group_collect.py: the act at `eps_now()`, the env step, the append
        to this agent's ring -- `memory.advance` included -- and the resets in front, all on a stacked env): `obs` = this agent's rows for the next act,
        `reward`, `done`, `info` = its rows of the step's outputs.  Calls neither `act_batch` nor the env; returns the cadence's tick as `collect` does."""
        self._begin(it)
        due = cadence_tick(self.agent, self.train_every)      # (behind the append, as vec_collect asks it)
        self._state = VecStepState(obs, reward, done, info, due, False)
        return due

    def finish(self, it, loss=None):
        agent, train_env, stats, episode_log, points, eps = self.agent, self.train_env, self.stats, self.episode_log, self._points, self._eps
        st = self._state
        self.obs = agent.vec_finish(train_env, st, self.per_iter)
        reward, done, info = st.reward, st.done, st.info
        self.guard.after_step(it)
        if loss is not None:
            stats["loss"] = loss
        if episode_log is not None:
            episode_log.step(reward, done, info, it, eps)
            if len(points):      # a summary row per evaluation interval, the evaluation's timestep on it
                episode_log.drain(int(round(agent.current_timestep * agent._report_scale)) if points[-1] is None else points[-1])
            elif episode_log.due():
                episode_log.drain(int(round(agent.current_timestep * agent._report_scale)), row=False)
        if self.on_step is not None:
            stats["last"] = dict(reward=reward, done=done, info=info, eps=eps)
        if self.verbose:
            self.ep_ret += (train_env.discount ** self.ep_len) * reward
            self.ep_len += 1
            d = done.bool()
            stats["episodes"] += int(d.sum())
            stats["successes"] += int((info == 4).sum())
            stats["collisions"] += int((info == 3).sum())
            stats["timeouts"] += int((info == 2).sum())
            self.ep_ret.masked_fill_(d, 0.0); self.ep_len.masked_fill_(d, 0.0)
        for point in (points if self._evaluate_now else ()):
            if self.deferred is not None:
                self.deferred.snapshot(vector_step=it, timestep=point)
            else:
                agent._evaluate_inline(it, point, self.eval_env, self.eval_config, self.eval_log_path, self.eval_adaptive, self.eval_one_launch, self.max_eval_steps)
        if self.on_step is not None:
            self.on_step(it, stats)

    def end(self):
        agent, episode_log = self.agent, self.episode_log
        if self.deferred is not None:
            self.deferred.flush()
        if episode_log is not None:
            if episode_log.row_open:      # (what ended behind the last evaluation point)
                episode_log.drain(int(round(agent.current_timestep * agent._report_scale)))
            episode_log.close()
        # the end-of-run look at the bounded waits happens while `reset_under_act` still says how this loop ran (every rank, evaluation env or not)
        if hasattr(self.train_env, "join_reset"):
            self.train_env.join_reset()
        agent.check_learner()

    def close(self):
        agent = self.agent
        if self.deferred is not None:
            self.deferred.close()
        self.guard.close()
        agent.under_act_fallback = self.guard.fallback
        agent.reset_under_act = self.was_under_act
        agent.reset_fallback = False
        if hasattr(self.train_env, "join_reset"):
            self.train_env.join_reset()

    # ---- checkpoints ---------------------------------------------------------------------------
    def state_dict(self, next_step):
        """The loop's own state behind a finished vector step (`next_step` = the index of the step that comes next): the observations the next act reads, the
        verbose accumulators, `stats`, the guard's verdict, and the state of the deferred evaluations (flushed first) and of the episode log.  The agent, its
        ring and the envs have their own `state_dict()`; train_iqn's checkpoint holds them side by side."""
        if hasattr(self.train_env, "join_reset"):      # (rows of `obs` may still await their reset: an owed one is launched here, one under the act kernel joined)
            self.train_env.join_reset()
        stats = {k: (v.detach().cpu() if torch.is_tensor(v) else v) for k, v in self.stats.items() if k != "last"}
        return dict(next_step=int(next_step), obs=self.obs.cpu(), ep_ret=self.ep_ret.cpu(), ep_len=self.ep_len.cpu(), stats=stats, guard=self.guard.state_dict(),
                    deferred=None if self.deferred is None else self.deferred.state_dict(),
                    episode_log=None if self.episode_log is None else self.episode_log.state_dict())

    def load_state_dict(self, sd):
        """Into a fresh loop over the same arguments, AFTER the agent, its ring and the train env were given their states.  Returns the index of the vector
        step to continue with."""
        if (sd["deferred"] is None) != (self.deferred is None) or (sd["episode_log"] is None) != (self.episode_log is None):
            raise ValueError("VecLoop.load_state_dict: the saved loop and this one differ in their deferred evaluations or their episode log")
        self.obs = self.train_env.obs if hasattr(self.train_env, "obs") else self.obs
        self.obs.copy_(sd["obs"])
        self.ep_ret.copy_(sd["ep_ret"]); self.ep_len.copy_(sd["ep_len"])
        self.stats = {k: (v.to(self.agent.device) if torch.is_tensor(v) else v) for k, v in sd["stats"].items()}
        self.guard.load_state_dict(sd["guard"])
        if self.deferred is not None:
            self.deferred.load_state_dict(sd["deferred"])
        if self.episode_log is not None:
            self.episode_log.load_state_dict(sd["episode_log"])
        return int(sd["next_step"])


class IQNAgent(ReferenceLoopMixin):
    def __init__(self, state_size, action_size, layer_size=64, n_step=1, BATCH_SIZE=32, BUFFER_SIZE=1_000_000,
                 LR=1e-4, TAU=1.0, GAMMA=0.99, UPDATE_EVERY=4, learning_starts=10000, target_update_interval=10000,
                 exploration_fraction=0.1, initial_eps=1.0, final_eps=0.05, device="cpu", seed=0,
                 distributed=False, act_chunk=8192, rank=0, n_step_mode="reference", per=False, per_alpha=0.6, per_beta0=0.4,
                 per_eps=1e-6, munchausen=False, m_alpha=0.9, m_tau=0.03, m_clip=-1.0, target_rule="max"):
        self.state_size = state_size
        self.action_size = action_size
        self.device = torch.device(device)
        self.LR, self.TAU, self.GAMMA = LR, TAU, GAMMA
        self.UPDATE_EVERY = UPDATE_EVERY
        self.BATCH_SIZE = BATCH_SIZE
        self.n_step = n_step
        self.n_step_mode = n_step_mode               # n_step > 1: "reference" (the reference's window, sliding across episode ends) or "episode" (cut at the first done): replay_buffer.py
        # proportional prioritized replay (opt-in; iqn/priority.py; include/marinenav_hip.h, "Prioritized replay"): rows are drawn in proportion to
        # (mean |TD error| + per_eps) ** per_alpha, the loss is weighted by (size * P(row)) ** -beta over the batch's largest, beta linear from per_beta0 to 1
        # over `per_beta_steps` gradient steps (None, the default, also under `learn_vec` called directly: constant per_beta0; train_iqn sets the number of gradient steps its plan will take)
        self.per, self.per_alpha, self.per_beta0, self.per_eps = bool(per), float(per_alpha), float(per_beta0), float(per_eps)
        self.per_beta_steps = None
        self._per_step = 0                           # beta's position: prioritized gradient steps so far
        if self.per and distributed:
            raise ValueError("prioritized replay (per=True) keeps one learner's priorities next to its own ring; a shared learner (distributed=True), whose ranks "
                             "average gradients of differently weighted batches, is refused")
        # the Munchausen target (opt-in; Vieillard et al. 2020; include/marinenav_hip.h, "Munchausen target"): a soft-max policy over the target network's mean
        # quantiles (temperature m_tau) replaces the hard max, its entropy enters the target, and m_alpha x the log-policy of the action taken, clipped to
        # [m_clip, 0], is added to the reward.  Defaults: the paper's
        self.munchausen, self.m_alpha, self.m_tau, self.m_clip = bool(munchausen), float(m_alpha), float(m_tau), float(m_clip)
        if self.munchausen:
            if not (math.isfinite(self.m_tau) and self.m_tau > 0 and self.m_clip <= 0 and math.isfinite(self.m_alpha) and self.m_alpha >= 0):
                raise ValueError(f"munchausen=True needs m_tau > 0, m_clip <= 0 and m_alpha >= 0 (got m_tau {m_tau!r}, m_clip {m_clip!r}, m_alpha {m_alpha!r})")
            if distributed:
                raise ValueError("munchausen=True: the Munchausen step runs on one learner's own launches; a shared learner (distributed=True), whose exchange rides "
                                 "in the plain step's launches, is refused")
            if self.per:
                raise ValueError("munchausen=True with per=True: the prioritized sampler emits two tau sets and the Munchausen step takes three; composing the two "
                                 "is refused")
        # which action the TD target bootstraps from (opt-in; include/marinenav_hip.h, "Target rules"): "max" -- the reference's max over actions PER quantile sample
        # (agent.py:281); "mean" -- the IQN paper's one greedy action per next state, the argmax of the target network's mean over its samples; "double" -- Double-IQN,
        # that argmax taken on the LOCAL network's quantiles of the next state (a tau set of its own), valued by the target network
        if target_rule not in ("max", "mean", "double"):
            raise ValueError(f"target_rule must be 'max', 'mean' or 'double', not {target_rule!r}")
        self.target_rule = target_rule
        if target_rule != "max":
            if self.munchausen:
                raise ValueError(f"target_rule={target_rule!r} with munchausen=True: the Munchausen target replaces the greedy choice by a soft-max policy; composing "
                                 "the two is refused")
            if self.per:
                raise ValueError(f"target_rule={target_rule!r} with per=True: the weighted step of prioritized replay has the per-sample max only; composing the two "
                                 "is refused")
            if distributed:
                raise ValueError(f"target_rule={target_rule!r}: the greedy-on-mean step runs on one learner's own launches; a shared learner (distributed=True), "
                                 "whose exchange rides in the plain step's launches, is refused")
        self.learning_starts = learning_starts
        self.target_update_interval = target_update_interval
        self.exploration_fraction = exploration_fraction
        self.initial_eps, self.final_eps = initial_eps, final_eps
        self.N = 8                                   # train-time quantile samples (agent.py:286,290)
        self.rank = int(rank)                        # shared learner: same `seed` (identical init) on every rank, but
                                                     # rank-specific exploration / tau / replay-sampling streams
        self.act_chunk = act_chunk
        self.grad_steps_per_update = 1               # vectorised loop only: grad steps per training event
        self.use_fused_act = True                    # GPU tensors: fused HIP act kernel (csrc/iqn_act.hip)
        self._act_rng = None                         # the act path's own counter-based tau / exploration draws (fused_act.ActRng)
        self.use_library_rng = True                  # False: taus / exploration uniforms from torch.rand on self.gen
        self.shared_taus = False                     # opt-in: one set of 32 taus per act LAUNCH instead of per row (fused_act(shared_taus=True))
        self.act_greedy_rows_only = True             # act_batch: the network runs only on the rows that do not explore (fused_act(greedy_rows=...)); False: on every row, same actions
        self.use_fused_graph = False                 # opt-in: the fused gradient steps of one training event as one captured hipGraph (train_steps_from_memory)
        self.reset_under_act = False                 # vec_step: the episode resets of a vector step run on the env's own stream UNDER the next step's act kernel (which takes
                                                     # the finished envs' rows last) instead of in front of it: same results, ~28 us off every vector step's critical path.  The
                                                     # `obs` vec_step returns then has rows still being written: hand it back to vec_step, or call `train_env.join_reset()` before
                                                     # reading it.  On in learn_vec / train_iqn / bench.py; off by default for callers that look at `obs` between steps
        self.use_train_graph = False                 # opt-in: grad step replayed from a captured hipGraph (measured: no gain, the step is bound by kernel time, not launches)
        self.reset_fallback = False                  # UnderActGuard went back to resets in front: vec_step then offers them to the next act call's preparation launch (mn_reset_done_next_act, fallback)
        self._late_acknowledged = 0                  # late-row time-outs of the act context that a loop has already answered by going back to resets in front (UnderActGuard)
        self.under_act_fallback = None               # learn_vec: dict(step, timeouts) if that happened in the last loop
        self._graph = None
        self._graph_bypass_logged = False
        # GPU: the whole optimizer step as five HIP kernels (csrc/iqn_train.hip: sample, forward+backward, reduce, norm,
        # Adam) instead of ~150 PyTorch autograd / Adam kernels; False = the PyTorch path (always used on the CPU)
        self.use_fused_train = torch.device(device).type == "cuda"
        self._fused = None

        self.qnetwork_local = ObsEncoder(state_size, action_size, seed, device)
        self.qnetwork_target = ObsEncoder(state_size, action_size, seed, device)   # identical init (App. A A1)
        self.optimizer = self._make_adam()
        self.memory = ReplayBuffer(BUFFER_SIZE, BATCH_SIZE, device, seed, GAMMA, n_step, state_size, nstep_mode=n_step_mode, prioritized=self.per)
        random.seed(seed)                            # replay_buffer.py:21 seeds python `random` (eps-greedy)
        self.gen = torch.Generator(device=self.device)
        self.gen.manual_seed(int(seed) + 12345 + 7919 * self.rank)
        if self.rank:
            self.memory.gen.manual_seed(int(seed) + 104729 * self.rank)
        self.target_sync_grad_steps = None           # vectorised loop: hard target copy every this many grad steps
                                                     # (None: every target_update_interval vector steps, see vec_step)
        self._last_sync_at = 0
        self._train_path = None                      # "hip" / "torch": which gradient step ran last (Adam step-count hand-over)

        self.current_timestep = 0
        self.learning_timestep = 0
        self.grad_steps = 0
        self.distributed = bool(distributed)
        self.exchange = "collective"                 # shared learner: "collective" = RCCL all-reduce of the flat gradient (default); "mailbox" =
                                                     # one-shot exchange over IPC-mapped mailboxes (iqn/mailbox.py; opt-in)
        self._flat = None

        self.eval_timesteps = dict(greedy=[], adaptive=[])
        self.eval_actions = dict(greedy=[], adaptive=[])
        self.eval_rewards = dict(greedy=[], adaptive=[])
        self.eval_successes = dict(greedy=[], adaptive=[])
        self.eval_times = dict(greedy=[], adaptive=[])
        self.eval_energies = dict(greedy=[], adaptive=[])
        self.best_eval = None                        # learn_vec: the best greedy evaluation so far (successes, mean return) and when

    def _make_adam(self):
        """Adam(lr=1e-4) as agent.py:66; on the GPU the fused single-kernel implementation (same update rule)."""
        fused = torch.device(self.device).type == "cuda" and os.environ.get("MN_FUSED_ADAM", "1") == "1"
        return optim.Adam(self.qnetwork_local.parameters(), lr=self.LR, fused=fused) if fused else \
            optim.Adam(self.qnetwork_local.parameters(), lr=self.LR)

    # ---- checkpoints ---------------------------------------------------------------------------
    def load_model(self, path, device="cpu"):
        """agent.py:86-92."""
        self.qnetwork_local = ObsEncoder.load(path, device)
        self.qnetwork_target = ObsEncoder.load(path, device)
        self.device = torch.device(device)
        self.optimizer = self._make_adam()
        self._train_path = None

    _COUNTERS = ("current_timestep", "learning_timestep", "grad_steps", "_last_sync_at")
    _EVAL_LISTS = ("eval_timesteps", "eval_actions", "eval_rewards", "eval_successes", "eval_times", "eval_energies")

    def _adam_state(self):
        """(exp_avg [P], exp_avg_sq [P], step) of the one Adam state both gradient-step paths update, from whichever path holds it: the fused step's flat
        buffers and device counter, or torch.optim.Adam's per-parameter state."""
        params = list(self.qnetwork_local.parameters())
        ft = self._fused if self._fused is not None and self._fused.owns(self) else None
        st0 = self.optimizer.state.get(params[0], None)
        opt_step = int(float(st0["step"])) if st0 is not None and "step" in st0 else 0
        if ft is not None:      # (the optimizer's moments are views of these)
            return ft.exp_avg.detach().cpu().clone(), ft.exp_avg_sq.detach().cpu().clone(), opt_step if self._train_path == "torch" else int(ft.step_dev.item())
        flat = lambda key: torch.cat([(self.optimizer.state[p][key] if key in self.optimizer.state.get(p, {}) else torch.zeros_like(p)).detach().reshape(-1).cpu()
                                      for p in params])
        return flat("exp_avg"), flat("exp_avg_sq"), opt_step

    def _load_adam_state(self, exp_avg, exp_avg_sq, step):
        """The reverse: into the fused trainer's buffers where this agent trains through it (the optimizer's views of them follow), and into the optimizer's
        own state in any case, step count included -- so whichever path runs next finds what the saving agent's path left (`_enter_train_path`)."""
        params = list(self.qnetwork_local.parameters())
        if self.use_fused_train and self.device.type == "cuda":
            ft = self._fused_trainer()
            ft.exp_avg.copy_(exp_avg); ft.exp_avg_sq.copy_(exp_avg_sq)
            ft.step_dev.fill_(int(step))
        opt = self.optimizer
        on_dev = any(g.get("fused") or g.get("capturable") for g in opt.param_groups)
        off = 0
        with torch.no_grad():
            for p in params:
                n = p.numel()
                st = opt.state[p]
                if "exp_avg" not in st:
                    st["exp_avg"], st["exp_avg_sq"] = torch.zeros_like(p), torch.zeros_like(p)
                if "step" not in st:
                    st["step"] = torch.zeros((), dtype=torch.float32, device=p.device if on_dev else "cpu")
                st["exp_avg"].copy_(exp_avg[off:off + n].view(p.shape)); st["exp_avg_sq"].copy_(exp_avg_sq[off:off + n].view(p.shape))
                st["step"].fill_(float(int(step)))
                off += n
        self._train_path = None      # both paths hold the same state now: nothing to hand over at the next step

    def state_dict(self):
        """Everything of the agent a continued run depends on, as CPU tensors and plain numbers (the replay ring has its own: `memory.state_dict()`): both
        networks, the Adam state of whichever gradient-step path holds it, the counters the cadences and the exploration schedule read, the evaluation
        record, the act stream's {seed, counter}, the gradient step's sampling state, and the generators the non-fused paths draw from (this agent's, torch's
        CPU and device generators, python's `random`).  Caches are not state: the act kernel's weight image, a staged next batch, captured graphs,
        the draw buffers and the workspaces are rebuilt by the next call that needs them."""
        import copy
        ft = self._fused if self._fused is not None and self._fused.owns(self) else None
        m, v, step = self._adam_state()
        cpu = lambda net: {k: t.detach().cpu().clone() for k, t in net.state_dict().items()}
        sd = dict(local=cpu(self.qnetwork_local), target=cpu(self.qnetwork_target), exp_avg=m, exp_avg_sq=v, adam_step=int(step),
                  counters={k: int(getattr(self, k)) for k in self._COUNTERS}, report_scale=float(getattr(self, "_report_scale", 1.0)),
                  eval_lists={k: copy.deepcopy(getattr(self, k)) for k in self._EVAL_LISTS}, best_eval=copy.deepcopy(self.best_eval),
                  act_rng=None if self._act_rng is None else self._act_rng.state.cpu(), train_rng=None if ft is None else ft.rng_state.cpu(),
                  gen=self.gen.get_state(), torch_cpu_rng=torch.get_rng_state(),
                  torch_device_rng=torch.cuda.get_rng_state(self.device) if self.device.type == "cuda" else None, py_random=random.getstate())
        if self.per:      # beta's position (the masses, mmax and the sampler's generator state are the ring's: memory.state_dict())
            sd["per"] = dict(step=int(self._per_step), beta_steps=self.per_beta_steps)
        return sd

    def load_state_dict(self, sd):
        """Continue where `state_dict()` was taken: bit-identical from here on, on either gradient-step path (a state saved by the fused HIP step loads into an
        agent that trains through PyTorch and the other way round -- the moments and the step count are handed over as `_enter_train_path` hands them)."""
        import copy
        with torch.no_grad():      # in place: the parameters may be views of the fused trainer's flat buffers
            for net, key in ((self.qnetwork_local, "local"), (self.qnetwork_target, "target")):
                own = net.state_dict()
                if own.keys() != sd[key].keys():
                    raise ValueError(f"IQNAgent.load_state_dict: the saved {key} network has other parameters ({sorted(set(own) ^ set(sd[key]))})")
                for k, t in own.items():
                    t.copy_(sd[key][k])
        self._load_adam_state(sd["exp_avg"], sd["exp_avg_sq"], sd["adam_step"])
        for k in self._COUNTERS:
            setattr(self, k, int(sd["counters"][k]))
        self._report_scale = float(sd["report_scale"])
        for k in self._EVAL_LISTS:
            setattr(self, k, copy.deepcopy(sd["eval_lists"][k]))
        self.best_eval = copy.deepcopy(sd["best_eval"])
        if self.per and sd.get("per") is not None:      # (absent: a state written without prioritized replay -- beta starts over)
            self._per_step = int(sd["per"]["step"])
            self.per_beta_steps = sd["per"]["beta_steps"]
        if sd["act_rng"] is not None:
            if self._act_rng is None:
                from .fused_act import ActRng
                self._act_rng = ActRng(self.gen.initial_seed(), self.device)
            self._act_rng.state.copy_(sd["act_rng"])
        else:
            self._act_rng = None
        ft = self._fused if self._fused is not None and self._fused.owns(self) else None
        if sd["train_rng"] is not None and ft is None and self.use_fused_train and self.device.type == "cuda":
            ft = self._fused_trainer()
        if ft is not None:
            if sd["train_rng"] is not None:
                ft.rng_state.copy_(sd["train_rng"])
            ft._staged_key = None      # caches: the next call rebuilds them (the staged and the unstaged step, a rebuilt image: the same bits)
            ft._graph, ft._graph_key = None, None
        self._graph = None
        self.gen.set_state(sd["gen"])
        torch.set_rng_state(sd["torch_cpu_rng"])
        if sd["torch_device_rng"] is not None and self.device.type == "cuda":
            torch.cuda.set_rng_state(sd["torch_device_rng"], self.device)
        random.setstate(sd["py_random"])
        if self.device.type == "cuda":
            from .fused_act import weights_changed
            weights_changed(self.qnetwork_local)      # (the copies above went through PyTorch, which the act context tracks; this costs one re-pack)

    def adjust_cvar_batch(self, states):
        """Batched adjust_cvar on device: states [n, 26] -> cvar [n]."""
        p = states[:, 4:].view(states.shape[0], -1, 2)
        skip = (p[:, :, 0].abs() < 1e-3) & (p[:, :, 1].abs() < 1e-3)
        if states.is_cuda:
            d = torch.linalg.vector_norm(p, dim=2)
        else:
            # on the CPU vector_norm rounds x^2 + y^2 once; written out, the norm is the device's (and adjust_cvar_row's, csrc/mn_rollout_iqn_body.h):
            # the two squares rounded separately, their sum, a correctly rounded root
            sq = p * p
            d = (sq[:, :, 0] + sq[:, :, 1]).sqrt()
        d = d.masked_fill(skip, float("inf"))
        closest = d.min(dim=1).values
        return torch.where(closest < 10.0, closest / 10.0, torch.ones_like(closest))

    # ---- acting --------------------------------------------------------------------------------
    @torch.no_grad()
    def act_eval_batch(self, states, eps=0.0, cvar=1.0, taus=None):
        """Batched act_eval (agent.py:217-236): states [n,26] on the device -> (actions [n] i32, quantiles [n,32,9],
        taus [n,32,1]) -- the per-action return distribution samples and the (cvar-scaled) quantile fractions they
        were evaluated at, as run_experiments.py:26-69 records them.  `cvar` is a float or a per-row tensor."""
        if states.is_cuda and self.use_fused_act:
            from .fused_act import fused_act, ActRng
            if taus is None and self.use_library_rng:
                if self._act_rng is None:
                    self._act_rng = ActRng(self.gen.initial_seed(), states.device)
                return fused_act(self.qnetwork_local, states.contiguous(), eps, cvar, rng=self._act_rng, want_quantiles=True,
                                 shared_taus=self.shared_taus)
            return fused_act(self.qnetwork_local, states.contiguous(), eps, cvar, taus=taus, generator=self.gen,
                             want_quantiles=True, shared_taus=self.shared_taus and (taus is None or taus.numel() == self.qnetwork_local.K))
        quantiles, t = self.qnetwork_local.forward(states, self.qnetwork_local.K, cvar, taus=taus)
        greedy = quantiles.mean(dim=1).argmax(dim=1).to(torch.int32)
        if eps > 0.0:
            n = states.shape[0]
            u = torch.rand(n, device=states.device, generator=self.gen)
            rnd = torch.randint(0, self.action_size, (n,), device=states.device, dtype=torch.int32, generator=self.gen)
            greedy = torch.where(u > eps, greedy, rnd)
        return greedy, quantiles, t

    @torch.no_grad()
    def qvals_batch(self, states, cvar=1.0, taus=None):
        """Q(s, .) = mean over K = 32 quantile samples, for a whole vector of states (device tensor).
        On the GPU this is the fused HIP kernel (csrc/iqn_act.hip); on CPU tensors (tests) plain PyTorch,
        chunked over envs."""
        if states.is_cuda and self.use_fused_act:
            from .fused_act import fused_qvals
            return fused_qvals(self.qnetwork_local, states, cvar, taus=taus, generator=self.gen)
        n = states.shape[0]
        out = torch.empty(n, self.action_size, dtype=torch.float32, device=states.device)
        step = self.act_chunk
        for lo in range(0, n, step):
            hi = min(n, lo + step)
            c = cvar[lo:hi] if torch.is_tensor(cvar) else cvar
            t = taus[lo:hi] if taus is not None else None
            out[lo:hi] = self.qnetwork_local.get_qvals(states[lo:hi], c, taus=t)
        return out

    @torch.no_grad()
    def act_batch(self, states, eps, cvar=1.0, late_env=None):
        """Batched eps-greedy act (agent.py:186-205 per row): states [n,26] f32 on device ->
        actions [n] int32 on device.  On the GPU this is ONE fused HIP kernel (network, mean over taus,
        argmax, exploration); exploration draws come from a device generator.
        `late_env`: the env whose `reset_done(under_next_act=True)` may still be writing rows of `states` (vec_step with `reset_under_act`):
        the fused kernel takes those rows last; every other path waits for the reset first."""
        if states.is_cuda and self.use_fused_act:
            from .fused_act import fused_act
            if not self.use_library_rng:
                return fused_act(self.qnetwork_local, states.contiguous(), eps, cvar, generator=self.gen, shared_taus=self.shared_taus, late_env=late_env,
                                 greedy_rows=self.act_greedy_rows_only)
            if self._act_rng is None:
                from .fused_act import ActRng
                self._act_rng = ActRng(self.gen.initial_seed(), states.device)
            return fused_act(self.qnetwork_local, states.contiguous(), eps, cvar, rng=self._act_rng, shared_taus=self.shared_taus, late_env=late_env,
                             greedy_rows=self.act_greedy_rows_only)
        if late_env is not None:
            late_env.join_reset()
        q = self.qvals_batch(states, cvar)
        greedy = q.argmax(dim=1).to(torch.int32)
        if eps <= 0.0:
            return greedy
        n = states.shape[0]
        u = torch.rand(n, device=states.device, generator=self.gen)
        rnd = torch.randint(0, self.action_size, (n,), device=states.device, dtype=torch.int32, generator=self.gen)
        return torch.where(u > eps, greedy, rnd)

    # ---- learning ------------------------------------------------------------------------------
    def _allreduce_grads(self):
        import torch.distributed as dist
        params = [p for p in self.qnetwork_local.parameters() if p.grad is not None]
        grads = [p.grad for p in params]
        if self._flat is None or self._flat.numel() != sum(g.numel() for g in grads):
            self._flat = torch.empty(sum(g.numel() for g in grads), dtype=torch.float32, device=grads[0].device)
        torch.cat([g.reshape(-1) for g in grads], out=self._flat)
        dist.all_reduce(self._flat, op=dist.ReduceOp.SUM)       # one 143 KB bucket over RCCL/xGMI
        self._flat.div_(dist.get_world_size())
        off = 0
        for g in grads:
            g.copy_(self._flat[off:off + g.numel()].view_as(g))
            off += g.numel()

    def td_targets(self, experiences, taus_target=None, taus_munch=None, taus_select=None, want_select=False):
        """The TD targets Q_targets [B, 1, N] of `compute_loss`, without a graph.  Plain (agent.py:279-283): r + gamma^n (1 - done) max_a Z_target(s', tau_j)[a].
        With `munchausen` (include/marinenav_hip.h, "Munchausen target", states the rule operation by operation): the policy is the soft-max, at temperature
        m_tau, of the target network's MEAN over its N quantile samples; the target takes its expectation of Z' minus m_tau x its log, and the reward gains
        m_alpha x the log-policy of the action taken at the current state, clipped to [m_clip, 0] -- from a second forward of the TARGET network, over `states`
        with a tau set of its own (`taus_munch`).  The target network's calls run in that order: next states, then states.
        With `target_rule` "mean" / "double" (include/marinenav_hip.h, "Target rules"): one action a* per next state -- the FIRST argmax of the mean over the N
        samples of the target network's quantiles ("mean") or of the LOCAL network's quantiles of the next states under `taus_select` ("double"; called after the
        target network, without a graph) -- and every sample bootstraps from Z'[j][a*].  `want_select`: return (Q_targets, a* [B] i64)."""
        states, actions, rewards, next_states, dones = experiences
        with torch.no_grad():
            Q_targets_next, _ = self.qnetwork_target(next_states, self.N, taus=taus_target)
            if self.target_rule != "max":
                Zs = Q_targets_next
                if self.target_rule == "double":
                    Zs, _ = self.qnetwork_local(next_states, self.N, taus=taus_select)
                s = Zs[:, 0]
                for j in range(1, self.N):      # (the sum in index order, as the kernel takes it)
                    s = s + Zs[:, j]
                q = (1.0 / self.N) * s                                                                    # (B, A)
                a_star = first_argmax(q)                                                                # (B,)
                Q_sel = Q_targets_next.gather(2, a_star.view(-1, 1, 1).expand(-1, self.N, 1)).squeeze(2).unsqueeze(1)      # (B, 1, N)
                y = rewards.unsqueeze(-1) + (self.GAMMA ** self.n_step * Q_sel * (1. - dones.unsqueeze(-1)))
                return (y, a_star) if want_select else y
            if not self.munchausen:
                Q_targets_next = Q_targets_next.max(2)[0].unsqueeze(1)                          # (B, 1, N)
                return rewards.unsqueeze(-1) + (self.GAMMA ** self.n_step * Q_targets_next * (1. - dones.unsqueeze(-1)))
            te = self.m_tau
            q_next = Q_targets_next.mean(dim=1) / te                                                       # (B, A)
            tlp_next, pi_next = te * torch.log_softmax(q_next, dim=1), torch.softmax(q_next, dim=1)         # te log pi', pi'
            V = (pi_next.unsqueeze(1) * (Q_targets_next - tlp_next.unsqueeze(1))).sum(2).unsqueeze(1)       # (B, 1, N)
            Q_now, _ = self.qnetwork_target(states, self.N, taus=taus_munch)
            tlp = te * torch.log_softmax(Q_now.mean(dim=1) / te, dim=1)
            bonus = self.m_alpha * tlp.gather(1, actions).clamp(min=self.m_clip, max=0.0)                  # (B, 1)
            return (rewards + bonus).unsqueeze(-1) + (self.GAMMA ** self.n_step * V * (1. - dones.unsqueeze(-1)))

    def compute_loss(self, experiences, taus_target=None, taus_local=None, weights=None, want_abs_td=False, taus_munch=None, want_targets=False, taus_select=None):
        """Quantile-Huber TD loss of agent.py:276-295 (taus can be injected for tests).  `weights` [B]: element b's terms scaled by weights[b] (prioritized
        replay's importance weights; ones give the unweighted loss bit for bit).  `want_abs_td`: return (loss, mean |TD error| per element [B], detached) --
        the elements' new priorities.  `taus_munch`: the third tau set of the Munchausen target (`td_targets`); `want_targets`: return (loss, Q_targets [B, N]).  `taus_select`: the third tau set of
        `target_rule="double"`."""
        states, actions, rewards, next_states, dones = experiences
        B = states.shape[0]
        Q_targets = self.td_targets(experiences, taus_target, taus_munch, taus_select)
        Q_expected, taus = self.qnetwork_local(states, self.N, taus=taus_local)
        Q_expected = Q_expected.gather(2, actions.unsqueeze(-1).expand(B, self.N, 1))
        # td_error[b, i, j] = Q_targets[b, 0, j] - Q_expected[b, i, 0]   (B, N, N); Huber with kappa = 1
        # (agent.py:401-407) as ONE fused op with its own backward instead of abs / le / pow / where chains
        qt, qe = Q_targets.expand(B, self.N, self.N), Q_expected.expand(B, self.N, self.N)
        huber_l = torch.nn.functional.huber_loss(qe, qt, reduction="none", delta=1.0)
        with torch.no_grad():
            weight = (taus - (qt < qe).to(taus.dtype)).abs()      # |tau - 1[td < 0]|, agent.py:293
        # sum over the local-quantile axis, mean over the target-sample axis, mean over the batch (agent.py:294-295)
        terms = weight * huber_l
        if weights is not None:
            terms = terms * weights.to(terms.dtype).view(B, 1, 1)
        loss = terms.sum() / (B * self.N)
        if want_abs_td:
            return loss, (qt - qe).detach().abs().mean(dim=(1, 2))
        if want_targets:
            return loss, Q_targets.view(B, self.N)
        return loss

    def _fused_trainer(self):
        from .fused_train import FusedTrainer
        if self._fused is None or not self._fused.owns(self):      # load_model() replaces the networks
            self._fused = FusedTrainer(self)
        return self._fused

    def _enter_train_path(self, path):
        """Both gradient-step paths update ONE Adam state (the moments are shared memory, iqn/fused_train.py); the step
        count is handed over whenever the path changes, so flipping `use_fused_train` mid-run continues the same
        optimizer instead of restarting its bias correction."""
        if self._train_path == path:
            return
        if self._fused is not None and self._fused.owns(self):
            if path == "torch" and self._train_path == "hip":
                self._fused.sync_to_optimizer(self.optimizer)
            elif path == "hip" and self._train_path == "torch":
                self._fused.sync_from_optimizer(self.optimizer)
        self._train_path = path

    def train_steps_from_memory(self, n_steps):
        """`n_steps` x train_from_memory().  With `use_fused_graph` (GPU, fused gradient step) the whole sequence -- every step's
        forward / backward, reduction, RCCL all-reduce of a shared learner, Adam -- is ONE hipGraph launch (iqn/fused_train.py:
        graphed_steps): the host enqueues one node instead of 3-4 launches per step, which is what a shared learner's 16 steps per
        vector step need to stay ahead of the GPU.  Same arithmetic, same generator stream: bit-identical to the eager calls."""
        # (while the ring is still filling its row count changes with every vector step and each change would be a re-capture +
        # device synchronisation: the eager steps -- bit-identical -- run until the ring is full)
        if self.munchausen and self.use_fused_graph:
            raise ValueError("munchausen=True: the Munchausen step samples three tau sets and steps in launches of its own; the captured graph of `use_fused_graph`, "
                             "which replays the plain step's in-launch draws, is refused")
        if self.target_rule != "max" and self.use_fused_graph:
            raise ValueError(f"target_rule={self.target_rule!r}: the greedy-on-mean step samples and steps in launches of its own; the captured graph of "
                             "`use_fused_graph`, which replays the plain step's in-launch draws, is refused")
        if self.per and self.use_fused_graph:
            raise ValueError("prioritized replay (per=True) samples, steps and updates priorities as separate launches per gradient step; the captured graph of "
                             "`use_fused_graph`, which replays in-launch uniform draws, is refused")
        want_graph = self.use_fused_graph and self.use_fused_train and self.device.type == "cuda" and n_steps > 1
        if want_graph and len(self.memory) < self.memory.capacity and not self._graph_bypass_logged:
            self._graph_bypass_logged = True
            print(f"[IQNAgent] use_fused_graph: eager gradient steps until the replay ring is full ({len(self.memory)} of {self.memory.capacity} rows)", flush=True)
        if want_graph and len(self.memory) >= self.BATCH_SIZE and len(self.memory) == self.memory.capacity:
            m = self.memory
            ft = self._fused_trainer()
            self._enter_train_path("hip")
            loss = ft.graphed_steps((m.states, m.actions, m.rewards, m.next_states, m.dones), m.size, self.BATCH_SIZE, n_steps)
            self.grad_steps += n_steps
            return loss
        loss = None
        for _ in range(n_steps):
            loss = self.train_from_memory()
        return loss

    def train_from_memory(self):
        """`self.train(self.memory.sample())` (agent.py:131-133).  With `use_fused_train` the HIP step gathers its batch
        straight from the device ring (no sampled copies).  With `per`: `_train_prioritized`."""
        if self.per:
            return self._train_prioritized()
        if self.munchausen and self.use_fused_train and self.device.type == "cuda":
            # one sampling launch (rows + three tau sets), the Munchausen forward / backward + reduction, clip + Adam
            m = self.memory
            ft = self._fused_trainer()
            self._enter_train_path("hip")
            idx, taus = ft.sample(m.size, self.BATCH_SIZE, tau_sets=3)
            loss = ft.step_munch((m.states, m.actions, m.rewards, m.next_states, m.dones), idx, taus[0], taus[1], taus[2])
            self.grad_steps += 1
            return loss
        if self.target_rule != "max" and self.use_fused_train and self.device.type == "cuda":
            # one sampling launch (rows + two tau sets, or three under "double"), the rule's forward / backward + reduction, clip + Adam
            m = self.memory
            ft = self._fused_trainer()
            self._enter_train_path("hip")
            double = self.target_rule == "double"
            idx, taus = ft.sample(m.size, self.BATCH_SIZE, tau_sets=3 if double else 2)
            loss = ft.step_rule((m.states, m.actions, m.rewards, m.next_states, m.dones), idx, taus[0], taus[2] if double else None, taus[1])
            self.grad_steps += 1
            return loss
        if self.use_fused_train and self.device.type == "cuda":
            m = self.memory
            ft = self._fused_trainer()
            self._enter_train_path("hip")
            # replay_buffer.py:47 + model.py:149 + agent.py:269-304: the batch is drawn inside the forward / backward launch
            loss = ft.step_sampled((m.states, m.actions, m.rewards, m.next_states, m.dones), m.size, self.BATCH_SIZE, m.version)
            self.grad_steps += 1
            return loss
        return self.train(self.memory.sample())

    def per_beta(self):
        """The importance exponent of the next prioritized gradient step."""
        from .priority import beta_at
        return beta_at(self.per_beta0, self._per_step, self.per_beta_steps)

    def _train_prioritized(self):
        """One gradient step of prioritized replay: sample (rows in proportion to their masses, importance weights, the step's taus) -> the weighted step --
        `FusedTrainer.step_per` (mn_iqn_train_grad_per + mn_iqn_train_adam), or autograd where `use_fused_train` is off and on the CPU -> the batch's mean
        |TD errors| become its rows' new masses.  On the GPU three small launches around the step's, nothing synchronises with the host."""
        m = self.memory
        idx, w, taus = m.priority.sample(m.size, self.BATCH_SIZE, self.per_beta())
        ring = (m.states, m.actions, m.rewards, m.next_states, m.dones)
        if self.use_fused_train and self.device.type == "cuda":
            ft = self._fused_trainer()
            self._enter_train_path("hip")
            loss, abs_td = ft.step_per(ring, idx, taus[0], taus[1], w)
        else:
            self._enter_train_path("torch")
            self.optimizer.zero_grad(set_to_none=False)
            loss, abs_td = self.compute_loss(tuple(t[idx] for t in ring), taus[0], taus[1], weights=w, want_abs_td=True)
            loss.backward()
            torch.nn.utils.clip_grad_norm_(self.qnetwork_local.parameters(), 0.5)
            self.optimizer.step()
            if self.device.type == "cuda":      # (as in `train`: the act path's cached weight image goes by a counter Adam(fused=True) does not bump)
                from .fused_act import weights_changed
                weights_changed(self.qnetwork_local)
            loss, abs_td = loss.detach(), abs_td.contiguous()
        m.priority.update(idx, abs_td, self.per_alpha, self.per_eps)
        self._per_step += 1
        self.grad_steps += 1
        return loss

    def train(self, experiences, taus_target=None, taus_local=None, taus_munch=None, taus_select=None):
        """agent.py:269-304: one optimizer step; returns the loss (device scalar tensor).
        GPU tensors with `use_fused_train` (the default on the GPU): the hand-written HIP step (csrc/iqn_train.hip:
        both forwards, quantile-Huber loss, backward, clip, Adam in four launches).  Otherwise PyTorch autograd +
        torch.optim.Adam -- the definition the HIP step is tested against and the only path on the CPU; with
        `use_train_graph` (opt-in, single learner, taus not injected) replayed from one captured hipGraph."""
        if self.munchausen and self.use_train_graph:
            raise ValueError("munchausen=True: `use_train_graph` captured the plain step's graph; the Munchausen target has no captured form and is refused")
        if self.munchausen and self.use_fused_train and experiences[0].is_cuda:
            exp = tuple(t.contiguous() for t in experiences)
            ft = self._fused_trainer()
            self._enter_train_path("hip")
            B = exp[0].shape[0]
            taus = torch.rand(3, B, self.N, device=self.device)      # model.py:149 per network call: target(s'), target(s), local(s)
            tt, tm, tl = (taus[k] if t is None else t.to(self.device, torch.float32).contiguous().view(B, self.N)
                          for k, t in enumerate((taus_target, taus_munch, taus_local)))
            loss = ft.step_munch(exp, torch.arange(B, dtype=torch.int64, device=self.device), tt, tm, tl)
            self.grad_steps += 1
            return loss
        if self.target_rule != "max" and self.use_train_graph:
            raise ValueError(f"target_rule={self.target_rule!r}: `use_train_graph` captured the plain step's graph; the greedy-on-mean targets have no captured form "
                             "and are refused")
        if self.target_rule != "max" and self.use_fused_train and experiences[0].is_cuda:
            exp = tuple(t.contiguous() for t in experiences)
            ft = self._fused_trainer()
            self._enter_train_path("hip")
            B = exp[0].shape[0]
            double = self.target_rule == "double"
            given = (taus_target, taus_select, taus_local) if double else (taus_target, taus_local)
            taus = torch.rand(len(given), B, self.N, device=self.device)      # model.py:149 per network call: target(s'), (double: local(s'),) local(s)
            sets = [taus[k] if t is None else t.to(self.device, torch.float32).contiguous().view(B, self.N) for k, t in enumerate(given)]
            loss = ft.step_rule(exp, torch.arange(B, dtype=torch.int64, device=self.device), sets[0], sets[1] if double else None, sets[-1])
            self.grad_steps += 1
            return loss
        if self.use_fused_train and experiences[0].is_cuda:
            exp = tuple(t.contiguous() for t in experiences)
            ft = self._fused_trainer()
            self._enter_train_path("hip")
            loss = ft.step(exp, None, taus_target, taus_local)
            self.grad_steps += 1
            return loss
        self._enter_train_path("torch")
        if (self.use_train_graph and experiences[0].is_cuda and not self.distributed
                and taus_target is None and taus_local is None and experiences[0].shape[0] == self.BATCH_SIZE):
            return self._train_graphed(experiences)
        self.optimizer.zero_grad(set_to_none=False)
        loss = self.compute_loss(experiences, taus_target, taus_local, taus_munch=taus_munch, taus_select=taus_select)
        loss.backward()
        if self.distributed:
            self._allreduce_grads()          # average first, then clip: same as one big-batch learner
        torch.nn.utils.clip_grad_norm_(self.qnetwork_local.parameters(), 0.5)
        self.optimizer.step()
        if experiences[0].is_cuda:
            # torch.optim.Adam(fused=True) writes the weights without bumping the parameters' version counters, which is what the act path's cached weight
            # image goes by (iqn/fused_act.py): it has to be told, or acting goes on with the weights of the last image
            from .fused_act import weights_changed
            weights_changed(self.qnetwork_local)
        self.grad_steps += 1
        return loss.detach()

    def _train_graphed(self, experiences):
        if self._graph is None:
            dev = experiences[0].device
            self._g_in = tuple(torch.empty_like(t) for t in experiences)
            for dst, src in zip(self._g_in, experiences):
                dst.copy_(src)
            # Adam must keep its step counter on the device to be capturable; same arithmetic
            state = self.optimizer.state_dict()
            self.optimizer = optim.Adam(self.qnetwork_local.parameters(), lr=self.LR, capturable=True)
            if state["state"]:
                for st in state["state"].values():
                    st["step"] = torch.as_tensor(st["step"], dtype=torch.float32, device=dev)
                self.optimizer.load_state_dict(state)
                for g_ in self.optimizer.param_groups:
                    g_["capturable"] = True
            side = torch.cuda.Stream(device=dev)
            side.wait_stream(torch.cuda.current_stream(dev))
            snap = [p.detach().clone() for p in self.qnetwork_local.parameters()]
            # the optimizer's moment tensors may be views of the fused trainer's flat buffers (one Adam state for both
            # paths, iqn/fused_train.py) and load_state_dict keeps the tensors it is given: snapshot the VALUES, the
            # warm-up steps below update them in place
            import copy
            opt_snap = {k: {kk: (vv.detach().clone() if torch.is_tensor(vv) else copy.deepcopy(vv)) for kk, vv in st.items()}
                        for k, st in state["state"].items()}
            with torch.cuda.stream(side):   # warm-up iterations on a side stream (allocations, lazy init)
                for _ in range(3):
                    self.optimizer.zero_grad(set_to_none=True)
                    self.compute_loss(self._g_in).backward()
                    torch.nn.utils.clip_grad_norm_(self.qnetwork_local.parameters(), 0.5)
                    self.optimizer.step()
            torch.cuda.current_stream(dev).wait_stream(side)
            # the warm-up must not count as training: restore weights and optimizer state (values copied back INTO the
            # tensors the optimizer holds, so moments shared with the fused trainer stay shared)
            with torch.no_grad():
                for p_, s_ in zip(self.qnetwork_local.parameters(), snap):
                    p_.copy_(s_)
                live = self.optimizer.state_dict()["state"]
                for k, st in opt_snap.items():
                    for kk, vv in st.items():
                        if torch.is_tensor(vv):
                            live[k][kk].copy_(vv)
                if not opt_snap:      # the optimizer had no state before the warm-up created it: zero what it made
                    for st in live.values():
                        for vv in st.values():
                            if torch.is_tensor(vv):
                                vv.zero_()
            if self._fused is not None and self._fused.owns(self):
                self._fused._adopt_optimizer_state(self.optimizer)     # re-attach the flat moment buffers to the new optimizer
            self._graph = torch.cuda.CUDAGraph()
            self.optimizer.zero_grad(set_to_none=True)
            with torch.cuda.graph(self._graph):
                loss = self.compute_loss(self._g_in)
                loss.backward()
                torch.nn.utils.clip_grad_norm_(self.qnetwork_local.parameters(), 0.5)
                self.optimizer.step()
                self._g_loss = loss.detach()
            # capture does not execute: weights / optimizer untouched so far
        for dst, src in zip(self._g_in, experiences):
            dst.copy_(src)
        self._graph.replay()
        # a graph replay writes the weights without bumping the parameters' version counters: the act path's cached
        # weight image (iqn/fused_act.py) has to be told (writes through `.data` / raw pointers need the same call)
        from .fused_act import weights_changed
        weights_changed(self.qnetwork_local)
        self.grad_steps += 1
        return self._g_loss

    def soft_update(self, local_model, target_model):
        """agent.py:307-317 (TAU = 1.0 -> hard copy)."""
        with torch.no_grad():
            ft = self._fused
            if (ft is not None and ft.owns(self) and local_model is self.qnetwork_local
                    and target_model is self.qnetwork_target):
                # both networks are views of two flat buffers (iqn/fused_train.py): one copy instead of 14
                if self.TAU == 1.0:
                    ft.target.copy_(ft.local)
                else:
                    ft.target.mul_(1.0 - self.TAU).add_(ft.local, alpha=self.TAU)
                return
            for tp, lp in zip(target_model.parameters(), local_model.parameters()):
                tp.data.copy_(self.TAU * lp.data + (1.0 - self.TAU) * tp.data)

    def _sync_target(self):
        """Target copy + the gradient-step mark the `target_sync_grad_steps` cadence counts from (iqn/cadence.py)."""
        self.soft_update(self.qnetwork_local, self.qnetwork_target)
        self._last_sync_at = self.grad_steps

    # ---- batched loop on the HIP vector env ----------------------------------------------------------
    def learn_vec(self, total_vector_steps, train_env, eval_env=None, eval_config=None, eval_freq=None,
                  eval_log_path=None, total_timesteps=None, world_size=1, cvar=1.0, verbose=True,
                  train_every=None, on_step=None, report_timestep_scale=1.0, eval_adaptive=True, reset_under_act=True, eval_one_launch=False,
                  eval_deferred=False, episode_log=None, eval_points=None, max_eval_steps=1000):
        """Vectorised agent.py:94-173.  One iteration = one vector step of `train_env` (n_envs env
        steps): act_batch -> mn_step -> replay.add_batch -> mn_reset_done -> (every UPDATE_EVERY vector
        steps) sample + train.  `current_timestep` counts env steps over all ranks, so eps, the
        learning_starts gate and the curriculum keep the reference's meaning of "timesteps";
        `learning_timestep` counts vector steps after learning_starts (UPDATE_EVERY,
        target_update_interval and eval_freq are applied to it).  `eval_one_launch`: the evaluations as one mn_rollout_iqn launch each
        (evaluation_vec(one_launch=True): the same results).  `eval_deferred` (True, or a dict of DeferredEvaluations arguments such as max_pending /
        max_steps): an evaluation point only KEEPS the policy of the moment (two device copies, no synchronisation); the episodes of all pending points run
        later as one mn_rollout_iqn_groups launch, each point on a tau stream of its own, and are logged as the inline form logs them
        (iqn/deferred_eval.py: what is on disk between flushes, and why the number of points then leaves the training run untouched).  Where that launch
        cannot reproduce the acting form (CPU, PyTorch acting, torch.rand taus, the exact-f32 variant, launch-shared taus) the points stay inline.
        `eval_points` ({vector step: [timesteps]}, train_iqn.plan_eval_points): evaluate after exactly these vector steps instead of on the `eval_freq`
        cadence and log each evaluation with the timestep given (the reference-budget plan: the reference's own evaluation timesteps, the final one
        included).  `max_eval_steps`: the step limit of an inline evaluation episode.
        `episode_log` (episode_log.EpisodeLog): the training episodes' record -- one more launch behind every vector step, drained (without a host
        look) at the evaluation points and wherever its arrays could fill up, closed at the end of the loop."""
        loop = VecLoop(self, total_vector_steps, train_env, eval_env=eval_env, eval_config=eval_config, eval_freq=eval_freq, eval_log_path=eval_log_path,
                       total_timesteps=total_timesteps, world_size=world_size, cvar=cvar, verbose=verbose, train_every=train_every, on_step=on_step,
                       report_timestep_scale=report_timestep_scale, eval_adaptive=eval_adaptive, reset_under_act=reset_under_act, eval_one_launch=eval_one_launch,
                       eval_deferred=eval_deferred, episode_log=episode_log, eval_points=eval_points, max_eval_steps=max_eval_steps)
        try:
            for it in range(total_vector_steps):
                due = loop.collect(it)
                loss = self.train_steps_from_memory(self.grad_steps_per_update) if due.train else None      # 1 = the reference's cadence (agent.py:129-133)
                loop.finish(it, loss)
            loop.end()
        finally:
            loop.close()
        return loop.stats

    def _evaluate_inline(self, it, timestep, eval_env, eval_config, eval_log_path, eval_adaptive, one_launch, max_steps):
        """An evaluation point of learn_vec, evaluated now: greedy and -- `eval_adaptive` -- adaptive, the `best_*` rule, the latest checkpoint.
        `timestep`: the timestep to log (None: now)."""
        self.check_learner()      # (a device synchronisation; the evaluation below is one anyway)
        res = self.evaluation_vec(eval_env, eval_config, greedy=True, eval_log_path=eval_log_path, one_launch=one_launch, max_steps=max_steps, timestep=timestep)
        if eval_adaptive:
            self.evaluation_vec(eval_env, eval_config, greedy=False, eval_log_path=eval_log_path, one_launch=one_launch, max_steps=max_steps, timestep=timestep)
        # agent.py:140-148 keeps the LATEST network at every evaluation point; the batched run also keeps the BEST greedy evaluation so far beside it
        # (`best_*`: ~1 run in 12 ends on a checkpoint far below its own best -- profiles/r05_learning_curve.txt)
        score = (int(sum(res["successes"])), float(np.mean(res["rewards"])))
        if self.best_eval is None or score > self.best_eval["score"]:
            self.best_eval = dict(score=score, timestep=self.eval_timesteps["greedy"][-1], grad_steps=self.grad_steps, vector_step=it)
            if eval_log_path is not None:
                self.qnetwork_local.save(eval_log_path, prefix="best_")
                with open(os.path.join(eval_log_path, "best_evaluation.json"), "w") as f:
                    json.dump(dict(successes=score[0], n_worlds=len(res["successes"]), mean_return=score[1], **{k: v for k, v in self.best_eval.items() if k != "score"}), f)
        if eval_log_path is not None:
            self.qnetwork_local.save(eval_log_path)

    def _deferred_evaluations(self, options, eval_env, eval_config, adaptive, eval_log_path):
        """learn_vec's DeferredEvaluations (iqn/deferred_eval.py), or None -- with one log line -- where the grouped launch has no twin of this agent's
        acting form.  `options`: True, or a dict of further DeferredEvaluations arguments."""
        from .fused_act import act_context
        ok = self.device.type == "cuda" and self.use_fused_act and self.use_library_rng and not self.shared_taus and hasattr(eval_env, "h")
        if ok and act_context(self.qnetwork_local).variant != 2:
            ok = False
        if not ok:
            print("[learn_vec] eval_deferred: the grouped episode launch does not reproduce this acting form; evaluating inline")
            return None
        from .deferred_eval import DeferredEvaluations
        kw = dict(options) if isinstance(options, dict) else {}
        return DeferredEvaluations(self, eval_config, adaptive=adaptive, eval_log_path=eval_log_path, precision=eval_env.precision, verbose=kw.pop("verbose", True), **kw)

    def check_learner(self):
        """Raise if a bounded wait of the fused gradient step ran out since the last look (`FusedTrainer.check_timeouts`): the step(s) concerned updated
        nothing, and with the mailbox exchange a peer's gradient did not arrive -- the ranks of a shared learner would drift apart silently otherwise."""
        if self._fused is not None and self._fused.owns(self):
            self._fused.check_timeouts()
        if self.reset_under_act and self.device.type == "cuda" and self.use_fused_act:
            from .fused_act import late_timeouts
            k = late_timeouts(self.qnetwork_local) - self._late_acknowledged
            if k > 0:
                raise RuntimeError(f"{k} act rows were taken before their episode reset had finished (mn_iqn_late_timeouts): the reset launch did not run beside the act kernel")

    def vec_step(self, train_env, obs, eps, cvar=1.0, train_every=None, per_iter=None):
        """One iteration of the vectorised loop: act_batch -> mn_step -> replay.add_batch ->
        mn_reset_done -> (cadence permitting) sample + train + target sync.  Everything is enqueued on
        the current HIP stream; nothing synchronises with the host.
        Returns (obs for the next act, reward, done, info, loss or None)."""
        st = self.vec_collect(train_env, obs, eps, cvar, train_every)
        loss = self.train_steps_from_memory(self.grad_steps_per_update) if st.due.train else None      # 1 = the reference's cadence (agent.py:129-133)
        obs = self.vec_finish(train_env, st, per_iter)
        return obs, st.reward, st.done, st.info, loss

    def vec_collect(self, train_env, obs, eps, cvar=1.0, train_every=None):
        """The part of `vec_step` in front of the gradient steps: act_batch -> mn_step + replay append -> the cadence's tick -> (resets in front: mn_reset_done).
        Returns a VecStepState; the caller performs the gradient steps `state.due.train` asks for -- `train_steps_from_memory(grad_steps_per_update)`, or a
        `LearnerGroup` for several agents in lockstep (iqn/group_train.py) -- and then calls `vec_finish`."""
        train_every = self.UPDATE_EVERY if train_every is None else train_every
        under_act = bool(self.reset_under_act) and obs.is_cuda and hasattr(train_env, "take_late_rows") and self.use_fused_act
        if under_act:      # only the default acting form takes late rows: with any other the reset stays in front (no cross-stream events for nothing)
            from .fused_act import late_rows_possible
            under_act = late_rows_possible(self.qnetwork_local, obs.shape[0], self.shared_taus)
        fallback = (not under_act and bool(self.reset_fallback) and obs.is_cuda and self.use_fused_act and self.use_library_rng and self.n_step == 1
                    and hasattr(train_env, "take_owed_reset") and train_env.reset_owed_max_rows >= 0)
        actions = self.act_batch(obs, eps, cvar, late_env=train_env if under_act or fallback or getattr(train_env, "late_rows", None) is not None else None)
        if obs.is_cuda and hasattr(train_env, "step_append") and self.n_step == 1:
            # mn_step_append: the step kernel itself writes (obs_t, a, r, obs_t+1 incl. terminal observations, done)
            # into the replay ring -- no separate append launch, obs_t+1 is not re-read
            next_obs, reward, done, info = train_env.step_append(actions, obs, self.memory)
        else:
            next_obs, reward, done, info = train_env.step(actions)      # other half of the double buffer
            if obs.is_cuda:   # terminal obs, appended before the reset overwrites the finished rows
                self.memory.add_vector_step(obs, actions, reward, next_obs, done)
            else:
                self.memory.add_batch(obs, actions, reward, next_obs, done.float())
        due = cadence_tick(self, train_every)      # iqn/cadence.py: agent.py:126-147's rule (+ the target cadence in gradient steps)
        # first observations where done (`reset_under_act`: on the env's own stream, under the next call's act kernel, which takes those rows last -- launched BEHIND the
        # training event: a reset wavefront finds room beside an act workgroup, not beside a gradient step's, whose launches it would only hold up)
        if not (under_act or fallback):
            obs = train_env.reset_done()
        return VecStepState(obs, reward, done, info, due, under_act or fallback, eps, fallback)

    def vec_finish(self, train_env, state, per_iter=None):
        """The part of `vec_step` behind the gradient steps: target copy if due, (resets under the next act: mn_reset_done_async), counters.  Returns the
        observations for the next act."""
        per_iter = train_env.n_envs if per_iter is None else per_iter
        obs = state.obs
        if state.due.sync:
            self._sync_target()
        if state.under_act:      # (eps and the row count of the next act call: the library may leave the resets to that call's preparation launch)
            obs = train_env.reset_done(under_next_act=True, **({} if state.eps is None else dict(eps=state.eps, n_rows=obs.shape[0], fallback=state.fallback)))
        if self.current_timestep >= self.learning_starts:
            self.learning_timestep += 1
        self.current_timestep += per_iter
        return obs

    def _rollout_evaluation(self, eval_env, greedy, max_steps):
        """The evaluation episodes of `evaluation_vec` as ONE mn_rollout_iqn launch (iqn/fused_act.rollout_iqn) -- the traces, or None where the
        loop's acting form has no one-launch twin (CPU, PyTorch acting, torch.rand taus, the exact-f32 variant, launch-shared taus)."""
        if not (self.device.type == "cuda" and self.use_fused_act and self.use_library_rng and hasattr(eval_env, "h")):
            return None
        from .fused_act import ActRng, rollout_iqn
        if self._act_rng is None:
            self._act_rng = ActRng(self.gen.initial_seed(), self.device)
        return rollout_iqn(self.qnetwork_local, eval_env, max_steps, self._act_rng, cvar=1.0, adaptive=not greedy, shared_taus=self.shared_taus,
                           trace=EPISODE_TRACES)

    @torch.no_grad()
    def evaluation_vec(self, eval_env, eval_config, greedy=True, eval_log_path=None, max_steps=1000, one_launch=False, timestep=None):
        """agent.py:319-398 with all evaluation worlds stepped side by side on the GPU.
        `eval_env` is a VecMarineNavEnv with n_envs == len(eval_config); the npz schema is unchanged.
        `one_launch`: every episode in one mn_rollout_iqn launch instead of a Python iteration per step -- the same results, bit for bit (the
        returned dict, the logged entries, the npz, the act draws' counter); where that launch cannot reproduce the loop's acting form it falls
        back to the loop.  `timestep`: the timestep to log, where that is not the agent's current one."""
        from ..marinenav_env.vec_env import VecMarineNavEnv
        cfgs = list(eval_config.values())
        assert eval_env.n_envs == len(cfgs)
        r0 = cfgs[0]["robot"]
        eval_env.set_attrs(N=r0["N"], dt=r0["dt"])
        obs = eval_env.load_worlds([VecMarineNavEnv.world_from_eval_config(c) for c in cfgs]).clone()
        self.qnetwork_local.eval()
        tr = self._rollout_evaluation(eval_env, greedy, max_steps) if one_launch else None
        if tr is None:
            tr = loop_episodes(eval_env, obs, lambda t, o: self.act_batch(o, 0.0, 1.0 if greedy else self.adjust_cvar_batch(o)), max_steps)
        self.qnetwork_local.train()
        data = evaluation_from_traces(**host_traces(tr), discount=eval_env.discount, energy_tab=energy_table(r0["a"], r0["w"]), dt=r0["dt"], N=r0["N"])
        self._log_evaluation(greedy, *data, eval_log_path, timestep=timestep)
        action_data, reward_data, success_data, time_data, energy_data = data
        return dict(rewards=reward_data, successes=success_data, times=time_data, energies=energy_data, actions=action_data)

    def _log_evaluation(self, greedy, action_data, reward_data, success_data, time_data, energy_data, eval_log_path,
                        verbose=True, timestep=None):
        """agent.py:367-398: summary print + append + npz with the reference's keys.  `timestep`: the reported timestep the evaluated policy was taken
        at, where that is not now (iqn/deferred_eval.py)."""
        policy = "greedy" if greedy else "adaptive"
        if verbose:
            idx = np.where(np.array(success_data) == 1)[0]
            avg_t = np.mean(np.array(time_data)[idx]) if len(idx) else float("nan")
            avg_e = np.mean(np.array(energy_data)[idx]) if len(idx) else float("nan")
            print(f"++++++++ Evaluation info ({policy} IQN) ++++++++")
            print(f"Avg cumulative reward: {np.mean(reward_data):.2f}")
            print(f"Success rate: {np.sum(success_data) / len(success_data):.2f}")
            print(f"Avg time: {avg_t:.2f}")
            print(f"Avg energy: {avg_e:.2f}")
            print(f"++++++++ Evaluation info ({policy} IQN) ++++++++\n")
        self.eval_timesteps[policy].append(int(round(self.current_timestep * getattr(self, "_report_scale", 1.0))) if timestep is None else int(timestep))
        self.eval_actions[policy].append(action_data)
        self.eval_rewards[policy].append(reward_data)
        self.eval_successes[policy].append(success_data)
        self.eval_times[policy].append(time_data)
        self.eval_energies[policy].append(energy_data)
        if eval_log_path is not None:
            filename = "greedy_evaluations.npz" if greedy else "adaptive_evaluations.npz"
            np.savez(os.path.join(eval_log_path, filename),
                     timesteps=np.array(self.eval_timesteps[policy]),
                     actions=np.array(self.eval_actions[policy], dtype=object),
                     rewards=np.array(self.eval_rewards[policy]),
                     successes=np.array(self.eval_successes[policy]),
                     times=np.array(self.eval_times[policy]),
                     energies=np.array(self.eval_energies[policy]))
