"""Evaluations of MANY DQN checkpoints as ONE launch (dqn/policy.rollout_dqn_groups, C-ABI mn_rollout_dqn_groups).

One evaluation launch per checkpoint leaves the device idle: the weight image fills a CU's LDS and a wavefront carries 8 envs, so the 30 evaluation
worlds are 4 workgroups on 4 CUs for as long as the longest episode lasts.  Here every checkpoint is one GROUP of rows of one big env -- the
evaluation worlds, once -- acting with its own weight image, and all groups run side by side in one launch.  The envs are
`iqn.deferred_eval.GroupEnvs` (without the adaptive half), the bookkeeping one `episodes.tally` over all columns.

* `DeferredEvaluations`: the evaluation points of a training run (train_dqn.run_trial(eval_deferred=True), train_dqn --eval-deferred).  Taking a
  point is one small pack launch and two device copies on the training stream; the episodes of all pending points run later, in one launch.
* `evaluate_checkpoints`: N saved networks on the evaluation worlds, one call, one launch (scripts/evaluate_checkpoints.py --agent dqn).

The greedy DQN draws nothing, so there are no seeds: a group computes bit for bit what `policy.rollout(env, T)` computes on an env of its own with the
group's rows, and a deferred run writes exactly the files of the inline run.
"""
import os

import numpy as np
import torch

from ..episodes import EPISODE_TRACES, energy_table, host_traces, steps_run, tally
from ..iqn.deferred_eval import GroupEnvs


def records_from_traces(traces, n_groups, n_worlds, discount, energy_tab, dt, N):
    """`train_dqn.evaluation_from_rollout`'s dict for every group from the numpy traces [T][n_groups * n_worlds] of a grouped launch: ONE
    `episodes.tally` over all columns -- its loop masks every column by its own `alive`, so a group's numbers are what a tally of its columns alone
    gives --, plus `steps_run`, the longest episode of the group."""
    R = n_worlds
    assert traces["reward"].shape[1] == n_groups * R
    tl = tally(traces["reward"], traces["done"], traces["info"], traces["action"], discount, energy_tab)
    out = []
    for g in range(n_groups):
        sl = slice(g * R, (g + 1) * R)
        out.append(dict(rewards=tl["ret"][sl], successes=tl["last_info"][sl] == 4, times=np.array([dt * N * l for l in tl["length"][sl]], dtype=np.float64),
                        energies=tl["energy"][sl], actions=tl["actions"][sl], steps_run=steps_run(traces["done"][:, sl])))
    return out


def state_dict_from_flat(agent, local, target):
    """`DQNAgent.state_dict()` (q_net.* and q_net_target.* keys, in that order) holding the FLAT parameter vectors `local` / `target`
    (`q_net.named_parameters()` order) instead of the agent's current weights, as CPU tensors: what `train_dqn.save_zip` writes."""
    sd = {}
    for prefix, net, flat in (("q_net.", agent.q_net, local), ("q_net_target.", agent.q_net_target, target)):
        off = 0
        for name, p in net.named_parameters():
            sd[prefix + name] = flat[off:off + p.numel()].detach().view(p.shape).cpu().clone()
            off += p.numel()
        assert off == flat.numel()
    assert list(sd) == list(agent.state_dict())
    return sd


def can_defer(agent):
    """Whether the agent's policy acts through the fused kernel (a GPU, the [64, 64] head, use_fused_act): only then the grouped launch is its twin."""
    if agent.device.type != "cuda":
        return False
    with torch.no_grad():
        return bool(agent.policy._fusable(torch.empty(1, agent.policy.state_size, device=agent.device)))


class DeferredEvaluations:
    """The evaluation points of a DQN training run, taken now and run later: `snapshot()` keeps the policy of the moment, `flush()` evaluates every
    pending snapshot in ONE mn_rollout_dqn_groups launch and then does, in order, exactly what `train_dqn.run_trial` does inline per point: append to
    the log, write evaluations.npz (once, after the last pending point), latest_model.zip from the last snapshot, best_model.zip whenever the mean
    reward beats the best so far -- from THAT snapshot's parameters, local and target, with `save_zip`'s keys --, and the verbose line.

    Group layout: one group per checkpoint, the worlds of `eval_config` once: R = 30 rows for the 30 evaluation worlds, 4 workgroups per group.
    The evaluation is deterministic and draws nothing; `snapshot()` enqueues one pack launch and two device copies and nothing else, so how often one
    evaluates does not change the training run, and the files equal the inline run's.
    `flush()` runs by itself once `max_pending` snapshots are pending; call it at the end of the run.
    Crash safety: between flushes NOTHING of the pending evaluations is on disk -- neither their npz entries nor their checkpoints; `max_pending`
    bounds what a crash loses.
    Device memory: `max_pending` x 127 KB of weight images (+ 2 x 111 KB of local and target parameters each), and for a flush 10 B x `max_steps` x
    rows of traces (rows = pending x R: 19 MB for 64 pending points of 30 rows at 1 000 steps).
    The host half (`log_traces`) works on numpy traces and needs no GPU."""

    def __init__(self, agent, eval_config, exp_dir, max_pending=64, max_steps=1000, precision="f64", verbose=True, label="", n_evals=None, t0=None):
        self.agent, self.eval_config, self.exp_dir = agent, eval_config, exp_dir
        self.max_pending, self.max_steps = int(max_pending), int(max_steps)
        assert self.max_pending >= 1 and self.max_steps >= 1
        self.precision, self.verbose, self.label, self.n_evals, self.t0 = precision, verbose, label, n_evals, t0
        cfgs = list(eval_config.values())
        self.n_worlds = len(cfgs)
        self.robot = cfgs[0]["robot"]
        self.pending = []          # the reported timestep of every pending snapshot; slot = position
        self.log = dict(timesteps=[], rewards=[], times=[], energies=[], successes=[], actions=[])
        self.best = -np.inf
        self.launches = 0
        self.steps_run = []        # per evaluated checkpoint: the longest episode of its group
        self._images = self._local = self._target = self._envs = None

    # ---- device half ---------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def snapshot(self, timestep):
        """Keep the policy of this moment for a later evaluation, reported at `timestep`: the weight image and the flat local and target parameters go
        into slot `len(pending)` on the current stream -- no host synchronisation.  The snapshot that fills the last of the `max_pending` slots runs
        `flush()`."""
        from .policy import image_floats
        agent = self.agent
        if self._images is None:
            dev, P = agent.device, sum(p.numel() for p in agent.q_net.parameters())
            self._images = torch.empty(self.max_pending, image_floats(), dtype=torch.float32, device=dev)
            self._local = torch.empty(self.max_pending, P, dtype=torch.float32, device=dev)
            self._target = torch.empty(self.max_pending, P, dtype=torch.float32, device=dev)
        slot = len(self.pending)
        agent.policy.export_image(self._images[slot])
        ft = agent._fused if agent._fused is not None and agent._fused.owns(agent) else None
        if ft is not None:      # the fused trainer's flat buffers ARE the parameters
            self._local[slot].copy_(ft.local)
            self._target[slot].copy_(ft.target)
        else:
            torch.cat([p.detach().reshape(-1) for p in agent.q_net.parameters()], out=self._local[slot])
            torch.cat([p.detach().reshape(-1) for p in agent.q_net_target.parameters()], out=self._target[slot])
        self.pending.append(int(timestep))
        if len(self.pending) >= self.max_pending:
            self.flush()

    @torch.no_grad()
    def flush(self):
        """Evaluate and log every pending snapshot: ONE launch on an env of pending x R rows, `done` copied first and then the rows of the steps run, one
        tally, then `log_traces`.  Returns the number of checkpoints evaluated."""
        from .policy import rollout_dqn_groups
        n = len(self.pending)
        if n == 0:
            return 0
        if self._envs is None:
            self._envs = GroupEnvs(self.eval_config, False, self._images.device, self.precision)
        env = self._envs.loaded(n)
        tr = rollout_dqn_groups(self._images[:n], env, self.max_steps, self._envs.R, trace=EPISODE_TRACES)
        self.launches += 1
        self.log_traces(host_traces(tr), self.pending, self._local[:n], self._target[:n], env.discount)
        self.pending = []
        return n

    def close(self):
        if self._envs is not None:
            self._envs.close()
            self._envs = None

    # ---- checkpoints ---------------------------------------------------------------------------------------------------
    def state_dict(self):
        """What a continued run needs of the deferred evaluations once nothing is pending: `flush()` runs first -- legal at any point, because every group of
        a grouped launch is bit for bit a launch of its own and the greedy DQN draws nothing -- and then the record logged so far, the best mean reward and
        the counts (`n_taken`: snapshots taken, all logged by now) are all there is.  Numpy arrays and plain values; no wall-clock value."""
        import copy
        self.flush()
        return dict(log=copy.deepcopy(self.log), best=float(self.best), n_taken=len(self.log["timesteps"]), launches=int(self.launches),
                    steps_run=[int(s) for s in self.steps_run])

    def load_state_dict(self, sd):
        import copy
        assert not self.pending, "load_state_dict into DeferredEvaluations with pending snapshots"
        if int(sd["n_taken"]) != len(sd["log"]["timesteps"]):
            raise ValueError("DeferredEvaluations.load_state_dict: the state counts other snapshots than its record holds")
        self.log, self.best = copy.deepcopy(sd["log"]), float(sd["best"])
        self.launches, self.steps_run = int(sd["launches"]), [int(s) for s in sd["steps_run"]]

    # ---- host half -----------------------------------------------------------------------------------------------------
    def log_traces(self, traces, timesteps, local, target, discount):
        """Log the checkpoints reported at `timesteps` from the numpy traces [T][len(timesteps) * R] of their launch, in order, as `run_trial` logs an
        inline evaluation; `local[j]` / `target[j]` are checkpoint j's flat parameter vectors (what best_model.zip and latest_model.zip are written
        from).  evaluations.npz is written once, after the last checkpoint.  Returns the per-checkpoint records."""
        import time
        from ..train_dqn import save_state_zip, write_evaluations
        r0, log = self.robot, self.log
        recs = records_from_traces(traces, len(timesteps), self.n_worlds, discount, energy_table(r0["a"], r0["w"]), r0["dt"], r0["N"])
        lines = []
        for j, (ts, ev) in enumerate(zip(timesteps, recs)):
            log["timesteps"].append(int(ts))
            for k in ("rewards", "times", "energies", "successes", "actions"):
                log[k].append(ev[k])
            self.steps_run.append(ev["steps_run"])
            mean_r = float(np.mean(ev["rewards"]))
            lines.append((len(log["timesteps"]), int(ts), int(np.sum(ev["successes"])), mean_r))
            if mean_r > self.best:
                self.best = mean_r
                save_state_zip(state_dict_from_flat(self.agent, local[j], target[j]), os.path.join(self.exp_dir, "best_model.zip"))
        if len(timesteps):
            write_evaluations(self.exp_dir, log)
            save_state_zip(state_dict_from_flat(self.agent, local[len(timesteps) - 1], target[len(timesteps) - 1]), os.path.join(self.exp_dir, "latest_model.zip"))
        if self.verbose:
            for k, ts, succ, mean_r in lines:
                print(f"[train_dqn] {self.label}eval {k}/{self.n_evals if self.n_evals is not None else '?'} at {ts} steps: "
                      f"{succ}/{self.n_worlds} successes, mean return {mean_r:.2f}" + (f" ({time.time() - self.t0:.1f} s)" if self.t0 is not None else ""),
                      flush=True)
        return recs


@torch.no_grad()
def evaluate_checkpoints(policies_or_paths, eval_config, device, max_steps=1000, precision="f64"):
    """N DQN networks (`DQNPolicy` objects, or anything `DQNPolicy.load` reads: an sb3-style .zip, a policy.pth, the q_net .npz) on the worlds of
    `eval_config`, greedy, as ONE launch.  Returns one record per network: the fields of `train_dqn.evaluation_from_rollout` for the network's
    columns (rewards, successes [per world, bool], times, energies, actions) plus n_successes, n_worlds, mean_return and steps_run (the longest
    episode of its group).  A network's record does not depend on its place in the list."""
    from .policy import DQNPolicy, image_floats, rollout_dqn_groups
    device = torch.device(device)
    pols = [DQNPolicy.load(os.fspath(x), device=device) if isinstance(x, (str, os.PathLike)) else x for x in policies_or_paths]
    assert len(pols) >= 1
    images = torch.empty(len(pols), image_floats(), dtype=torch.float32, device=device)
    for j, pol in enumerate(pols):
        pol.export_image(images[j])
    envs = GroupEnvs(eval_config, False, device, precision)
    try:
        env = envs.loaded(len(pols))
        tr = rollout_dqn_groups(images, env, max_steps, envs.R, trace=EPISODE_TRACES)
        host, discount = host_traces(tr), env.discount
    finally:
        envs.close()
    r0 = envs.robot
    recs = records_from_traces(host, len(pols), len(envs.worlds), discount, energy_table(r0["a"], r0["w"]), r0["dt"], r0["N"])
    for rec in recs:
        rec.update(n_successes=int(np.sum(rec["successes"])), n_worlds=len(rec["successes"]), mean_return=float(np.mean(rec["rewards"])))
    return recs
