"""Evaluations of MANY IQN checkpoints as ONE launch (iqn/fused_act.rollout_iqn_groups, C-ABI mn_rollout_iqn_groups).

One evaluation launch per checkpoint leaves the device idle: an episode workgroup has its CU to itself, so 30 evaluation worlds occupy 30 CUs for
as long as the longest episode lasts.  Here every checkpoint is one GROUP of rows of one big env -- the evaluation worlds once with cvar 1 (greedy)
and, with `adaptive`, once more with the adaptive flag: the layout the experiment sweep uses for its IQN group -- acting with its own weight image
and its own tau stream, and all groups run side by side in one launch.

* `DeferredEvaluations`: the evaluation points of a training run (IQNAgent.learn_vec(eval_deferred=True), train_iqn --eval-deferred).  Taking a
  point is two device copies on the training stream; the episodes of all pending points run later, in one launch.
* `evaluate_checkpoints`: N saved networks on the evaluation worlds, one call, one launch (scripts/evaluate_checkpoints.py).

A group computes bit for bit what `rollout_iqn(net, env, T, ActRng(seed), cvar_rows=..., adaptive_rows=...)` computes on an env of its own with the
group's rows; `episodes.tally` turns the traces of all groups into per-episode numbers at once.
"""
import json
import os

import numpy as np
import torch

from ..episodes import EPISODE_TRACES, energy_table, host_traces, tally

SEED_STEP = 0x9E3779B97F4A7C15
SEED_MASK = 0x7FFFFFFFFFFFFFFF


def checkpoint_seed(base_seed, j):
    """The tau-stream seed of checkpoint j (counted from 0 over the whole run) of an agent whose generator was seeded with `base_seed`: a stream of its
    own per checkpoint, none of them the agent's training stream."""
    return (int(base_seed) + SEED_STEP * (int(j) + 1)) & SEED_MASK


def group_rows(n_worlds, adaptive=True):
    """Per-row cvar [R] float32 and adaptive flag [R] bool of ONE group: the worlds with cvar 1 (greedy), then -- `adaptive` -- once more with the flag."""
    reps = 2 if adaptive else 1
    return (torch.ones(n_worlds * reps, dtype=torch.float32),
            torch.tensor([False] * n_worlds + ([True] * n_worlds if adaptive else []), dtype=torch.bool))


def records_from_traces(traces, n_groups, n_worlds, adaptive, discount, energy_tab, dt, N):
    """The evaluation lists of every group from the numpy traces [T][n_groups * R] of a grouped launch (R = n_worlds, twice that with `adaptive`): ONE
    `episodes.tally` over all columns -- its loop masks every column by its own `alive`, so a group's numbers are what a tally of its columns alone
    gives --, then per group {policy: (action_data, reward_data, success_data, time_data, energy_data)}, `evaluation_from_traces`' tuple."""
    R = n_worlds * (2 if adaptive else 1)
    assert traces["reward"].shape[1] == n_groups * R
    tl = tally(traces["reward"], traces["done"], traces["info"], traces["action"], discount, energy_tab)
    out = []
    for g in range(n_groups):
        rec = {}
        for p, policy in enumerate(("greedy", "adaptive") if adaptive else ("greedy",)):
            sl = slice(g * R + p * n_worlds, g * R + (p + 1) * n_worlds)
            rec[policy] = (tl["actions"][sl], [float(x) for x in tl["ret"][sl]], [bool(x) for x in (tl["last_info"][sl] == 4)],
                           [float(dt * N * l) for l in tl["length"][sl]], [float(x) for x in tl["energy"][sl]])
        out.append(rec)
    return out


def save_flat_checkpoint(net, flat, directory, prefix=""):
    """`ObsEncoder.save` for the FLAT parameter vector `flat` (named_parameters() order) of a network shaped like `net`: the same two files."""
    sd, off = {}, 0
    for name, p in net.named_parameters():
        sd[name] = flat[off:off + p.numel()].detach().clone().view(p.shape)
        off += p.numel()
    assert off == flat.numel() and list(sd) == list(net.state_dict())
    torch.save(sd, os.path.join(directory, prefix + "network_params.pth"))
    with open(os.path.join(directory, prefix + "constructor_params.json"), mode="w") as f:
        json.dump(net.get_constructor_parameters(), f)


class GroupEnvs:
    """The envs grouped launches run in, one per row count, loaded with the evaluation worlds once per group row block."""

    def __init__(self, eval_config, adaptive, device, precision):
        from ..marinenav_env.vec_env import VecMarineNavEnv
        cfgs = list(eval_config.values())
        self.robot = cfgs[0]["robot"]
        self.worlds = [VecMarineNavEnv.world_from_eval_config(c) for c in cfgs]
        self.adaptive, self.device, self.precision = bool(adaptive), torch.device(device), precision
        self.R = len(self.worlds) * (2 if adaptive else 1)
        self._envs = {}

    def loaded(self, n_groups):
        from ..marinenav_env.vec_env import VecMarineNavEnv
        env = self._envs.get(n_groups)
        if env is None:
            env = self._envs[n_groups] = VecMarineNavEnv(n_groups * self.R, device=self.device, precision=self.precision)
            env.set_attrs(N=self.robot["N"], dt=self.robot["dt"])
        env.load_worlds(self.worlds, repeat=n_groups * self.R // len(self.worlds))
        return env

    def rows(self, n_groups):
        cv, ad = group_rows(len(self.worlds), self.adaptive)
        return cv.repeat(n_groups), ad.repeat(n_groups)

    def run(self, images, rng_states, max_steps):
        """ONE launch for the groups of `images` / `rng_states`; returns (host traces of the steps run, steps_run [G] numpy, discount)."""
        from .fused_act import rollout_iqn_groups
        G = images.shape[0]
        env = self.loaded(G)
        cv, ad = self.rows(G)
        tr = rollout_iqn_groups(images, env, max_steps, rng_states, self.R, cvar_rows=cv, adaptive_rows=ad, trace=EPISODE_TRACES)
        host = host_traces(tr)      # `done` first, then of the others the rows of the steps run
        return host, tr["steps_run"].cpu().numpy(), env.discount

    def close(self):
        for env in self._envs.values():
            env.close()
        self._envs = {}


class DeferredEvaluations:
    """The evaluation points of a training run, taken now and run later: `snapshot()` keeps the policy of the moment, `flush()` evaluates every pending
    snapshot in ONE mn_rollout_iqn_groups launch and logs them, in order, exactly as `IQNAgent.evaluation_vec` logs an evaluation -- `_log_evaluation`
    with the snapshot's timestep (the npz files keep the reference's schema and keys), the `best_*` rule of `learn_vec`, `network_params.pth` of the
    latest snapshot.

    Group layout: one group per checkpoint -- the worlds of `eval_config` with cvar 1 (greedy), then, with `adaptive`, once more with the adaptive
    flag: R = 30 or 60 rows for the 30 evaluation worlds.
    Taus: checkpoint j (counted over the run) draws from a stream of its own, seed `checkpoint_seed(agent.gen.initial_seed(), j)`, counter 0.  The agent's
    own act stream (`_act_rng`, the one training acts with) is never touched, and `snapshot()` enqueues two device copies and nothing else: how often one
    evaluates does not change the training run.
    `flush()` runs by itself once `max_pending` snapshots are pending; call it at the end of the run.
    Crash safety: between flushes NOTHING of the pending evaluations is on disk -- neither their npz entries nor their checkpoints; `max_pending`
    bounds what a crash loses.
    Device memory: `max_pending` x 151 KB of weight images (+ 143 KB of parameters each), and for a flush 10 B x `max_steps` x rows of traces (rows =
    pending x R: 38 MB for 64 pending points of 60 rows at 1 000 steps).
    The host half (`log_traces`) works on numpy traces and needs no GPU."""

    def __init__(self, agent, eval_config, adaptive=True, max_pending=64, max_steps=1000, eval_log_path=None, precision="f64", verbose=True):
        self.agent, self.eval_config = agent, eval_config
        self.adaptive, self.max_pending, self.max_steps = bool(adaptive), int(max_pending), int(max_steps)
        assert self.max_pending >= 1 and self.max_steps >= 1
        self.eval_log_path, self.precision, self.verbose = eval_log_path, precision, verbose
        cfgs = list(eval_config.values())
        self.n_worlds = len(cfgs)
        self.robot = cfgs[0]["robot"]
        self.pending = []          # dict(timestep, grad_steps, vector_step, seed) per pending snapshot; slot = position
        self.n_taken = 0           # snapshots over the whole run: the j of the seed formula
        self.launches = 0
        self.steps_run = []        # per evaluated checkpoint: the longest episode of its group
        self._images = self._params = self._envs = None

    def seed_of(self, j):
        return checkpoint_seed(self.agent.gen.initial_seed(), j)

    # ---- device half ---------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def snapshot(self, vector_step=None, timestep=None):
        """Keep the policy of this moment for a later evaluation: the acting weight image and the flat parameters go into slot `len(pending)` on the
        current stream -- two device copies, no host synchronisation -- and the reported timestep is noted (`timestep`, or the agent's current one).  The snapshot that fills the last of the
        `max_pending` slots runs `flush()`."""
        from .fused_act import export_image, image_floats
        agent, net = self.agent, self.agent.qnetwork_local
        dev = net.output_layer.weight.device
        if self._images is None:
            self._images = torch.empty(self.max_pending, image_floats(), dtype=torch.int32, device=dev)
            self._params = torch.empty(self.max_pending, sum(p.numel() for p in net.parameters()), dtype=torch.float32, device=dev)
        slot = len(self.pending)
        export_image(net, self._images[slot])
        torch.cat([p.detach().reshape(-1) for p in net.parameters()], out=self._params[slot])
        self.pending.append(dict(timestep=int(round(agent.current_timestep * getattr(agent, "_report_scale", 1.0))) if timestep is None else int(timestep), grad_steps=agent.grad_steps,
                                 vector_step=vector_step, seed=self.seed_of(self.n_taken)))
        self.n_taken += 1
        if len(self.pending) >= self.max_pending:
            self.flush()

    @torch.no_grad()
    def flush(self):
        """Evaluate and log every pending snapshot: ONE launch on an env of pending x R rows, `done` copied first and then the rows of the steps run, one
        tally, then `log_traces`.  Returns the number of checkpoints evaluated."""
        n = len(self.pending)
        if n == 0:
            return 0
        if self._envs is None:
            self._envs = GroupEnvs(self.eval_config, self.adaptive, self._images.device, self.precision)
        states = torch.tensor([[m["seed"], 0] for m in self.pending], dtype=torch.int64, device=self._images.device)
        host, steps, discount = self._envs.run(self._images[:n], states, self.max_steps)
        self.launches += 1
        self.steps_run += [int(s) for s in steps]
        self.log_traces(host, self.pending, self._params[:n], discount)
        self.pending = []
        return n

    def close(self):
        if self._envs is not None:
            self._envs.close()
            self._envs = None

    # ---- checkpoints ---------------------------------------------------------------------------------------------------
    def state_dict(self):
        """What a continued run needs of the deferred evaluations once nothing is pending: `flush()` runs first -- legal at any point, because every
        group of a grouped launch is bit for bit a launch of its own and the training streams are untouched -- and then the count of snapshots taken (the
        j of the seed formula) is all there is; the record logged so far and the best-so-far score live in the agent (`IQNAgent.state_dict`)."""
        self.flush()
        return dict(n_taken=int(self.n_taken), launches=int(self.launches), steps_run=list(self.steps_run))

    def load_state_dict(self, sd):
        assert not self.pending, "load_state_dict into DeferredEvaluations with pending snapshots"
        self.n_taken, self.launches, self.steps_run = int(sd["n_taken"]), int(sd["launches"]), list(sd["steps_run"])

    # ---- host half -----------------------------------------------------------------------------------------------------
    def log_traces(self, traces, metas, params, discount):
        """Log the checkpoints `metas` (dicts with timestep / grad_steps / vector_step) from the numpy traces [T][len(metas) * R] of their launch, in
        order: per checkpoint `agent._log_evaluation` for greedy and -- `adaptive` -- adaptive with the checkpoint's timestep, then `learn_vec`'s
        `best_*` rule on its greedy record; `params[j]` is checkpoint j's flat parameter vector (what the `best_*` and the latest files are written
        from).  The npz files are written once, after the last checkpoint.  Returns the per-checkpoint records."""
        agent, r0 = self.agent, self.robot
        recs = records_from_traces(traces, len(metas), self.n_worlds, self.adaptive, discount, energy_table(r0["a"], r0["w"]), r0["dt"], r0["N"])
        path = self.eval_log_path
        for j, (meta, rec) in enumerate(zip(metas, recs)):
            last = j == len(metas) - 1
            for policy in rec:
                agent._log_evaluation(policy == "greedy", *rec[policy], path if last else None, verbose=self.verbose, timestep=meta["timestep"])
            _, rewards, successes = rec["greedy"][:3]
            score = (int(sum(successes)), float(np.mean(rewards)))
            if agent.best_eval is None or score > agent.best_eval["score"]:
                agent.best_eval = dict(score=score, timestep=meta["timestep"], grad_steps=meta["grad_steps"], vector_step=meta["vector_step"])
                if path is not None:
                    save_flat_checkpoint(agent.qnetwork_local, params[j], path, prefix="best_")
                    with open(os.path.join(path, "best_evaluation.json"), "w") as f:
                        json.dump(dict(successes=score[0], n_worlds=len(successes), mean_return=score[1],
                                       **{k: v for k, v in agent.best_eval.items() if k != "score"}), f)
        if path is not None and len(metas):
            save_flat_checkpoint(agent.qnetwork_local, params[len(metas) - 1], path)
        return recs


@torch.no_grad()
def evaluate_checkpoints(nets_or_paths, eval_config, device, adaptive=True, seeds=None, max_steps=1000, precision="f64"):
    """N IQN networks (`ObsEncoder`s, or checkpoint directories holding network_params.pth + constructor_params.json) on the worlds of `eval_config`,
    greedy and -- `adaptive` -- adaptive, as ONE launch.  `seeds`: one tau-stream seed per network (default 0 for each: a network's result does not
    depend on its place in the list).  Returns one record per network: {policy: dict(successes, n_worlds, mean_return, rewards, success, times,
    energies, actions)} plus `steps_run`, the longest episode of its group."""
    from .fused_act import export_image, image_floats
    from .model import ObsEncoder
    device = torch.device(device)
    nets = [ObsEncoder.load(x, device) if isinstance(x, (str, os.PathLike)) else x for x in nets_or_paths]
    seeds = [0] * len(nets) if seeds is None else [int(s) for s in seeds]
    assert len(seeds) == len(nets) and len(nets) >= 1
    images = torch.empty(len(nets), image_floats(), dtype=torch.int32, device=device)
    for j, net in enumerate(nets):
        export_image(net, images[j])
    states = torch.tensor([[s & SEED_MASK, 0] for s in seeds], dtype=torch.int64, device=device)
    envs = GroupEnvs(eval_config, adaptive, device, precision)
    try:
        host, steps, discount = envs.run(images, states, max_steps)
    finally:
        envs.close()
    r0 = envs.robot
    recs = records_from_traces(host, len(nets), len(envs.worlds), adaptive, discount, energy_table(r0["a"], r0["w"]), r0["dt"], r0["N"])
    out = []
    for rec, s in zip(recs, steps):
        o = {p: dict(successes=int(sum(succ)), n_worlds=len(succ), mean_return=float(np.mean(rew)), rewards=rew, success=succ, times=times,
                     energies=energies, actions=actions) for p, (actions, rew, succ, times, energies) in rec.items()}
        o["steps_run"] = int(s)
        out.append(o)
    return out
