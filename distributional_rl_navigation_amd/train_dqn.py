"""Training driver of the DQN baseline: counterpart of the reference's train_sb3_model.py with config/config_DQN.json for the batched
path, with the interface of train_iqn.

    python -m distributional_rl_navigation_amd.train_dqn -C config_DQN.json [--n-envs 4096] [--batch 256] [--replay N]
        [--grad-steps G] [--total-grad-steps N] [--n-evals K] [--torch-train] [--eval-one-launch] [--eval-deferred] [--dry-run]
        [--env-budget reference] [--episode-log [full]] [--train-steps-per-call {auto,1,K,multi}] [--fused-collect] [--together [--stack-envs]]
        [--checkpoint-every K] [--stop-after K] [--resume TRAINING_DIR] [--run-name NAME]

Same JSON schema as train_iqn (agent, seed (list -> grid), total_timesteps, eval_freq, save_dir); the trials run one after another
on one device, or -- `--together` -- the seeds of a config in lockstep with ONE launch per gradient step for all of them (`run_trials_together`,
dqn/group_train.py): the same per-seed files.  Cadence: `train_iqn.plan_cadence` with the reference DQN's values (one batch-32 gradient step per env step, target
copy every 10 000 env steps) -- the reference's learner budget in batches of `--batch`, every run fraction rescaled.  Learning starts
after ceil(10 000 / n_envs) vector steps (sb3's learning_starts), exploration falls linearly from 1.0 to 0.05 over the first 10 % of the
planned run (exploration_fraction), the target network is hard-copied every `target_sync_grad_steps` gradient steps, the curriculum
is TRAINING_SCHEDULE on reference-scaled time, and the agent seed is seed + 100.  The gradient step is the fused HIP launch
(csrc/dqn_train.hip); `--torch-train` selects the eager PyTorch step.

Per trial, in save_dir/training_<time>/seed_<s>/, what the sb3 fork's EvalCallback writes: trial_config.json (with the batched
plan), training_schedule.json, evaluations.npz (timesteps, rewards, times, energies, successes, actions on the 30 evaluation worlds
of create_eval_configs), latest_model.zip after every evaluation and best_model.zip on a new best mean reward (a zip holding
policy.pth with q_net.* and q_net_target.*).

`--env-budget reference`: the reference's own experiment instead of its learner budget in big batches -- total_timesteps env steps in vector steps of
N = 80, one batch-32 gradient step per env step from learning_starts on (2 990 000), target copy every 10 000 of them, the 1 M-row ring, evaluations logged
at the reference's timesteps (deferred), and training_log.npz from the device-side episode log (episode_log.py; `--episode-log [full]` elsewhere).

`--fused-collect`: the collect phase on the device -- the act launch draws the exploration itself (C-ABI mn_dqn_act_rng, the library's counter-based
generator instead of torch.Generator: other draws, hence opt-in) and the env step appends the transitions (mn_step_append).  `--together --stack-envs`:
the seeds' envs are the rows of ONE handle and each vector step is one act, one step, one append and one reset launch for all of them
(dqn/group_collect.py); every seed's files equal those of its own `--fused-collect` run.

`--eval-deferred`: an evaluation point only keeps the policy of the moment (a weight image and the parameters, device copies on the training
stream); the episodes of all pending points run later as ONE mn_rollout_dqn_groups launch (dqn/deferred_eval.py) and are logged as above -- the same
files, bit for bit, without a host round trip per point: `--n-evals 300` logs the reference's evaluation density.

`--checkpoint-every K`, `--stop-after K`, `--resume TRAINING_DIR`: as train_iqn's, with its helpers -- behind every K-th vector step the whole trial (env snapshot,
replay ring, the learner's full state, the evaluations, the episode log, `TrialRun`'s own words) goes into checkpoint.pt of the seed's directory; a stopped run
continues in a fresh process and, on the same gradient-step path, writes the files of the uninterrupted run.  Also under `--together` (per-seed envs): every
seed writes its own checkpoint, the one its sequential run writes, so a run stopped in lockstep resumes sequentially and the other way round.  Not with
`--stack-envs` (CHECKPOINT_REFUSALS).  Every trial directory ends with completed.json, written last.
"""
import argparse
import io
import json
import os
import time
import zipfile
from datetime import datetime

import numpy as np

from .train_iqn import (CHECKPOINT_FILE, CHECKPOINT_FORMAT, CHECKPOINT_PREV_FILE, COMPLETED_FILE, TRAINING_SCHEDULE, check_resumable, create_eval_configs,
                        first_difference, load_checkpoint, make_episode_log, plan_cadence, plan_eval_points, resolve_budget_args, resume_point, trial_dir,
                        trial_params, trial_shape, write_checkpoint)

REF_BATCH, REF_UPDATE_EVERY, REF_TARGET_INTERVAL, REF_LEARNING_STARTS = 32, 1, 10_000, 10_000      # config_DQN.json / sb3 DQN defaults
EXPLORATION_FRACTION, EPS_INITIAL, EPS_FINAL = 0.1, 1.0, 0.05
# What `--train-steps-per-call auto` takes: 1, the loop of single launches.  The multi-step call is opt-in ("multi", or a number of steps per call) until
# profiles/dqn_multi_step_bench.txt shows its median per-step time at K = 80 below the loop's with ranges that do not overlap (README).
AUTO_TRAIN_STEPS_PER_CALL = 1


def steps_per_call(value):
    """`--train-steps-per-call`: "auto" -> AUTO_TRAIN_STEPS_PER_CALL; "multi" -> None (a whole stretch between target copies per call); K >= 1 -> at most K
    gradient steps per call (1: one `agent.train()` per step)."""
    if value == "auto":
        value = AUTO_TRAIN_STEPS_PER_CALL
    if value == "multi":
        return None
    k = int(value)
    if k < 1:
        raise ValueError(f"train_steps_per_call: 'auto', 'multi' or a number >= 1, not {value!r}")
    return k


def make_plan(params, n_envs, batch, grad_steps=None, total_grad_steps=None, n_evals=None, budget="learner", reference=None):
    """`train_iqn.plan_cadence` with the reference DQN's constants.  `budget="reference"`: the reference's own experiment in vector steps of `n_envs` env
    steps -- one batch-32 gradient step per env step from the vector step that starts at learning_starts on (n_envs per vector step, total_timesteps -
    learning_starts in all), target copy every 10 000 of them, the reference's evaluation timesteps (`train_iqn.plan_reference`)."""
    plan = plan_cadence(params["total_timesteps"], params["eval_freq"], n_envs, batch, ref_batch=REF_BATCH, ref_update_every=REF_UPDATE_EVERY,
                        ref_target_interval=REF_TARGET_INTERVAL, grad_steps_per_vector_step=grad_steps, total_grad_steps=total_grad_steps,
                        n_evals=n_evals, budget=budget, reference=reference)
    if budget == "reference":
        # the loop below trains behind vector step `it` once it + 1 >= learning_starts_vector_steps: the first that trains STARTS at learning_starts
        plan["learning_starts_vector_steps"] = plan["learning_starts"] // n_envs + 1
    else:
        plan["learning_starts_vector_steps"] = -(-REF_LEARNING_STARTS // n_envs)
    plan["exploration_vector_steps"] = EXPLORATION_FRACTION * plan["vector_steps"]
    return plan


def plan_trial(params, n_envs, batch=None, replay=None, grad_steps=None, total_grad_steps=None, n_evals=None, env_budget="learner", reference=None):
    """(n_envs, batch, replay, plan) of one trial: the budget's defaults filled in, `make_plan`, and the check every trial passes before anything is written or
    allocated.  No GPU needed: `--resume` and `--dry-run --resume` plan with it as `TrialRun` does."""
    n_envs, batch, replay = resolve_budget_args(env_budget, n_envs, batch, replay)
    plan = make_plan(params, n_envs, batch, grad_steps, total_grad_steps, n_evals, budget=env_budget, reference=reference)
    if env_budget == "reference":
        if replay is not None and replay != plan["replay"]:
            raise ValueError(f"env_budget='reference' keeps the reference's replay ring ({plan['replay']} rows); {replay} contradicts it")
        replay = plan["replay"]
    return n_envs, batch, replay, plan


def run_shaping_args(env_budget="learner", fused_collect=False, eval_deferred=False, eval_one_launch=False, episode_log=None, max_eval_steps=1000, reference=None,
                     eval_worlds=None, **_):
    """The arguments of `run_trial` that shape a run beside its plan, normalised: what a checkpoint records and `--resume` compares (`train_iqn.check_resumable`).
    ONE place builds it, for the run, the lockstep run and `--dry-run --resume`; the defaults are `run_trial`'s.  (`torch_train` and `train_steps_per_call` are
    recorded by the checkpoint but not compared: the multi-step call is bit-identical to the loop, and a checkpoint of one gradient-step path continues on the
    other as a valid run.)"""
    return dict(env_budget=env_budget, fused_collect=bool(fused_collect), eval_deferred=bool(eval_deferred) or env_budget == "reference",
                eval_one_launch=bool(eval_one_launch), episode_log=episode_log, max_eval_steps=int(max_eval_steps), reference=dict(reference or {}),
                eval_worlds=eval_worlds)


CHECKPOINT_REFUSALS = dict(
    stack_envs="--checkpoint-every, --stop-after and --resume keep one checkpoint per seed; with --stack-envs the seeds share ONE env handle, whose snapshot is one "
               "blob for all rows, which a seed's checkpoint cannot hold: use --together without --stack-envs")


def _log(line):
    print(line.replace("[train_iqn]", "[train_dqn]", 1), flush=True)


def check_lockstep(points):
    """`points`: (seed, what, state) of the seeds that are left of a group (`train_iqn.resume_point`; none "completed").  The lockstep loop continues them only
    from ONE vector step: all at "start", or all with checkpoints of the same step.  Returns that step (0: the start); ValueError names every seed with its
    step."""
    steps = [0 if state is None else int(state["vector_step"]) for _, _, state in points]
    if len(set(steps)) > 1:
        where = ", ".join(f"seed {seed} at vector step {k}" + (" (no checkpoint)" if state is None else "") for (seed, _, state), k in zip(points, steps))
        raise ValueError(f"--resume --together: the seeds of a group continue in lockstep from one vector step, but {where}; resume without --together (the "
                         "seeds one after the other), which always works")
    return steps[0] if steps else 0


def exploration_rate(it, plan):
    """sb3 get_linear_fn(1.0, 0.05, 0.1) of the run's progress at vector step `it`."""
    progress = it / max(1, plan["vector_steps"])
    if progress > EXPLORATION_FRACTION:
        return EPS_FINAL
    return EPS_INITIAL + progress * (EPS_FINAL - EPS_INITIAL) / EXPLORATION_FRACTION


def evaluation_from_rollout(tr, discount, energy_tab, dt, N):
    """`evaluate`'s result dict from the traces (numpy [T][n] reward / done / info / action) of its episodes, whichever way they were produced:
    `episodes.tally`'s numbers as arrays."""
    from .episodes import tally
    tl = tally(tr["reward"], tr["done"], tr["info"], tr["action"], discount, energy_tab)
    return dict(rewards=tl["ret"], successes=tl["last_info"] == 4, times=np.array([dt * N * l for l in tl["length"]], dtype=np.float64),
                energies=tl["energy"], actions=tl["actions"])


def evaluate(agent, eval_env, eval_config, max_steps=1000, one_launch=False):
    """The greedy DQN on the evaluation worlds, stepped side by side on the GPU (as IQNAgent.evaluation_vec).
    `one_launch`: every episode in one mn_rollout_dqn launch (DQNPolicy.rollout) instead of a Python iteration per step -- the same dict, bit for
    bit; where the policy does not act through the fused kernel the loop runs."""
    from .episodes import EPISODE_TRACES, energy_table, host_traces, loop_episodes
    from .marinenav_env.vec_env import VecMarineNavEnv
    cfgs = list(eval_config.values())
    r0 = cfgs[0]["robot"]
    eval_env.set_attrs(N=r0["N"], dt=r0["dt"])
    obs = eval_env.load_worlds([VecMarineNavEnv.world_from_eval_config(c) for c in cfgs]).clone()
    tr = agent.policy.rollout(eval_env, max_steps, trace=EPISODE_TRACES) if one_launch else None
    if tr is None:
        tr = loop_episodes(eval_env, obs, lambda t, o: agent.policy.act_batch(o), max_steps)
    return evaluation_from_rollout(host_traces(tr), eval_env.discount, energy_table(r0["a"], r0["w"]), r0["dt"], r0["N"])


def save_state_zip(state_dict, path):
    """An sb3-style checkpoint zip holding `state_dict` as policy.pth."""
    import torch
    buf = io.BytesIO()
    torch.save({k: v.cpu() for k, v in state_dict.items()}, buf)
    with zipfile.ZipFile(path, "w") as z:
        z.writestr("policy.pth", buf.getvalue())


def save_zip(agent, path):
    """An sb3-style checkpoint zip holding policy.pth (q_net.* and q_net_target.*): what DQNPolicy.load / DQNAgent.load read."""
    save_state_zip(agent.state_dict(), path)


def write_evaluations(exp_dir, log):
    """evaluations.npz of the sb3 fork's EvalCallback from the lists of `log` (timesteps, rewards, times, energies, successes, actions)."""
    actions = np.empty(len(log["actions"]), dtype=object)
    actions[:] = log["actions"]
    np.savez(os.path.join(exp_dir, "evaluations.npz"), timesteps=np.array(log["timesteps"], dtype=np.int64),
             rewards=np.array(log["rewards"], dtype=np.float64), times=np.array(log["times"], dtype=np.float64),
             energies=np.array(log["energies"], dtype=np.float64), successes=np.array(log["successes"], dtype=bool),
             actions=actions)


class TrialRun:
    """One trial of the config grid, set up and ready to be driven vector step by vector step: what `run_trial` and `run_trials_together` share.  A vector
    step of a trial is `collect(it)` (act, env step, episode log, `on_step`, replay append, resets), then the gradient steps behind it (`trains_after(it)`:
    the caller runs them, alone or grouped with other trials', and counts them in `grad_steps_done`), then `evaluate_points(it)`; `finish()` closes the run."""

    def __init__(self, device, params, n_envs, batch=None, replay=None, grad_steps=None, total_grad_steps=None, n_evals=None, torch_train=False,
                 verbose=True, eval_one_launch=False, eval_deferred=False, eval_config=None, max_eval_steps=1000, env_budget="learner",
                 reference=None, episode_log=None, on_step=None, fused_collect=False, train_env=None, eval_worlds=None):
        from .dqn.agent import DQNAgent
        from .marinenav_env.vec_env import VecMarineNavEnv
        self.params, self.verbose, self.on_step, self.eval_one_launch, self.max_eval_steps = params, verbose, on_step, eval_one_launch, max_eval_steps
        self.exp_dir = exp_dir = trial_dir(params)
        ref_mode = env_budget == "reference"
        n_envs, batch, replay, plan = plan_trial(params, n_envs, batch, replay, grad_steps, total_grad_steps, n_evals, env_budget, reference)
        self.n_envs, self.batch, self.plan = n_envs, batch, plan
        self.shape = trial_shape(plan, n_envs, 1, batch, replay)      # (what a checkpoint keeps and `--resume` compares)
        if ref_mode:
            eval_deferred = eval_deferred or True      # (300 evaluation points: each only keeps the policy of the moment)
        self.eval_points = plan_eval_points(plan, n_envs) if ref_mode else None
        os.makedirs(exp_dir, exist_ok=True)
        with open(os.path.join(exp_dir, "trial_config.json"), "w+") as f:
            json.dump(dict(params, batched=self.shape), f)
        with open(os.path.join(exp_dir, "training_schedule.json"), "w+") as f:
            json.dump(TRAINING_SCHEDULE, f)
        if verbose:
            print(f"[train_dqn] seed {params['seed']}: {plan['vector_steps']} vector steps x {n_envs} envs; {plan['total_grad_steps']} grad steps of "
                  f"batch {batch} (reference: {plan['reference_grad_steps']} of 32); target copy every {plan['target_sync_grad_steps']} grad steps; "
                  f"evaluation every {plan['eval_every_vector_steps']} vector steps", flush=True)

        if train_env is None:      # (given: this seed's rows of a stacked env, run_trials_together(stack_envs=True))
            train_env = VecMarineNavEnv(n_envs, seed=params["seed"], schedule=TRAINING_SCHEDULE, timestep_scale=plan["timestep_scale"], device=device,
                                        precision="f64")
        self.train_env = train_env
        if eval_config is None:
            eval_config = create_eval_configs(device)
        if eval_worlds is not None:      # (a run at toy size: the first few of the evaluation worlds)
            eval_config = {k: eval_config[k] for k in list(eval_config)[:int(eval_worlds)]}
        self.eval_config = eval_config
        self.eval_env = VecMarineNavEnv(len(eval_config), device=device, precision="f64")
        self.agent = agent = DQNAgent(26, 9, buffer_size=replay, batch_size=batch, learning_starts=0, device=device, seed=params["seed"] + 100,
                                      fused_train=not torch_train, fused_collect=fused_collect)
        self.report_scale = params["total_timesteps"] / (plan["vector_steps"] * n_envs)      # evaluations.npz counts reference-scaled env steps
        self.log = dict(timesteps=[], rewards=[], times=[], energies=[], successes=[], actions=[])
        self.best = -np.inf
        self.t0 = t0 = time.time()
        self.deferred = None
        if eval_deferred:
            from .dqn.deferred_eval import DeferredEvaluations, can_defer
            if can_defer(agent):
                self.deferred = DeferredEvaluations(agent, eval_config, exp_dir, **dict(dict(max_steps=max_eval_steps, verbose=verbose, label=f"seed {params['seed']} ",
                                                                                             n_evals=plan["n_evals"], t0=t0),
                                                                                        **(eval_deferred if isinstance(eval_deferred, dict) else {})))
            else:
                print("[train_dqn] eval_deferred: the policy does not act through the fused kernel here (CPU or another net_arch); evaluations stay inline", flush=True)
        self.ep_log = make_episode_log(episode_log, env_budget, n_envs, plan["eval_every_vector_steps"], self.train_env.discount, device)
        self.n_points = 0
        self.obs = self.train_env.reset()
        self.grad_steps_done = 0
        # run_trials_together with checkpoints: the process's global generators belong to no single seed there, so a seed's checkpoint records them as they
        # stood behind THIS seed's constructor -- where its sequential run, whose loop draws nothing from them, still finds them at every checkpoint
        self.global_rng = None

    def collect(self, it):
        """Act, step the envs, log, append the transitions to the replay ring, reset the finished envs."""
        agent, train_env, obs = self.agent, self.train_env, self.obs
        eps = exploration_rate(it, self.plan)
        a = agent.act_batch(obs, eps)
        fused = agent.uses_fused_collect()
        if fused:      # the step kernel appends the transitions itself
            nxt, reward, done, info = train_env.step_append(a, obs, agent.memory)
        else:
            nxt, reward, done, info = train_env.step(a)
        if self.ep_log is not None:
            self.ep_log.step(reward, done, info, it, eps)
        if self.on_step is not None:
            self.on_step(it, dict(last=dict(reward=reward, done=done, info=info, eps=eps)))
        if not fused:
            agent.memory.add_vector_step(obs, a, reward, nxt, done)
        self.obs = train_env.reset_done()
        agent.num_timesteps += self.n_envs

    def collect_given(self, it, obs, reward, done, info):
        """What is left of `collect(it)` when the act, the env step, the append and the resets were made for this seed's rows of a stacked env
        (`run_trials_together(stack_envs=True)`): the episode log, `on_step`, the timestep count.  `obs`: the rows' observations after the resets."""
        eps = exploration_rate(it, self.plan)
        if self.ep_log is not None:
            self.ep_log.step(reward, done, info, it, eps)
        if self.on_step is not None:
            self.on_step(it, dict(last=dict(reward=reward, done=done, info=info, eps=eps)))
        self.obs = obs
        self.agent.num_timesteps += self.n_envs

    def trains_after(self, it):
        """Whether gradient steps follow vector step `it` (behind `collect(it)`): plan["grad_steps_per_vector_step"] of them, cut at the target copies that
        fall every plan["target_sync_grad_steps"]."""
        return it + 1 >= self.plan["learning_starts_vector_steps"] and len(self.agent.memory) >= self.batch

    def evaluate_points(self, it):
        """The evaluation points (inline or deferred) and the episode-log rows behind vector step `it` and its gradient steps."""
        plan, params, agent, n_envs, ep_log, log, exp_dir = self.plan, self.params, self.agent, self.n_envs, self.ep_log, self.log, self.exp_dir
        if self.eval_points is not None:
            points = self.eval_points.get(it, ())
        elif ((it + 1) % plan["eval_every_vector_steps"] == 0 or it + 1 == plan["vector_steps"]) and self.n_points < plan["n_evals"]:
            points = (int(round((it + 1) * n_envs * self.report_scale)),)
        else:
            points = ()
        if ep_log is not None:
            if len(points):      # a summary row per evaluation interval, the evaluation's timestep on it
                ep_log.drain(points[-1])
            elif ep_log.due():
                ep_log.drain(int(round((it + 1) * n_envs * self.report_scale)), row=False)
        for timestep in points:
            self.n_points += 1
            if self.deferred is not None:      # keep the policy of this moment; its episodes run with the other pending points'
                self.deferred.snapshot(timestep)
                continue
            ev = evaluate(agent, self.eval_env, self.eval_config, max_steps=self.max_eval_steps, one_launch=self.eval_one_launch)
            log["timesteps"].append(timestep)
            for k in ("rewards", "times", "energies", "successes", "actions"):
                log[k].append(ev[k])
            write_evaluations(exp_dir, log)
            save_zip(agent, os.path.join(exp_dir, "latest_model.zip"))
            mean_r = float(np.mean(ev["rewards"]))
            if mean_r > self.best:
                self.best = mean_r
                save_zip(agent, os.path.join(exp_dir, "best_model.zip"))
            if self.verbose:
                print(f"[train_dqn] seed {params['seed']} eval {len(log['timesteps'])}/{plan['n_evals']} at {log['timesteps'][-1]} steps: "
                      f"{int(np.sum(ev['successes']))}/{len(self.eval_config)} successes, mean return {mean_r:.2f} ({time.time() - self.t0:.1f} s)", flush=True)

    def finish(self):
        import torch
        if self.deferred is not None:
            self.deferred.flush()
            self.deferred.close()
        if self.ep_log is not None:
            if self.ep_log.row_open:      # (what ended behind the last evaluation point)
                self.ep_log.drain(int(round(self.plan["vector_steps"] * self.n_envs * self.report_scale)))
            self.ep_log.close()
            self.ep_log.save(self.exp_dir)
        torch.cuda.synchronize()
        self.train_env.close()
        self.eval_env.close()
        with open(os.path.join(self.exp_dir, COMPLETED_FILE), "w") as f:      # last: the marker says every file of the trial is there (`--resume` skips the seed)
            json.dump(dict(vector_steps=int(self.plan["vector_steps"]), grad_steps=int(self.grad_steps_done)), f)
        return self.exp_dir

    def release(self):
        """Close the envs and wait for the device; writes nothing (`finish` without its files: a run that stopped at a checkpoint, whose deferred evaluations
        the checkpoint flushed)."""
        import torch
        if self.deferred is not None:
            self.deferred.close()
        self.train_env.close()
        self.eval_env.close()
        torch.cuda.synchronize()

    # ---- checkpoints (--checkpoint-every, --stop-after, --resume) -------------------------------------------------------------------
    def own_state(self):
        """TrialRun's own words behind a finished vector step: the observation rows the next act reads, the gradient steps done, the evaluation points
        taken, and the inline evaluations' record and best mean reward.  CPU tensors, numpy arrays and plain values."""
        import copy
        return dict(obs=self.obs.detach().cpu().clone(), grad_steps_done=int(self.grad_steps_done), n_points=int(self.n_points), log=copy.deepcopy(self.log),
                    best=float(self.best))

    def load_own_state(self, sd):
        import copy
        self.obs.copy_(sd["obs"])
        self.grad_steps_done, self.n_points = int(sd["grad_steps_done"]), int(sd["n_points"])
        self.log, self.best = copy.deepcopy(sd["log"]), float(sd["best"])

    def checkpoint_state(self, next_step, run_args=None):
        """The whole trial behind vector step `next_step - 1` as one dict of CPU tensors and plain values.  Order matters: the env first (its save settles an
        owed reset, so the observation rows saved are final), then the deferred evaluations (flushed: that writes their files) and the episode log, then
        the ring, the agent last."""
        env = self.train_env.state_dict()      # (the evaluation env is not state: every evaluation loads its worlds afresh and draws nothing)
        deferred = None if self.deferred is None else self.deferred.state_dict()
        ep_log = None if self.ep_log is None else self.ep_log.state_dict()
        return dict(format=CHECKPOINT_FORMAT, vector_step=int(next_step), params=dict(self.params), plan=dict(self.shape), args=dict(run_args or {}),
                    env=env, deferred=deferred, episode_log=ep_log, run=self.own_state(), ring=self.agent.memory.state_dict(),
                    agent=dict(self.agent.train_state_dict(), **(self.global_rng or {})))

    def restore(self, state):
        """`checkpoint_state` back into this (freshly built) trial.  Returns the vector step to continue with.  The agent comes last: its state holds torch's
        generator states, which nothing behind it may move."""
        if (state["deferred"] is None) != (self.deferred is None) or (state["episode_log"] is None) != (self.ep_log is None):
            raise ValueError("TrialRun.restore: the saved trial and this one differ in their deferred evaluations or their episode log")
        self.train_env.load_state_dict(state["env"])
        if self.deferred is not None:
            self.deferred.load_state_dict(state["deferred"])
        if self.ep_log is not None:
            self.ep_log.load_state_dict(state["episode_log"])
        self.agent.memory.load_state_dict(state["ring"])
        self.obs = self.train_env.obs
        self.load_own_state(state["run"])
        self.agent.load_train_state_dict(state["agent"])
        return int(state["vector_step"])


def run_trial(device, params, n_envs, batch=None, replay=None, grad_steps=None, total_grad_steps=None, n_evals=None, torch_train=False,
              verbose=True, eval_one_launch=False, eval_deferred=False, eval_config=None, max_eval_steps=1000, return_agent=False, env_budget="learner",
              reference=None, episode_log=None, on_step=None, train_steps_per_call="auto", fused_collect=False, eval_worlds=None, checkpoint_every=None,
              stop_after=None, resume=False, dump_final_state=None):
    """train_sb3_model.py on the vector env for one trial of the config grid; returns the trial directory (`return_agent`: and the agent).
    `eval_one_launch`: each evaluation as one mn_rollout_dqn launch instead of one Python iteration per env step (same results).
    `eval_deferred` (True, or a dict of DeferredEvaluations arguments such as max_pending): an evaluation point keeps the policy of the moment and the
    episodes of all pending points run as one mn_rollout_dqn_groups launch (dqn/deferred_eval.py) -- the same files as the inline form; where the policy
    does not act through the fused kernel (CPU, another net_arch) one line says so and the evaluations stay inline.
    `eval_config`: the evaluation worlds (default: the 30 of create_eval_configs); `max_eval_steps`: the step limit of an evaluation episode.
    `env_budget`, `reference`, `episode_log`: as train_iqn.run_trial's -- "reference" is the reference's env-step budget (`make_plan`), with deferred
    evaluations at its evaluation timesteps and the training-episode log on.  `on_step(it, dict(last=dict(reward, done, info, eps)))`: a hook behind
    every vector step (device tensors).
    `train_steps_per_call` (`steps_per_call`): 1 -- one `agent.train()` per gradient step; "multi" -- the gradient steps behind a vector step as multi-step
    calls (`DQNAgent.train_many`), one per stretch between target copies (at batch <= 32 on the fused path one HIP call each, elsewhere the loop); K > 1 -- the
    same with at most K steps per call; "auto" -- AUTO_TRAIN_STEPS_PER_CALL.  The same files either way.
    `fused_collect`: the collect phase on the device (`DQNAgent(fused_collect=True)`): one exploring act launch with the library's draws, the append inside
    the env step.  Other exploration draws than the default's, so other files.
    `eval_worlds`: evaluate on the first so many evaluation worlds only (runs at toy size).
    `checkpoint_every` = K: behind every K-th vector step -- behind its evaluation points -- the whole trial goes into checkpoint.pt of the trial's directory
    (`TrialRun.checkpoint_state`, `train_iqn.write_checkpoint`: atomically, the previous one kept as checkpoint.prev.pt); `stop_after` = K: a checkpoint behind
    vector step K, where the trial then ends without its final files and without completed.json; `resume`: skip the trial if its directory holds
    completed.json, continue from its checkpoint if it holds one (refused if that was written under another plan or other run-shaping arguments,
    `run_shaping_args`), start from the beginning otherwise.  A run stopped and resumed on the same gradient-step path writes the files of the
    uninterrupted run; a checkpoint of one path continues on the other as a valid run (eager Adam and the fused step differ in the last bits).  Without the
    three the loop does nothing it did not do before.
    `dump_final_state`: a file for torch.save(dict(env=, ring=, agent=)) of the states behind the last vector step (tests)."""
    from .dqn.agent import split_at_target_sync
    per_call = steps_per_call(train_steps_per_call)
    checkpointing = checkpoint_every is not None or stop_after is not None or resume
    if checkpoint_every is not None and int(checkpoint_every) < 1 or stop_after is not None and int(stop_after) < 1:
        raise ValueError("checkpoint_every and stop_after count vector steps: at least 1")
    run_args = run_shaping_args(env_budget=env_budget, fused_collect=fused_collect, eval_deferred=eval_deferred, eval_one_launch=eval_one_launch,
                                episode_log=episode_log, max_eval_steps=max_eval_steps, reference=reference, eval_worlds=eval_worlds)
    state = None
    if resume:      # (looked at before anything is built or written: a finished seed is left alone, a foreign checkpoint refused)
        exp_dir = trial_dir(params)
        ne, b, r, plan = plan_trial(params, n_envs, batch, replay, grad_steps, total_grad_steps, n_evals, env_budget, reference)
        what, state, name = resume_point(exp_dir, trial_shape(plan, ne, 1, b, r), run_args, log=_log)
        if what == "completed":
            print(f"[train_dqn] seed {params['seed']}: {exp_dir} holds {COMPLETED_FILE}, nothing to do", flush=True)
            return (exp_dir, None) if return_agent else exp_dir
        if verbose:
            print(f"[train_dqn] seed {params['seed']}: " + (f"continuing from vector step {state['vector_step']} ({name})" if state is not None
                                                            else "no checkpoint, starting from the beginning"), flush=True)
    run = TrialRun(device, params, n_envs, batch=batch, replay=replay, grad_steps=grad_steps, total_grad_steps=total_grad_steps, n_evals=n_evals,
                   torch_train=torch_train, verbose=verbose, eval_one_launch=eval_one_launch, eval_deferred=eval_deferred, eval_config=eval_config,
                   max_eval_steps=max_eval_steps, env_budget=env_budget, reference=reference, episode_log=episode_log, on_step=on_step,
                   fused_collect=fused_collect, eval_worlds=eval_worlds)
    agent, plan = run.agent, run.plan
    G, sync_every = plan["grad_steps_per_vector_step"], plan["target_sync_grad_steps"]
    first = run.restore(state) if state is not None else 0
    saved_args = dict(run_args, torch_train=bool(torch_train), train_steps_per_call=str(train_steps_per_call))
    for it in range(first, plan["vector_steps"]):
        run.collect(it)
        if run.trains_after(it):
            for steps, sync_after in split_at_target_sync(run.grad_steps_done, G, sync_every):
                if per_call == 1:
                    for _ in range(steps):
                        agent.train()
                else:
                    for k0 in range(0, steps, per_call or steps):
                        agent.train_many(min(per_call or steps, steps - k0))
                run.grad_steps_done += steps
                if sync_after:
                    agent.sync_target()
        run.evaluate_points(it)
        if checkpointing and checkpoint_behind(run, it + 1, checkpoint_every, stop_after, saved_args):
            run.release()
            print(stopped_line(run, it + 1), flush=True)
            return (run.exp_dir, agent) if return_agent else run.exp_dir
    if dump_final_state is not None:
        import torch
        torch.save(dict(env=run.train_env.state_dict(), ring=agent.memory.state_dict(), agent=agent.train_state_dict()), dump_final_state)
    exp_dir = run.finish()
    return (exp_dir, agent) if return_agent else exp_dir


def checkpoint_behind(run, done, checkpoint_every, stop_after, saved_args):
    """Behind vector step `done` (1-based count) of `run`: write its checkpoint if `checkpoint_every` or `stop_after` asks for one.  Returns whether the
    run stops here (`stop_after` = `done`, short of the plan's last vector step: a K at or beyond it stops nothing)."""
    stop = stop_after is not None and done == int(stop_after) and done < run.plan["vector_steps"]
    if stop or (checkpoint_every and done % int(checkpoint_every) == 0):
        write_checkpoint(run.exp_dir, run.checkpoint_state(done, saved_args))
    return stop


def stopped_line(run, done):
    return (f"[train_dqn] seed {run.params['seed']}: stopped after vector step {done} of {run.plan['vector_steps']}; checkpoint in "
            f"{os.path.join(run.exp_dir, CHECKPOINT_FILE)} (continue with --resume {os.path.dirname(run.exp_dir)})")


def group_trials(trials, limit=None):
    """The trials of a config grid that can train together: lists of indices into `trials`, in order, each of trials that differ only in their seed (hence
    share a plan), at most `limit` (default MN_DQN_MAX_LEARNERS = 64) to a list."""
    if limit is None:
        from ._capi import DQN_MAX_LEARNERS as limit
    by_key = {}
    for i, p in enumerate(trials):
        key = json.dumps({k: v for k, v in p.items() if k != "seed"}, sort_keys=True, default=str)
        by_key.setdefault(key, []).append(i)
    return [idx[k:k + limit] for idx in by_key.values() for k in range(0, len(idx), limit)]


TOGETHER_REFUSALS = dict(
    torch_train="--together needs the fused HIP gradient step: there is no grouped form of the eager PyTorch step (--torch-train)",
    stack_envs="--stack-envs stacks the envs of seeds that train together in one handle; it needs --together")


def stacked_train_env(device, trials, n_envs, env_budget="learner", batch=None, replay=None, grad_steps=None, total_grad_steps=None, n_evals=None, reference=None):
    """The ONE train env of trials that train together with stacked envs, and the rows per seed: `VecMarineNavEnv(G n, ...)` whose rows [g n, (g + 1) n)
    are seeded, scheduled and scaled as trial g's own env of n rows is (`TrialRun`), so every row steps and resets as it does there."""
    from .marinenav_env.vec_env import VecMarineNavEnv, stacked_seeds
    n, batch, replay = resolve_budget_args(env_budget, n_envs, batch, replay)
    plan = make_plan(trials[0], n, batch, grad_steps, total_grad_steps, n_evals, budget=env_budget, reference=reference)
    env = VecMarineNavEnv(len(trials) * n, seeds=stacked_seeds(n, [t["seed"] for t in trials]), schedule=TRAINING_SCHEDULE, timestep_scale=plan["timestep_scale"],
                          device=device, precision="f64")
    return env, n


def run_trials_together(device, trials, n_envs, torch_train=False, on_step=None, return_agents=False, train_steps_per_call="auto", stack_envs=False,
                        checkpoint_every=None, stop_after=None, resume=False, **kwargs):
    """`run_trial` for several trials that differ only in their seed (one list of `group_trials`), in LOCKSTEP: per vector step every trial collects as it
    does alone -- its own envs, agent, exploration, generator, replay ring, episode log and hook -- then the gradient steps behind that vector step run for
    ALL trials through one `LearnerGroup` (dqn/group_train.py): one launch per gradient step, or one multi-step call per stretch between target copies,
    instead of one per trial; then every trial handles its evaluation points.  Every learner is bit for bit what it is alone, so each seed's directory
    holds what `run_trial` writes, with the same contents.  `on_step`: None or one hook per trial.  `train_steps_per_call` and the other arguments as
    `run_trial`'s.  Returns the trial directories (`return_agents`: and the agents).
    `stack_envs` (implies `fused_collect`): the collect phase is shared too -- the seeds' envs are the rows of ONE handle (`stacked_train_env`) and per vector
    step there is one act launch at the common exploration rate, one env step, one append into all rings and one reset launch (dqn/group_collect.py:
    `CollectorGroup`) instead of one chain per seed; every seed then finishes the step on its own rows (`TrialRun.collect_given`).  Every seed's files are
    what `run_trial(fused_collect=True)` writes.
    `checkpoint_every`, `stop_after`, `resume` (per-seed envs only: refused with `stack_envs`, CHECKPOINT_REFUSALS): every learner and every env is bit for
    bit what it is alone, so behind lockstep vector step k every seed writes ITS OWN checkpoint.pt into its own directory -- the dict the sequential run
    writes at k -- and a run stopped here resumes sequentially, and the other way round.  `resume`: completed seeds leave the group (a group of one runs as
    `run_trial`); the others must all be at the start or all hold checkpoints of ONE vector step (`check_lockstep`), which is refused before anything is
    built or written otherwise.  A stopped run returns the trial directories as a finished one does."""
    import torch
    from .dqn.agent import split_at_target_sync
    from .dqn.group_train import LearnerGroup
    if torch_train:
        raise ValueError("training trials together needs the fused gradient step: there is no grouped form of the eager PyTorch step (torch_train)")
    checkpointing = checkpoint_every is not None or stop_after is not None or resume
    if checkpointing and stack_envs:
        raise ValueError(CHECKPOINT_REFUSALS["stack_envs"])
    if checkpoint_every is not None and int(checkpoint_every) < 1 or stop_after is not None and int(stop_after) < 1:
        raise ValueError("checkpoint_every and stop_after count vector steps: at least 1")
    if stack_envs and torch.device(device).type != "cuda":
        raise ValueError(f"stack_envs: the stacked collect runs on HIP kernels; device {device} has none")
    trials = list(trials)
    if len(group_trials(trials)) != 1:
        raise ValueError("trials that train together differ only in their seed, and are at most 64 (group_trials)")
    per_call = steps_per_call(train_steps_per_call)
    hooks = list(on_step) if on_step is not None else [None] * len(trials)
    run_args = run_shaping_args(**kwargs)
    states, all_dirs, all_agents = [None] * len(trials), [trial_dir(p) for p in trials], [None] * len(trials)
    if resume:      # (looked at before anything is built or written)
        plan_kw = {k: kwargs.get(k) for k in ("batch", "replay", "grad_steps", "total_grad_steps", "n_evals", "reference")}
        ne, b, r, plan = plan_trial(trials[0], n_envs, env_budget=kwargs.get("env_budget", "learner"), **plan_kw)
        shape = trial_shape(plan, ne, 1, b, r)
        points = [(p["seed"],) + resume_point(d, shape, run_args, log=_log)[:2] for p, d in zip(trials, all_dirs)]
        left = [i for i, pt in enumerate(points) if pt[1] != "completed"]
        for i, pt in enumerate(points):
            if pt[1] == "completed":
                print(f"[train_dqn] seed {pt[0]}: {all_dirs[i]} holds {COMPLETED_FILE}, nothing to do", flush=True)
        first = check_lockstep([points[i] for i in left])
        if len(left) <= 1:      # a group of one runs as run_trial (which looks at its directory again)
            for i in left:
                out = run_trial(device, trials[i], n_envs, on_step=hooks[i], return_agent=True, train_steps_per_call=train_steps_per_call,
                                checkpoint_every=checkpoint_every, stop_after=stop_after, resume=True, **kwargs)
                all_agents[i] = out[1]
            return (all_dirs, all_agents) if return_agents else all_dirs
        if kwargs.get("verbose", True):
            seeds = [points[i][0] for i in left]
            print(f"[train_dqn] seeds {seeds}: " + (f"continuing from vector step {first} (their checkpoints)" if first else "no checkpoints, starting from the beginning"),
                  flush=True)
        states = [points[i][2] for i in left]
        keep = left
        trials, hooks = [trials[i] for i in keep], [hooks[i] for i in keep]
    else:
        keep = list(range(len(trials)))
    saved_args = dict(run_args, torch_train=False, train_steps_per_call=str(train_steps_per_call))
    stacked, views, collectors = None, [None] * len(trials), None
    if stack_envs:
        from .dqn.group_collect import CollectorGroup
        from .marinenav_env.vec_env import StackedRows
        kwargs["fused_collect"] = True
        env_kw = {k: kwargs[k] for k in ("env_budget", "batch", "replay", "grad_steps", "total_grad_steps", "n_evals", "reference") if k in kwargs}
        stacked, n_rows = stacked_train_env(device, trials, n_envs, **env_kw)
        views = [StackedRows(stacked, g, n_rows) for g in range(len(trials))]
    runs = []
    for p, h, v in zip(trials, hooks, views):
        runs.append(TrialRun(device, p, n_envs, on_step=h, train_env=v, **kwargs))
        if checkpointing:
            runs[-1].global_rng = runs[-1].agent.global_rng_state()
    plan = runs[0].plan
    assert all(r.plan == plan for r in runs)
    group = LearnerGroup([r.agent for r in runs])
    if stack_envs:      # (behind the LearnerGroup: the fused trainer it makes re-allocates the networks' parameters into its flat buffers)
        collectors = CollectorGroup([r.agent for r in runs], stacked)
        obs = stacked.obs
    G, sync_every = plan["grad_steps_per_vector_step"], plan["target_sync_grad_steps"]
    done, first = 0, 0
    if any(st is not None for st in states):      # (behind the LearnerGroup: every learner's state goes IN PLACE into the buffers its device table names)
        firsts = [r.restore(st) for r, st in zip(runs, states)]
        for r, st in zip(runs, states):
            r.global_rng = {k: st["agent"][k] for k in ("torch_cpu_rng", "torch_device_rng", "py_random")}
        first, done = firsts[0], runs[0].grad_steps_done
        assert all(f == first for f in firsts) and all(r.grad_steps_done == done for r in runs), (firsts, [r.grad_steps_done for r in runs])
    for it in range(first, plan["vector_steps"]):
        if stack_envs:
            actions = collectors.act(obs, exploration_rate(it, plan))
            next_obs, reward, ended, info = stacked.step(actions)
            collectors.append(obs, actions, reward, next_obs, ended)
            obs = stacked.reset_done()
            for r, v in zip(runs, views):
                r.collect_given(it, obs[v.rows], reward[v.rows], ended[v.rows], info[v.rows])
        else:
            for r in runs:
                r.collect(it)
        trains = [r.trains_after(it) for r in runs]
        assert all(t == trains[0] for t in trains)      # (equal plans, equally full rings)
        if trains[0]:
            for steps, sync_after in split_at_target_sync(done, G, sync_every):
                if per_call == 1:
                    for _ in range(steps):
                        group.train()
                else:
                    for k0 in range(0, steps, per_call or steps):
                        group.train_many(min(per_call or steps, steps - k0))
                done += steps
                if sync_after:
                    group.sync_target()
            for r in runs:
                r.grad_steps_done = done
        for r in runs:
            r.evaluate_points(it)
        if checkpointing:
            stops = [checkpoint_behind(r, it + 1, checkpoint_every, stop_after, saved_args) for r in runs]
            if stops[0]:
                for r in runs:
                    r.release()
                    print(stopped_line(r, it + 1), flush=True)
                group.close()
                for i, r in zip(keep, runs):
                    all_agents[i] = r.agent
                return (all_dirs, all_agents) if return_agents else all_dirs
    dirs = [r.finish() for r in runs]
    group.close()
    if collectors is not None:
        collectors.close()
        stacked.close()
    for i, r, d in zip(keep, runs, dirs):
        all_dirs[i], all_agents[i] = d, r.agent
    return (all_dirs, all_agents) if return_agents else all_dirs


def main(argv=None):
    ap = argparse.ArgumentParser(description="Train the DQN baseline (batched MI355X path)")
    ap.add_argument("-C", "--config-file", dest="config_file", type=open, required=True)
    ap.add_argument("-D", "--device", dest="device", type=str, default=None)
    ap.add_argument("--n-envs", type=int, default=None, help="default 4096 (--env-budget reference: env steps per vector step, default 80)")
    ap.add_argument("--batch", type=int, default=None, help="default 256 (--env-budget reference: 32, the reference's)")
    ap.add_argument("--replay", type=int, default=None, help="replay ring rows, default 100 000 (--env-budget reference: 1 000 000, the reference's)")
    ap.add_argument("--env-budget", default="learner", choices=["learner", "reference"],
                    help="learner (default): the reference's learner budget in big batches -- the fast mode; reference: the reference's own experiment -- total_timesteps "
                         "env steps, one batch-32 gradient step per env step after learning_starts, its target cadence and evaluation timesteps (deferred evaluations, "
                         "episode log on) -- the drop-in mode; an explicit value that contradicts it is an error")
    ap.add_argument("--episode-log", nargs="?", const=True, default=None, choices=["full"],
                    help="training_log.npz: one summary row of the training episodes per evaluation interval, from a device-side log; `--episode-log full`: "
                         "training_episodes.npz with every episode's record too.  Default: off (on with --env-budget reference)")
    ap.add_argument("--grad-steps", type=int, default=None, help="gradient steps per vector step (default: one per 4 096 envs)")
    ap.add_argument("--total-grad-steps", type=int, default=None,
                    help="learner budget (default: the reference's sample count, total_timesteps x 32 / batch)")
    ap.add_argument("--n-evals", type=int, default=None, help="evaluation points over the run (default: min(30, total_timesteps / eval_freq))")
    ap.add_argument("--torch-train", action="store_true", help="eager PyTorch gradient step instead of the fused HIP kernel")
    ap.add_argument("--train-steps-per-call", default="auto", metavar="{auto,1,K,multi}",
                    help="1: one launch per gradient step; multi: the gradient steps behind a vector step as multi-step calls, cut at the target copies -- at "
                         "batch <= 32 on the fused path one mn_dqn_train_steps call each, elsewhere the loop; K > 1: the same, at most K steps per call; auto "
                         "(default): 1 until the multi-step call is measured faster (README).  The run's files are bit-equal either way")
    ap.add_argument("--eval-one-launch", action="store_true",
                    help="run each evaluation's episodes in one HIP launch (mn_rollout_dqn) instead of one Python iteration per env step; same results")
    ap.add_argument("--eval-deferred", action="store_true",
                    help="evaluations: a point only keeps the policy of the moment; all pending points run later as ONE mn_rollout_dqn_groups launch and are "
                         "logged as the inline form logs them (the same files); with --n-evals 300 the reference's evaluation density")
    ap.add_argument("--together", action="store_true",
                    help="train the trials that differ only in their seed in lockstep, up to 64 at a time: their gradient steps share ONE launch per step (or one "
                         "multi-step call per stretch, with --train-steps-per-call multi / K) through mn_dqn_group_train_step[s]; every seed's files equal the "
                         "sequential run's.  Needs the fused gradient step (not --torch-train); a trial without companions runs as without the option")
    ap.add_argument("--fused-collect", action="store_true",
                    help="collect on the device: ONE act launch that draws the exploration itself (mn_dqn_act_rng, the library's counter-based generator "
                         "instead of torch.Generator: other draws) and the replay append inside the env step (mn_step_append)")
    ap.add_argument("--stack-envs", action="store_true",
                    help="with --together: the envs of the seeds that train together are the rows of ONE handle, and each vector step is one act, one step, one "
                         "append and one reset launch for all of them; implies --fused-collect, and every seed's files equal its own --fused-collect run's")
    ap.add_argument("--dry-run", action="store_true", help="print the plan of every trial as JSON and exit (no GPU needed); with --together also which trials "
                                                           "would share a group")
    ap.add_argument("--checkpoint-every", type=int, default=None, metavar="K",
                    help="behind every K-th vector step write checkpoint.pt into the trial's directory (atomically; the previous one is kept as checkpoint.prev.pt): the "
                         "env handle's snapshot (mn_state_save), the replay ring, the learner (both networks, Adam, the draw counters, the generators), the "
                         "evaluations and the episode log.  With --together every seed writes its own.  Off by default: the loop then does nothing it did not do before")
    ap.add_argument("--stop-after", type=int, default=None, metavar="K",
                    help="end every trial behind vector step K with a checkpoint written at that step; exit status 0 (a time-limited session: continue with --resume).  A K "
                         "at or beyond the plan's vector steps stops nothing: the trial completes")
    ap.add_argument("--resume", default=None, metavar="TRAINING_DIR",
                    help="continue the run in save_dir/training_<time>: per seed, skip it if it holds completed.json, continue from its checkpoint.pt (checkpoint.prev.pt if "
                         "that is unreadable) or start it if it has none.  Give the command line of the original run: another plan is refused.  On the same gradient-step "
                         "path the files written equal those of the uninterrupted run.  A run stopped under --together resumes with or without it; with --together the "
                         "seeds left of a group must be at one vector step.  With --dry-run: print where every seed would continue")
    ap.add_argument("--run-name", default=None, metavar="NAME", help="name the run directory training_NAME instead of training_<start time>")
    ap.add_argument("--reference", nargs="*", default=None, metavar="KEY=VALUE",
                    help="with --env-budget reference: overrides of the reference's constants (learning_starts, target_update_interval, exploration_fraction, replay) "
                         "for runs at toy size")
    ap.add_argument("--max-eval-steps", type=int, default=1000, help="step limit of an evaluation episode (default 1000, the reference's)")
    ap.add_argument("--eval-worlds", type=int, default=None, metavar="N", help="evaluate on the first N of the 30 evaluation worlds (runs at toy size)")
    ap.add_argument("--dump-final-state", default=None, metavar="FILE",
                    help="behind the last vector step, torch.save the agent's train_state_dict() and the state_dict()s of its replay ring and the train env of the LAST "
                         "trial run to FILE (tests)")
    args = ap.parse_args(argv)
    if args.together and args.torch_train:
        raise SystemExit("train_dqn: " + TOGETHER_REFUSALS["torch_train"])
    if args.stack_envs and not args.together:
        raise SystemExit("train_dqn: " + TOGETHER_REFUSALS["stack_envs"])
    checkpointing = args.checkpoint_every is not None or args.stop_after is not None or args.resume is not None
    if checkpointing:
        if args.stack_envs:
            raise SystemExit("train_dqn: " + CHECKPOINT_REFUSALS["stack_envs"])
        if (args.checkpoint_every is not None and args.checkpoint_every < 1) or (args.stop_after is not None and args.stop_after < 1):
            raise SystemExit("train_dqn: --checkpoint-every and --stop-after count vector steps: at least 1")
    reference = None
    if args.reference is not None:
        if args.env_budget != "reference":
            raise SystemExit("train_dqn: --reference overrides belong to --env-budget reference")
        try:
            reference = {k: (float(v) if k == "exploration_fraction" else int(v)) for k, v in (kv.split("=", 1) for kv in args.reference)}
        except ValueError:
            raise SystemExit("train_dqn: --reference takes KEY=VALUE pairs with numeric values")
    if args.dump_final_state is not None and args.together:
        raise SystemExit("train_dqn: --dump-final-state dumps one trial's state; the lockstep loop of --together has none to dump")
    fused_collect = args.fused_collect or args.stack_envs
    try:
        steps_per_call(args.train_steps_per_call)
    except ValueError as e:
        raise SystemExit(f"train_dqn: {e}")
    params = json.load(args.config_file)
    stamp = args.run_name if args.run_name is not None else datetime.now().strftime("%Y-%m-%d-%H-%M-%S")
    if args.resume is not None:
        rdir = os.path.abspath(args.resume)
        if not os.path.isdir(rdir) or not os.path.basename(rdir).startswith("training_"):
            raise SystemExit(f"train_dqn: --resume takes a run directory, save_dir/training_<time>; {args.resume!r} is none")
        stamp = os.path.basename(rdir)[len("training_"):]
        for p in trial_params(params):
            if os.path.realpath(os.path.join(p["save_dir"], "training_" + stamp)) != os.path.realpath(rdir):
                raise SystemExit(f"train_dqn: --resume {args.resume}: the config's save_dir ({p['save_dir']!r}) does not lead to that directory")
    # (only what was asked for is passed on: without these options run_trial and run_trials_together are called as ever)
    more = {}
    if reference is not None:
        more["reference"] = reference
    if args.max_eval_steps != 1000:
        more["max_eval_steps"] = args.max_eval_steps
    if args.eval_worlds is not None:
        more["eval_worlds"] = args.eval_worlds
    if checkpointing:
        more.update(checkpoint_every=args.checkpoint_every, stop_after=args.stop_after, resume=args.resume is not None)
    trials = trial_params(params)
    for p in trials:
        p["training_time"] = stamp
    groups = group_trials(trials) if args.together else [[i] for i in range(len(trials))]

    def where_to_continue(emit):
        """`--resume`: every seed's resume point, checked as the run checks it -- a foreign checkpoint and, under --together, seeds of a group at different
        vector steps end the command here, before anything is built or written."""
        run_args = run_shaping_args(env_budget=args.env_budget, fused_collect=fused_collect, eval_deferred=args.eval_deferred, eval_one_launch=args.eval_one_launch,
                                    episode_log=args.episode_log, **more)
        try:
            points = []
            for p in trials:
                ne, b, r, plan = plan_trial(p, args.n_envs, args.batch, args.replay, args.grad_steps, args.total_grad_steps, args.n_evals, args.env_budget, reference)
                what, state, name = resume_point(trial_dir(p), trial_shape(plan, ne, 1, b, r), run_args, log=_log if emit is not None else (lambda line: None))
                points.append((p["seed"], what, state))
                if emit is not None:
                    emit(dict(seed=p["seed"], resume=what, vector_step=None if state is None else int(state["vector_step"]), checkpoint=name))
            for g in groups:      # (--together: the seeds left of a group continue from one vector step)
                check_lockstep([points[i] for i in g if points[i][1] != "completed"])
        except ValueError as e:
            raise SystemExit(f"train_dqn: {e}")

    if args.dry_run:
        n_envs, batch, replay = resolve_budget_args(args.env_budget, args.n_envs, args.batch, args.replay)
        for p in trials:
            try:
                plan = make_plan(p, n_envs, batch, args.grad_steps, args.total_grad_steps, args.n_evals, budget=args.env_budget, reference=reference)
                if args.env_budget == "reference" and replay is not None and replay != plan["replay"]:
                    raise ValueError(f"env_budget='reference' keeps the reference's replay ring ({plan['replay']} rows); {replay} contradicts it")
            except ValueError as e:
                raise SystemExit(f"train_dqn: {e}")
            extra = dict(env_budget=args.env_budget, episode_log=True if args.episode_log is None else args.episode_log) if args.env_budget == "reference" else {}
            print(json.dumps(dict(seed=p["seed"], n_envs=n_envs, batch=batch, replay=plan.get("replay", replay), fused=not args.torch_train,
                                  eval_one_launch=args.eval_one_launch, eval_deferred=args.eval_deferred or args.env_budget == "reference", **extra, **(dict(fused_collect=True) if fused_collect else {}), eps_start=exploration_rate(0, plan), eps_end=exploration_rate(int(np.ceil(plan["exploration_vector_steps"])), plan),
                                  plan=plan)))
        if args.resume is not None:      # where every seed would continue (reads its checkpoint on the host; the same checks as the run itself)
            where_to_continue(lambda line: print(json.dumps(line), flush=True))
        if args.together:
            stacked = lambda g: dict(stacked_env_rows=len(g) * n_envs, rows_per_seed=n_envs) if args.stack_envs and len(g) > 1 else {}
            print(json.dumps(dict(together=[dict(group=k, seeds=[trials[i]["seed"] for i in g], one_launch_per_gradient_step=len(g) > 1, **stacked(g))
                                            for k, g in enumerate(groups)])))
        return
    if args.resume is not None:
        where_to_continue(None)
    import torch
    device = "cuda:0" if args.device in (None, "cuda") else args.device
    torch.cuda.set_device(torch.device(device))
    common = dict(batch=args.batch, replay=args.replay, grad_steps=args.grad_steps, total_grad_steps=args.total_grad_steps, n_evals=args.n_evals,
                  torch_train=args.torch_train, eval_one_launch=args.eval_one_launch, eval_deferred=args.eval_deferred, env_budget=args.env_budget,
                  episode_log=args.episode_log, train_steps_per_call=args.train_steps_per_call, fused_collect=fused_collect, **more)
    for g in groups:
        t0 = time.time()
        if len(g) > 1:
            seeds = [trials[i]["seed"] for i in g]
            print(f"[train_dqn] seeds {seeds} train together: one launch per gradient step for the {len(g)} of them"
                  + (", their envs stacked in one handle" if args.stack_envs else ""), flush=True)
            dirs = run_trials_together(device, [trials[i] for i in g], args.n_envs, stack_envs=args.stack_envs, **common)
            print(f"[train_dqn] seeds {seeds}: {time.time() - t0:.1f} s -> {os.path.dirname(dirs[0])}", flush=True)
            continue
        p = trials[g[0]]
        d = run_trial(device, p, args.n_envs, **common, **(dict(dump_final_state=args.dump_final_state) if args.dump_final_state is not None else {}))
        print(f"[train_dqn] seed {p['seed']}: {time.time() - t0:.1f} s -> {d}", flush=True)


if __name__ == "__main__":
    main()
