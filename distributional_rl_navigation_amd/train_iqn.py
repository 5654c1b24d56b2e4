"""Training driver: counterpart of the reference's train_IQN_model.py (:15-179) for the batched path.

Same JSON config (`config/config_IQN.json` schema: agent, seed (list -> grid), total_timesteps,
eval_freq, save_dir), same per-trial outputs (`trial_config.json`, `training_schedule.json`,
`eval_config.json`, `greedy_evaluations.npz`, `adaptive_evaluations.npz`, `network_params.pth`,
`constructor_params.json`; `completed.json` last, the marker `--resume` skips a finished seed by).  One process per GPU: launch with torch.distributed.run for several
GPUs (independent learners per rank by default, `--shared-learner` for one IQN with an RCCL
gradient all-reduce).

    python -m distributional_rl_navigation_amd.train_iqn -C config_IQN.json [--n-envs 4096] [--env-budget reference] [--episode-log [full]] [--together [--stack-envs]] [--dry-run]
    python -m distributional_rl_navigation_amd.train_iqn -C config_IQN.json ... [--n-step N [--n-step-mode episode]]        # N-step returns; episode: windows cut at episode ends
    python -m distributional_rl_navigation_amd.train_iqn -C config_IQN.json ... [--checkpoint-every K] [--stop-after K]      # checkpoint.pt per seed; end behind vector step K
    python -m distributional_rl_navigation_amd.train_iqn -C config_IQN.json ... --resume SAVE_DIR/training_<time> [--dry-run]   # continue in a fresh process, bit for bit

Cadence.  The reference does one batch-32 gradient step per 4 env steps (replay ratio 8 sampled per generated
transition).  Two modes (`--env-budget`):
  reference  the DROP-IN: the reference's own experiment -- total_timesteps env steps in vector steps of N = 80, N / 4 batch-32 gradient
             steps behind each from learning_starts on, its target / evaluation cadence, its evaluation timesteps (10 000 ... 3 000 000),
             its 1 M-row ring; deferred evaluations and the training-episode log (episode_log.py) on.  Learner-bound (`plan_reference`).
  learner    the FAST one (default).  With 65 536 envs a vector step IS 65 536 env steps (the reference's ratio would be 16 384 gradient
steps per vector step); the batched loop instead spends the reference's LEARNER budget (750 000 x 32 samples =
93 750 gradient steps of batch 256) at G gradient steps per vector step (16 per 65 536 envs, one per 4 096: replay ratio
0.06 either way) and rescales every run-fraction cadence (exploration ramp, curriculum, evaluations) -- `plan_cadence`.

Envs per GPU.  Default 4 096 (round 6): the same env steps and learner budget cut into 93 760 vector steps of ONE
gradient step each, ring 100 000 = 24 vector steps of history.  Of the cells swept (profiles/r06_learning_curve.txt: envs
2 048 ... 65 536 x ring 100 k ... 16 M, 12-24 seeds each, 252 runs) it is the one whose LAST evaluation sits on the reference's
own final evaluation without best-checkpoint selection -- 26.1 +- 1.4 of 30 successes, mean return 68.0 +- 7.1 over 24
runs (reference: 26, 69.25) -- at 9.6 s per run on one MI355X; --n-envs 65536 (the bench's configuration: 5 860 vector
steps of 16 gradient steps) runs 6.4 s and ends 1 success / 6 return points lower (25.0 +- 1.8, 62.3 +- 11.0 over 24 runs).
"""
import argparse
import itertools
import json
import os
from datetime import datetime

import numpy as np


def trial_params(params):
    """train_IQN_model.py:52-65: list-valued keys expand to a Cartesian grid."""
    if isinstance(params, (str, int, float)):
        return [params]
    if isinstance(params, list):
        return params
    if isinstance(params, dict):
        keys, vals = zip(*params.items())
        return [dict(zip(keys, mix)) for mix in itertools.product(*[trial_params(v) for v in vals])]
    raise TypeError("Parameter type is incorrect.")


TRAINING_SCHEDULE = dict(timesteps=[0, 1000000, 2000000], num_cores=[4, 6, 8], num_obstacles=[6, 8, 10],
                         min_start_goal_dis=[30.0, 35.0, 40.0])   # train_IQN_model.py:86-90


def create_eval_configs(device, seed=348):
    """train_IQN_model.py:123-148: 30 evaluation worlds from ONE RNG stream (seed 348), fixed start/goal,
    10 x (4 cores, 6 obstacles), 10 x (6, 8), 10 x (8, 10).  Bit-identical to the reference's."""
    from .marinenav_env.env import MarineNavEnv
    env = MarineNavEnv(seed=seed, device=device)
    env.obs_r_range = [1, 3]
    env.reset_start_and_goal = False
    env.start = np.array([5.0, 5.0])
    env.goal = np.array([45.0, 45.0])
    cfg, count = {}, 0
    for nc, no in ((4, 6), (6, 8), (8, 10)):
        for _ in range(10):
            env.num_cores, env.num_obs = nc, no
            env.reset()
            cfg[f"env_{count}"] = env.episode_data()
            count += 1
    env.close()
    return cfg


REFERENCE_N_ENVS = 80      # --env-budget reference: env steps per vector step (20 IQN gradient steps each, 37 500 vector steps)
REFERENCE_DEFAULTS = dict(learning_starts=10_000, target_update_interval=10_000, exploration_fraction=0.1, replay=1_000_000)      # agent.py:10-29 / sb3 DQN


def reference_n_envs(total_timesteps, eval_freq, learning_starts, target_interval, update_every, thresholds=()):
    """Every N the reference-budget plan takes: N env steps per vector step must cut the run, `learning_starts`, the evaluation and target
    intervals and the curriculum thresholds into whole vector steps, and hold a whole number of training events (a multiple of `update_every`)."""
    from math import gcd
    g = 0
    for v in (total_timesteps, eval_freq, learning_starts, target_interval) + tuple(t for t in thresholds if t):
        g = gcd(g, int(v))
    return [d for d in range(1, g + 1) if g % d == 0 and d % update_every == 0]


def plan_reference(total_timesteps, eval_freq, n_envs_total, batch, ref_batch=32, ref_update_every=4, ref_target_interval=10_000, reference=None):
    """`plan_cadence(budget="reference")`: the reference's own experiment -- its env-step budget, its replay ratio, its cadences -- cut into
    vector steps of N = n_envs_total env steps.  Vector step k stands for the env steps [k N, (k + 1) N): it trains from the one that starts at
    `learning_starts` on, N / update_every gradient steps of the reference's batch each, (total_timesteps - learning_starts) / update_every in
    all (the reference's `<=` loop does one more).  An evaluation follows the vector step that starts at learning_starts + j eval_freq and is
    logged with that env step; one more follows the last vector step, logged with total_timesteps: eval_freq, 2 eval_freq, ...,
    total_timesteps when learning_starts = eval_freq, the reference's own list.  `reference`: overrides of REFERENCE_DEFAULTS (a run at toy size)."""
    ref = dict(REFERENCE_DEFAULTS, target_update_interval=ref_target_interval)
    unknown = set(reference or {}) - set(ref)
    if unknown:
        raise ValueError(f"reference=: unknown keys {sorted(unknown)} (known: {sorted(ref)})")
    ref.update(reference or {})
    N, ls, ti = int(n_envs_total), int(ref["learning_starts"]), int(ref["target_update_interval"])
    if batch != ref_batch:
        raise ValueError(f"budget='reference' trains with the reference's batch ({ref_batch}), not {batch}")
    valid = reference_n_envs(total_timesteps, eval_freq, ls, ti, ref_update_every, TRAINING_SCHEDULE["timesteps"])
    if N not in valid:
        near = sorted(set(([max(v for v in valid if v < N)] if any(v < N for v in valid) else []) + ([min(v for v in valid if v > N)] if any(v > N for v in valid) else [])))
        raise ValueError(f"budget='reference': {N} env steps per vector step do not divide total_timesteps ({total_timesteps}), learning_starts ({ls}), eval_freq "
                         f"({eval_freq}), the target interval ({ti}) and the curriculum thresholds into whole vector steps of whole training events (a multiple of "
                         f"{ref_update_every}); nearest valid values: {near} (all: {valid})")
    if ls >= total_timesteps:
        raise ValueError(f"budget='reference': learning_starts ({ls}) is not inside the run ({total_timesteps} timesteps)")
    V, G = total_timesteps // N, N // ref_update_every
    points = list(range(ls, total_timesteps, eval_freq)) + [total_timesteps]
    total_grad = (total_timesteps - ls) // ref_update_every
    return dict(
        vector_steps=V, grad_steps_per_vector_step=G, total_grad_steps=total_grad, reference_grad_steps=total_timesteps // ref_update_every,
        reference_samples=total_timesteps // ref_update_every * ref_batch, samples=total_grad * ref_batch, env_steps=total_timesteps,
        target_sync_grad_steps=ti // ref_update_every, eval_every_vector_steps=eval_freq // N, n_evals=len(points), timestep_scale=float(N),
        replay_ratio=G * ref_batch / N, reference_replay_ratio=ref_batch / ref_update_every,
        budget="reference", batch=ref_batch, learning_starts=ls, learning_starts_vector_steps=ls // N, exploration_fraction=ref["exploration_fraction"],
        exploration_timesteps=int(round(ref["exploration_fraction"] * total_timesteps)), replay=int(ref["replay"]), report_timestep_scale=1,
        eval_timesteps=points)


def plan_eval_points(plan, n_envs_total):
    """{vector step: [timesteps to log]} of a reference-budget plan: the evaluations that follow that vector step."""
    after = {}
    for t in plan["eval_timesteps"]:
        after.setdefault(min(t // n_envs_total, plan["vector_steps"] - 1), []).append(t)
    return after


def plan_cadence(total_timesteps, eval_freq, n_envs_total, batch, ref_batch=32, ref_update_every=4,
                 ref_target_interval=10_000, grad_steps_per_vector_step=None, total_grad_steps=None, n_evals=None, budget="learner", reference=None):
    """Translate the reference's env-step cadences (config_IQN.json + agent.py defaults: 3 M timesteps, one batch-32
    gradient step every 4 env steps, target copy every 10 000 learning steps, evaluation every 10 000) into the
    batched loop's units.

    The reference consumes total_timesteps / 4 gradient steps x 32 samples.  A vector step is n_envs_total env steps
    at once, so the batched loop cannot keep the reference's replay ratio (that would be n_envs_total / 4 gradient
    steps per vector step); it keeps the reference's LEARNER budget instead -- the same number of sampled transitions,
    total_grad_steps = total_timesteps / 4 * 32 / batch -- and spreads it over as many vector steps as the chosen
    gradient-steps-per-vector-step G needs.  Everything that the reference expresses as a fraction of the run
    (exploration ramp, curriculum stages, evaluation points) keeps its fraction.
    Returns a dict; `replay_ratio` = sampled transitions per generated env step (reference: 8).

    `budget`: "learner" (default) is the above.  "reference" keeps the reference's ENV-STEP budget instead -- total_timesteps env steps at its own
    replay ratio, batch and cadences (`plan_reference`; `reference`: overrides of its constants): the drop-in experiment, learner-bound."""
    if budget == "reference":
        given = dict(grad_steps_per_vector_step=grad_steps_per_vector_step, total_grad_steps=total_grad_steps, n_evals=n_evals)
        plan = plan_reference(total_timesteps, eval_freq, n_envs_total, batch, ref_batch, ref_update_every, ref_target_interval, reference)
        for k, v in given.items():
            if v is not None and int(v) != plan[k]:
                raise ValueError(f"budget='reference' fixes {k} = {plan[k]}; {v} contradicts it")
        return plan
    if budget != "learner":
        raise ValueError(f"budget={budget!r}: 'learner' or 'reference'")
    if reference:
        raise ValueError("reference= overrides belong to budget='reference'")
    ref_grad_steps = total_timesteps // ref_update_every
    if total_grad_steps is None:
        total_grad_steps = max(1, int(round(ref_grad_steps * ref_batch / batch)))
    if grad_steps_per_vector_step is None:
        # keep the learner at roughly half of the GPU time: one fused grad step ~ 57 us, one vector step ~ 16 ns / env
        grad_steps_per_vector_step = int(min(32, max(1, round(n_envs_total / 65536 * 16))))
    G = int(grad_steps_per_vector_step)
    vector_steps = int(np.ceil(total_grad_steps / G))
    if n_evals is None:
        n_evals = int(min(30, max(1, total_timesteps // max(1, eval_freq))))
    plan = dict(
        vector_steps=vector_steps, grad_steps_per_vector_step=G, total_grad_steps=vector_steps * G,
        reference_grad_steps=ref_grad_steps, reference_samples=ref_grad_steps * ref_batch, samples=vector_steps * G * batch,
        env_steps=vector_steps * n_envs_total,
        # target copy every 10 000 learning steps = 2 500 gradient steps x 32 samples -> same number of samples
        target_sync_grad_steps=max(50, int(round(ref_target_interval / ref_update_every * ref_batch / batch))),
        eval_every_vector_steps=max(1, vector_steps // n_evals), n_evals=n_evals,
        # env.total_timesteps counts vector steps per env; the curriculum (and eps) see reference-scaled time
        timestep_scale=total_timesteps / vector_steps,
        replay_ratio=G * batch / n_envs_total, reference_replay_ratio=ref_batch / ref_update_every)
    return plan


def resolve_budget_args(env_budget, n_envs, batch, replay, default_n_envs=4096):
    """(n_envs, batch, replay) with the defaults of the budget filled in for what was left None: learner 4 096 envs / batch 256 / ring 100 000;
    reference REFERENCE_N_ENVS / the reference's batch 32 / its ring (a contradicting explicit value is refused by the plan)."""
    if env_budget == "reference":
        return (REFERENCE_N_ENVS if n_envs is None else n_envs, 32 if batch is None else batch, replay)
    return (default_n_envs if n_envs is None else n_envs, 256 if batch is None else batch, 100_000 if replay is None else replay)


def make_episode_log(option, env_budget, n_envs, eval_every_vector_steps, discount, device, max_records=1 << 20):
    """The EpisodeLog of a trial, or None.  `option`: None = the budget's default (on with "reference", off with "learner"), False, True, or "full".
    Capacity: n_envs x the vector steps of one evaluation interval (an env ends at most one episode per vector step), at most `max_records` rows
    (the loop then drains inside the interval as well)."""
    if option is None:
        option = env_budget == "reference"
    if not option:
        return None
    from .episode_log import EpisodeLog
    steps = max(1, min(int(eval_every_vector_steps) + 1, max_records // n_envs))
    return EpisodeLog(n_envs, n_envs * steps, discount, device, full=option == "full")


def trial_dir(params, rank=0, world=1, shared=False):
    """The directory of one trial: save_dir/training_<time>/seed_<seed> (train_IQN_model.py:76-78), one per rank for independent learners."""
    exp_dir = os.path.join(params["save_dir"], "training_" + params["training_time"], "seed_" + str(params["seed"]))
    return os.path.join(exp_dir, f"rank_{rank}") if world > 1 and not shared else exp_dir


def plan_trial(params, n_envs, world=1, shared=False, batch=None, replay=None, grad_steps=None, total_grad_steps=None, n_evals=None, env_budget="learner",
               reference=None):
    """(n_envs, batch, replay, plan) of one trial: the budget's defaults filled in, `plan_cadence`, and the checks every trial passes before anything is
    written or allocated.  No GPU needed: `--dry-run` and `--resume` plan with it as `TrialRun` does."""
    ref_mode = env_budget == "reference"
    if ref_mode and (world > 1 or shared):
        raise ValueError("env_budget='reference' is the reference's single-learner experiment: one process, one GPU")
    n_envs, batch, replay = resolve_budget_args(env_budget, n_envs, batch, replay)
    plan = plan_cadence(params["total_timesteps"], params["eval_freq"], n_envs * world, batch,
                        grad_steps_per_vector_step=grad_steps, total_grad_steps=total_grad_steps, n_evals=n_evals, budget=env_budget, reference=reference)
    if ref_mode:
        if replay is not None and replay != plan["replay"]:
            raise ValueError(f"env_budget='reference' keeps the reference's replay ring ({plan['replay']} rows); {replay} contradicts it")
        replay = plan["replay"]
    if plan["total_grad_steps"] * batch < 0.1 * plan["reference_samples"]:
        raise ValueError(f"planned learner budget ({plan['total_grad_steps']} grad steps x {batch}) is more than 10x below the "
                         f"reference's ({plan['reference_grad_steps']} x 32): raise --total-grad-steps")
    return n_envs, batch, replay, plan


def trial_shape(plan, n_envs, world, batch, replay):
    """The plan and the sizes it was made for, as trial_config.json records them under "batched": what a checkpoint keeps and `--resume` compares."""
    return dict(plan, n_envs=n_envs, world=world, batch=batch, replay=replay)


class TrialRun:
    """One trial of `run_trial` in the parts a lockstep driver needs (`run_trials_together`): the constructor does everything in front of the loop -- plan,
    directory and its JSON files, envs, agent, episode log -- and leaves `learn_args`, the arguments of `IQNAgent.learn_vec` (or of its loop in parts,
    `iqn.agent.VecLoop`); `conclude()` does everything behind it."""

    def __init__(self, device, params, n_envs, rank=0, world=1, shared=False, batch=None, replay=None, verbose=True,
                 grad_steps=None, torch_train=False, total_grad_steps=None, n_evals=None, cvar=1.0, precision="f64",
                 exchange="collective", shared_taus=False, target_sync_mult=1.0, final_eps=0.05, eval_adaptive=True, n_step=1, n_step_mode="reference",
                 eval_one_launch=False, eval_deferred=False, env_budget="learner", reference=None, episode_log=None, eval_config=None, max_eval_steps=1000,
                 on_step=None, train_env=None, eval_worlds=None, per=None, munchausen=None, target_rule="max"):
        import torch
        from .iqn.agent import IQNAgent
        from .marinenav_env.vec_env import VecMarineNavEnv

        if per and shared:
            raise ValueError(PER_REFUSALS["shared"])
        if munchausen and (shared or per):
            raise ValueError(MUNCHAUSEN_REFUSALS["shared" if shared else "per"])
        if target_rule != "max" and (shared or per or munchausen):
            raise ValueError(TARGET_RULE_REFUSALS["shared" if shared else ("per" if per else "munchausen")])
        exp_dir = trial_dir(params, rank, world, shared)
        writer = rank == 0 or not shared
        ref_mode = env_budget == "reference"
        n_envs, batch, replay, plan = plan_trial(params, n_envs, world=world, shared=shared, batch=batch, replay=replay, grad_steps=grad_steps,
                                                 total_grad_steps=total_grad_steps, n_evals=n_evals, env_budget=env_budget, reference=reference)
        total = n_envs * world
        self.shape = trial_shape(plan, n_envs, world, batch, replay)
        if writer:
            os.makedirs(exp_dir, exist_ok=True)
            with open(os.path.join(exp_dir, "trial_config.json"), "w+") as f:
                json.dump(dict(params, batched=self.shape), f)
            with open(os.path.join(exp_dir, "training_schedule.json"), "w+") as f:
                json.dump(TRAINING_SCHEDULE, f)
            if verbose:
                print(f"[train_iqn] {plan['vector_steps']} vector steps x {total} envs = {plan['env_steps']:.3g} env steps; "
                      f"{plan['total_grad_steps']} grad steps of batch {batch} ({plan['grad_steps_per_vector_step']} per vector step; "
                      f"reference: {plan['reference_grad_steps']} of 32); replay ratio {plan['replay_ratio']:.3g} sampled / generated "
                      f"transition (reference {plan['reference_replay_ratio']:.0f}); target copy every {plan['target_sync_grad_steps']} "
                      f"grad steps; evaluation every {plan['eval_every_vector_steps']} vector steps")

        if train_env is None:      # (given: this seed's rows of a stacked env, run_trials_together(stack_envs=True))
            train_env = VecMarineNavEnv(n_envs, seed=params["seed"], first_index=rank * n_envs, schedule=TRAINING_SCHEDULE,
                                        timestep_scale=plan["timestep_scale"], device=device, precision=precision)
        elif train_env.n_envs != n_envs:
            raise ValueError(f"the train env given holds {train_env.n_envs} rows; the plan is for {n_envs}")
        if eval_config is None:
            eval_config = create_eval_configs(device)
        if eval_worlds is not None:      # (a run at toy size: the first few of the evaluation worlds)
            eval_config = {k: eval_config[k] for k in list(eval_config)[:int(eval_worlds)]}
        if writer:
            with open(os.path.join(exp_dir, "eval_config.json"), "w+") as f:
                json.dump(eval_config, f)
        eval_env = VecMarineNavEnv(len(eval_config), device=device, precision=precision) if writer else None

        agent = IQNAgent(26, 9, n_step=n_step, n_step_mode=n_step_mode, BATCH_SIZE=batch, BUFFER_SIZE=replay, device=device,
                         seed=params["seed"] + 100 + (0 if shared else rank), distributed=shared and world > 1,
                         UPDATE_EVERY=1, learning_starts=plan["learning_starts"] if ref_mode else 0, rank=rank if shared else 0, final_eps=final_eps,
                         **(dict(exploration_fraction=plan["exploration_fraction"]) if ref_mode else {}),
                         **(dict(per=True, per_alpha=per["alpha"], per_beta0=per["beta0"]) if per else {}),
                         **(dict(munchausen=True, m_alpha=munchausen["alpha"], m_tau=munchausen["tau"], m_clip=munchausen["clip"]) if munchausen else {}),
                         **(dict(target_rule=target_rule) if target_rule != "max" else {}))
        if per:      # beta reaches 1 with the run's last gradient step (the reference plan's total already leaves out the vector steps in front of learning_starts)
            agent.per_beta_steps = int(plan["total_grad_steps"])
        agent.grad_steps_per_update = plan["grad_steps_per_vector_step"]
        agent.target_sync_grad_steps = max(1, int(round(plan["target_sync_grad_steps"] * target_sync_mult)))
        agent.exchange = exchange
        agent.shared_taus = bool(shared_taus)
        if torch_train:
            agent.use_fused_train = False          # PyTorch autograd + Adam instead of csrc/iqn_train.hip
        log = make_episode_log(episode_log, env_budget, n_envs, plan["eval_every_vector_steps"], train_env.discount, device)
        if ref_mode and not eval_deferred:
            eval_deferred = True      # (300 evaluation points: each only keeps the policy of the moment)
        if max_eval_steps != 1000 and eval_deferred:
            eval_deferred = dict(dict(max_steps=max_eval_steps), **(eval_deferred if isinstance(eval_deferred, dict) else {}))
        self.learn_args = dict(total_vector_steps=plan["vector_steps"], train_env=train_env, eval_env=eval_env, eval_config=eval_config,
                               eval_freq=plan["eval_every_vector_steps"], eval_log_path=exp_dir if writer else None,
                               total_timesteps=plan["vector_steps"] * total, world_size=world, cvar=cvar, verbose=False,
                               report_timestep_scale=params["total_timesteps"] / (plan["vector_steps"] * total), eval_adaptive=eval_adaptive,
                               eval_one_launch=eval_one_launch, eval_deferred=eval_deferred, on_step=on_step, episode_log=log, max_eval_steps=max_eval_steps,
                               eval_points=plan_eval_points(plan, total) if ref_mode else None)
        self.exp_dir, self.writer, self.plan, self.agent, self.train_env, self.eval_env, self.log = exp_dir, writer, plan, agent, train_env, eval_env, log
        self.params = params

    def conclude(self):
        import torch
        exp_dir, writer, agent, train_env, eval_env, log = self.exp_dir, self.writer, self.agent, self.train_env, self.eval_env, self.log
        if writer:
            agent.qnetwork_local.save(exp_dir)
            if log is not None:
                log.save(exp_dir)
        self.release()
        if writer:      # last: the marker says every file of the trial is there (`--resume` skips the seed)
            with open(os.path.join(exp_dir, COMPLETED_FILE), "w") as f:
                json.dump(dict(vector_steps=self.plan["vector_steps"], grad_steps=int(agent.grad_steps)), f)
        return exp_dir

    def release(self):
        """Close the envs and wait for the device; writes nothing (`conclude` without its files: a run that stopped at a checkpoint)."""
        import torch
        self.train_env.close()
        if self.eval_env is not None:
            self.eval_env.close()
        torch.cuda.synchronize()

    # ---- checkpoints (--checkpoint-every, --stop-after, --resume) -------------------------------------------------------------------
    def checkpoint_state(self, loop, next_step, run_args=None):
        """The whole trial behind vector step `next_step - 1` as one dict of CPU tensors and plain values.  Order matters: the env first (its save launches an
        owed reset and joins one under the act kernel, so the observation rows the loop saves are final), then the loop (which flushes the deferred
        evaluations -- that logs into the agent), then the ring and the agent."""
        env = self.train_env.state_dict()      # (the evaluation env is not state: every evaluation loads its worlds afresh and draws nothing from its streams)
        lp = loop.state_dict(next_step)
        return dict(format=CHECKPOINT_FORMAT, vector_step=int(next_step), params=dict(self.params), plan=dict(self.shape), args=dict(run_args or {}),
                    env=env, loop=lp, ring=self.agent.memory.state_dict(), agent=self.agent.state_dict())

    def restore(self, loop, state):
        """`checkpoint_state` back into this (freshly built) trial and its fresh `loop`.  Returns the vector step to continue with.  The agent comes last: its
        state holds torch's generator states, which nothing behind it may move."""
        self.train_env.load_state_dict(state["env"])
        self.agent.memory.load_state_dict(state["ring"])
        next_step = loop.load_state_dict(state["loop"])
        self.agent.load_state_dict(state["agent"])
        assert next_step == int(state["vector_step"])
        return next_step


CHECKPOINT_FORMAT = 1
CHECKPOINT_FILE, CHECKPOINT_PREV_FILE, COMPLETED_FILE = "checkpoint.pt", "checkpoint.prev.pt", "completed.json"
CHECKPOINT_REFUSALS = dict(
    together="--checkpoint-every, --stop-after and --resume save and restore one trial's loop; the lockstep loop of --together (with or without --stack-envs) has no "
             "checkpoint yet: run the seeds one after the other, or with -P",
    shared="--checkpoint-every, --stop-after and --resume save and restore one process's learner; a shared learner (--shared-learner) would need every rank's "
           "state from the same vector step, which has no checkpoint yet",
    world="--checkpoint-every, --stop-after and --resume are the single-process form; they are not combinable with torch.distributed.run (WORLD_SIZE > 1)")
PER_REFUSALS = dict(
    together="--per keeps one learner's priorities next to its own ring and samples, steps and updates them in launches of its own; the grouped gradient launches of "
             "--together draw uniformly inside the launch and have no prioritized form",
    shared="--per weights one learner's batch by its own priorities; a shared learner (--shared-learner) averages the gradients of several ranks' batches, which "
           "has no prioritized form")
MUNCHAUSEN_REFUSALS = dict(
    together="--munchausen runs a second target forward per batch element in a launch of its own; the grouped gradient launches of --together have no "
             "Munchausen form",
    shared="--munchausen steps one learner in launches of its own; a shared learner (--shared-learner), whose gradient exchange rides in the plain step's "
           "launches, has no Munchausen form",
    per="--munchausen takes three tau sets per step and the prioritized sampler of --per emits two; the two options are not combinable yet")
TARGET_RULE_REFUSALS = dict(
    together="--target-rule mean / double step one learner in launches of their own; the grouped gradient launches of --together take the per-sample max and "
             "have no greedy-on-mean form",
    shared="--target-rule mean / double step one learner in launches of their own; a shared learner (--shared-learner), whose gradient exchange rides in the "
           "plain step's launches, has no greedy-on-mean form",
    per="--target-rule mean / double: the weighted step of --per takes the per-sample max only; the two options are not combinable yet",
    munchausen="--target-rule mean / double: the soft-max policy of --munchausen takes the place of the greedy choice; the two options are not combinable")
SHAPE_KEYS_FIRST = ("n_envs", "batch", "replay", "world")      # (named before the plan's own keys, which follow from them)


def write_checkpoint(exp_dir, state):
    """checkpoint.pt in the trial directory `exp_dir`, atomically: written under a temporary name in the same directory and synced, the previous checkpoint
    kept as checkpoint.prev.pt, then renamed into place.  Whatever interrupts this leaves a readable checkpoint.pt or a readable checkpoint.prev.pt."""
    import torch
    path, prev, tmp = (os.path.join(exp_dir, n) for n in (CHECKPOINT_FILE, CHECKPOINT_PREV_FILE, CHECKPOINT_FILE + ".tmp"))
    with open(tmp, "wb") as f:
        torch.save(state, f)
        f.flush()
        os.fsync(f.fileno())
    if os.path.exists(path):
        os.replace(path, prev)
    os.replace(tmp, path)
    return path


def run_shaping_args(env_budget="learner", precision="f64", n_step=1, n_step_mode="reference", shared_taus=False, cvar=1.0, eval_adaptive=True, eval_deferred=False, eval_one_launch=False,
                     episode_log=None, max_eval_steps=1000, reference=None, target_sync_mult=1.0, final_eps=0.05, eval_worlds=None, per=None, munchausen=None, target_rule="max", **_):
    """The arguments of `run_trial` that shape a run beside its plan, normalised: what a checkpoint records and `--resume` compares (`check_resumable`).  ONE
    place builds it, for the run itself and for `--dry-run --resume`; the defaults are `run_trial`'s.  (`torch_train` is recorded by the checkpoint but not
    compared: a checkpoint of one gradient-step path continues on the other.)"""
    return dict(env_budget=env_budget, precision=precision, n_step=int(n_step), n_step_mode=str(n_step_mode), shared_taus=bool(shared_taus), cvar=float(cvar), eval_adaptive=bool(eval_adaptive),
                eval_deferred=bool(eval_deferred), eval_one_launch=bool(eval_one_launch), episode_log=episode_log, max_eval_steps=int(max_eval_steps),
                reference=dict(reference or {}), target_sync_mult=float(target_sync_mult), final_eps=float(final_eps), eval_worlds=eval_worlds,
                **(dict(per=dict(alpha=float(per["alpha"]), beta0=float(per["beta0"]))) if per else {}),      # (a uniform run records no such key, as before there were priorities)
                **(dict(munchausen=dict(alpha=float(munchausen["alpha"]), tau=float(munchausen["tau"]), clip=float(munchausen["clip"]))) if munchausen else {}),      # (nor a run with the plain target this one)
                **(dict(target_rule=str(target_rule)) if target_rule != "max" else {}))      # (nor a run with the per-sample max this one)


def first_difference(saved, now, first=()):
    """(key, saved value, value now) of the first key in which two dicts differ -- `first`, then the others in sorted order -- or None."""
    keys = [k for k in first if k in saved or k in now] + sorted((set(saved) | set(now)) - set(first))
    for k in keys:
        if k not in saved or k not in now or saved[k] != now[k]:
            return k, saved.get(k, "<absent>"), now.get(k, "<absent>")
    return None


def load_checkpoint(seed_dir, log=print):
    """The checkpoint of a trial directory: checkpoint.pt, or -- where that is missing or unreadable while checkpoint.prev.pt is there -- the previous one, with one
    log line saying so.  Returns (state, file name), or (None, None) for a directory without a checkpoint."""
    import torch
    path, prev = os.path.join(seed_dir, CHECKPOINT_FILE), os.path.join(seed_dir, CHECKPOINT_PREV_FILE)
    why = None
    if os.path.exists(path):
        try:
            state = torch.load(path, map_location="cpu", weights_only=False)
            if not isinstance(state, dict) or state.get("format") != CHECKPOINT_FORMAT:
                raise ValueError(f"format {state.get('format') if isinstance(state, dict) else type(state).__name__!r}, this version reads {CHECKPOINT_FORMAT}")
            return state, CHECKPOINT_FILE
        except Exception as e:
            why = f"unreadable ({type(e).__name__}: {e})"
    elif os.path.exists(prev):
        why = "missing"
    if why is None:
        return None, None
    if not os.path.exists(prev):
        raise ValueError(f"{path} is {why} and there is no {CHECKPOINT_PREV_FILE} beside it")
    state = torch.load(prev, map_location="cpu", weights_only=False)
    if not isinstance(state, dict) or state.get("format") != CHECKPOINT_FORMAT:
        raise ValueError(f"{prev}: not a checkpoint of format {CHECKPOINT_FORMAT}")
    log(f"[train_iqn] {path} is {why}: continuing from {CHECKPOINT_PREV_FILE} (vector step {state['vector_step']})")
    return state, CHECKPOINT_PREV_FILE


def check_resumable(state, shape, run_args=None):
    """A checkpoint continues only the run it was taken from: the plan recomputed from the command line must equal the saved one, and so must the arguments
    that shape the run.  ValueError names the first key that differs and both values."""
    d = first_difference(state["plan"], shape, SHAPE_KEYS_FIRST)
    if d is not None:
        raise ValueError(f"--resume: the checkpoint was written by a run with another plan: {d[0]} was {d[1]!r} there and is {d[2]!r} on this command line")
    if run_args is not None and state.get("args"):
        d = first_difference({k: v for k, v in state["args"].items() if k in run_args}, {k: v for k, v in run_args.items() if k in state["args"]})
        if d is None and state["args"].get("per") != run_args.get("per"):      # (recorded only by a run with --per: absent on either side means uniform replay)
            d = ("per", state["args"].get("per"), run_args.get("per"))
        if d is None and state["args"].get("munchausen") != run_args.get("munchausen"):      # (recorded only by a run with --munchausen: absent on either side means the plain target)
            d = ("munchausen", state["args"].get("munchausen"), run_args.get("munchausen"))
        if d is None and state["args"].get("target_rule", "max") != run_args.get("target_rule", "max"):      # (recorded only by a run with --target-rule mean / double)
            d = ("target_rule", state["args"].get("target_rule", "max"), run_args.get("target_rule", "max"))
        if d is not None:
            raise ValueError(f"--resume: the checkpoint was written by a run with other arguments: {d[0]} was {d[1]!r} there and is {d[2]!r} on this command line")


def resume_point(seed_dir, shape, run_args=None, log=print):
    """What `--resume` does with one trial directory: ("completed", None, None), ("start", None, None) or ("checkpoint", state, file name) -- checked."""
    if os.path.exists(os.path.join(seed_dir, COMPLETED_FILE)):
        return "completed", None, None
    state, name = load_checkpoint(seed_dir, log)
    if state is None:
        return "start", None, None
    check_resumable(state, shape, run_args)
    return "checkpoint", state, name


def run_loop_with_checkpoints(run, state=None, checkpoint_every=None, stop_after=None, run_args=None):
    """`IQNAgent.learn_vec` for the trial `run`, in its parts (`iqn.agent.VecLoop`), continued from `state` and with a checkpoint behind every
    `checkpoint_every`-th vector step and behind vector step `stop_after`, where the loop then ends.  Returns the number of vector steps done if it
    stopped there, None if it ran to its end."""
    from .iqn.agent import VecLoop
    agent, total = run.agent, run.learn_args["total_vector_steps"]
    loop = VecLoop(agent, **run.learn_args)
    stopped = None
    try:
        first = run.restore(loop, state) if state is not None else 0
        for it in range(first, total):
            due = loop.collect(it)
            loss = agent.train_steps_from_memory(agent.grad_steps_per_update) if due.train else None
            loop.finish(it, loss)
            done = it + 1
            stop = stop_after is not None and done == stop_after and done < total
            if stop or (checkpoint_every and done % checkpoint_every == 0):
                write_checkpoint(run.exp_dir, run.checkpoint_state(loop, done, run_args))
            if stop:
                stopped = done
                break
        if stopped is None:
            loop.end()
    finally:
        loop.close()
    return stopped


def run_trial(device, params, n_envs, rank=0, world=1, shared=False, batch=None, replay=None, verbose=True,
              grad_steps=None, torch_train=False, total_grad_steps=None, n_evals=None, cvar=1.0, precision="f64",
              exchange="collective", shared_taus=False, target_sync_mult=1.0, final_eps=0.05, eval_adaptive=True, n_step=1, n_step_mode="reference",
              eval_one_launch=False, eval_deferred=False, env_budget="learner", reference=None, episode_log=None, eval_config=None, max_eval_steps=1000,
              on_step=None, return_agent=False, eval_worlds=None, checkpoint_every=None, stop_after=None, resume=False, dump_final_state=None, per=None, munchausen=None, target_rule="max"):
    """train_IQN_model.py:74-121 on the vector env.  `params` is one trial of the reference's config grid
    (seed, total_timesteps, eval_freq, save_dir); see `plan_cadence` for how its env-step cadences map to vector steps.
    `precision`: the env kernels' arithmetic.  "f64" (default: every float32 output within 1e-5 of the reference, no
    outliers; measured free while an IQN acts in the loop) or "mixed" (float32 field / sonar decisions).
    `exchange` (shared learner): "collective" = RCCL all-reduce of the flat gradient, "mailbox" = the exchange inside the gradient step's launch (iqn/mailbox.py).
    `shared_taus`: acting draws its 32 quantile fractions once per act launch instead of once per env (opt-in: a different random variable from the
    reference's per-call draw, model.py:149; A/B on learning in profiles/; the learner's taus are untouched).
    `target_sync_mult`, `final_eps`: study knobs (scripts/learning_curve.py) -- the target network is copied every target_sync_mult x the planned number of gradient
    steps; the exploration floor (agent.py: 0.05); `n_step`: the agent's n-step returns (agent.py:12-29; the reference's scripts use 1; > 1 takes the step + append launch pair
    instead of the fused mn_step_append: mn_step, then the window append mn_replay_append_nstep); `n_step_mode`: "reference" (the reference's window, which slides across
    episode ends) or "episode" (the window cut at its first episode end: iqn/replay_buffer.py).  `eval_adaptive` = False skips the adaptive-CVaR evaluation at the evaluation points (the reference runs both).
    `eval_one_launch`: each evaluation as one mn_rollout_iqn launch instead of one Python iteration per env step (same results).
    `eval_deferred`: an evaluation point keeps the policy of the moment and the episodes of all pending points run as one mn_rollout_iqn_groups launch
    (iqn/deferred_eval.py) -- with `n_evals=300` the reference's evaluation density.
    `env_budget`: "learner" (the above) or "reference" -- the reference's own env-step budget, replay ratio 8, batch 32, its cadences and its evaluation
    timesteps (`plan_reference`; `n_envs` = env steps per vector step, None = 80; `reference` = overrides of its constants for runs at toy size); implies
    deferred evaluations at every eval_freq.  `episode_log`: None (on with "reference", off otherwise), True or "full" -- training_log.npz with one
    summary row of the training episodes per evaluation interval, "full": training_episodes.npz with every episode's record (episode_log.py).
    `eval_config`: the evaluation worlds (default: the 30 of create_eval_configs); `max_eval_steps`: the step limit of an evaluation episode;
    `on_step`: learn_vec's hook; `return_agent`: return (directory, agent); `eval_worlds`: evaluate on the first so many evaluation worlds only.
    `checkpoint_every` = K: behind every K-th vector step the whole trial -- env handle, ring, agent, loop, evaluations, episode log -- goes into
    checkpoint.pt of the trial's directory (`TrialRun.write_checkpoint`); `stop_after` = K: a checkpoint behind vector step K, where the trial then ends without
    its final files; `resume`: skip the trial if its directory holds the completion marker, continue from its checkpoint if it holds one (refused if that was
    written under another plan or other run-shaping arguments), start from the beginning otherwise.  A run stopped and resumed writes, byte for byte, the files
    of the uninterrupted run.  Single process, single learner.  Without the three the loop is `IQNAgent.learn_vec` as ever.
    `per`: None (uniform replay) or dict(alpha=, beta0=) -- proportional prioritized replay (iqn/priority.py): rows drawn in proportion to (mean |TD error| + 1e-6) ** alpha,
    the loss weighted by importance weights whose exponent runs linearly from beta0 to 1 over the run's gradient steps; single learner only.
    `munchausen`: None (the plain target) or dict(alpha=, tau=, clip=) -- the Munchausen target (include/marinenav_hip.h): soft-max policy at temperature tau over the target
    network's mean quantiles, alpha x the log-policy of the action taken, clipped to [clip, 0], added to the reward; single learner, not with `per`.
    `target_rule`: "max" (the reference's max over actions per quantile sample), "mean" (one greedy action per next state, from the target network's mean quantiles) or
    "double" (that action chosen by the local network, valued by the target network) -- include/marinenav_hip.h, "Target rules"; single learner, not with `per` or `munchausen`.
    `dump_final_state`: a file for torch.save(dict(agent=, ring=, env=)) of the `state_dict()`s behind the last vector step (tests)."""
    checkpointing = checkpoint_every is not None or stop_after is not None or resume
    if checkpointing and (shared or world > 1):
        raise ValueError(CHECKPOINT_REFUSALS["shared" if shared else "world"])
    if checkpoint_every is not None and int(checkpoint_every) < 1 or stop_after is not None and int(stop_after) < 1:
        raise ValueError("checkpoint_every and stop_after count vector steps: at least 1")
    run_args = run_shaping_args(env_budget=env_budget, precision=precision, n_step=n_step, n_step_mode=n_step_mode, shared_taus=shared_taus, cvar=cvar, eval_adaptive=eval_adaptive,
                                eval_deferred=eval_deferred, eval_one_launch=eval_one_launch, episode_log=episode_log, max_eval_steps=max_eval_steps, reference=reference,
                                target_sync_mult=target_sync_mult, final_eps=final_eps, eval_worlds=eval_worlds, per=per, munchausen=munchausen, target_rule=target_rule)
    state = None
    if resume:      # (looked at before anything is built or written: a finished seed is left alone, a foreign checkpoint refused)
        exp_dir = trial_dir(params, rank, world, shared)
        ne, b, r, plan = plan_trial(params, n_envs, world=world, shared=shared, batch=batch, replay=replay, grad_steps=grad_steps, total_grad_steps=total_grad_steps,
                                    n_evals=n_evals, env_budget=env_budget, reference=reference)
        what, state, name = resume_point(exp_dir, trial_shape(plan, ne, world, b, r), run_args)
        if what == "completed":
            print(f"[train_iqn] seed {params['seed']}: {exp_dir} holds {COMPLETED_FILE}, nothing to do", flush=True)
            return (exp_dir, None) if return_agent else exp_dir
        if verbose:
            print(f"[train_iqn] seed {params['seed']}: " + (f"continuing from vector step {state['vector_step']} ({name})" if state is not None
                                                            else "no checkpoint, starting from the beginning"), flush=True)
    run = TrialRun(device, params, n_envs, rank=rank, world=world, shared=shared, batch=batch, replay=replay, verbose=verbose, grad_steps=grad_steps,
                   torch_train=torch_train, total_grad_steps=total_grad_steps, n_evals=n_evals, cvar=cvar, precision=precision, exchange=exchange,
                   shared_taus=shared_taus, target_sync_mult=target_sync_mult, final_eps=final_eps, eval_adaptive=eval_adaptive, n_step=n_step, n_step_mode=n_step_mode,
                   eval_one_launch=eval_one_launch, eval_deferred=eval_deferred, env_budget=env_budget, reference=reference, episode_log=episode_log,
                   eval_config=eval_config, max_eval_steps=max_eval_steps, on_step=on_step, eval_worlds=eval_worlds, per=per, munchausen=munchausen, target_rule=target_rule)
    if checkpoint_every is None and stop_after is None and state is None:
        run.agent.learn_vec(**run.learn_args)
    else:
        stopped = run_loop_with_checkpoints(run, state, checkpoint_every, stop_after, dict(run_args, torch_train=bool(torch_train)))
        if stopped is not None:
            run.release()
            print(f"[train_iqn] seed {params['seed']}: stopped after vector step {stopped} of {run.plan['vector_steps']}; checkpoint in "
                  f"{os.path.join(run.exp_dir, CHECKPOINT_FILE)} (continue with --resume {os.path.dirname(run.exp_dir)})", flush=True)
            return (run.exp_dir, run.agent) if return_agent else run.exp_dir
    if dump_final_state is not None:
        import torch
        torch.save(dict(env=run.train_env.state_dict(), ring=run.agent.memory.state_dict(), agent=run.agent.state_dict()), dump_final_state)
    exp_dir = run.conclude()
    return (exp_dir, run.agent) if return_agent else exp_dir


def group_trials(trials, limit=None):
    """The trials of a config grid that can train together: lists of indices into `trials`, in order, each of trials that differ only in their seed (hence
    share a plan), at most `limit` (default MN_IQN_MAX_LEARNERS = 64) to a list."""
    if limit is None:
        from ._capi import IQN_MAX_LEARNERS as limit
    by_key = {}
    for i, p in enumerate(trials):
        key = json.dumps({k: v for k, v in p.items() if k != "seed"}, sort_keys=True, default=str)
        by_key.setdefault(key, []).append(i)
    return [idx[k:k + limit] for idx in by_key.values() for k in range(0, len(idx), limit)]


TOGETHER_REFUSALS = dict(
    torch_train="--together needs the fused HIP gradient step: there is no grouped form of the PyTorch step (--torch-train)",
    shared="--together trains independent learners, one per seed; a shared learner (--shared-learner) exchanges its gradient with other ranks, which has no grouped form",
    procs="--together runs the seeds in ONE process so that their gradient steps can share launches; -P > 1 would put them into separate processes",
    world="--together is the single-process, single-GPU form; it is not combinable with torch.distributed.run (WORLD_SIZE > 1)",
    stack_envs="--stack-envs stacks the envs of seeds that train together in one handle; it needs --together",
    stack_n_step="--stack-envs appends 1-step transitions in one grouped launch; n_step > 1 keeps its window per seed and has no stacked form",
    stack_shared_taus="--stack-envs acts with per-row taus in one grouped launch; launch-shared taus (--shared-taus) have no stacked form")


def stacked_train_env(device, trials, n_envs, env_budget="learner", batch=None, replay=None, grad_steps=None, total_grad_steps=None, n_evals=None, reference=None,
                      precision="f64"):
    """The ONE train env of trials that train together with stacked envs, and the rows per seed: `VecMarineNavEnv(G n, ...)` whose rows [g n, (g + 1) n)
    are seeded, scheduled and scaled as trial g's own env of n rows is (`TrialRun`), so every row steps and resets as it does there."""
    from .marinenav_env.vec_env import VecMarineNavEnv, stacked_seeds
    n, batch, replay = resolve_budget_args(env_budget, n_envs, batch, replay)
    p = trials[0]
    plan = plan_cadence(p["total_timesteps"], p["eval_freq"], n, batch, grad_steps_per_vector_step=grad_steps, total_grad_steps=total_grad_steps, n_evals=n_evals,
                        budget=env_budget, reference=reference)
    env = VecMarineNavEnv(len(trials) * n, seeds=stacked_seeds(n, [t["seed"] for t in trials]), schedule=TRAINING_SCHEDULE, timestep_scale=plan["timestep_scale"],
                          device=device, precision=precision)
    return env, n


def run_trials_together(device, trials, n_envs, on_step=None, return_agents=False, torch_train=False, shared=False, world=1, stack_envs=False, sync_every_step=None,
                        **kwargs):
    """`run_trial` for several trials that differ only in their seed (one list of `group_trials`), in LOCKSTEP: per vector step every trial collects as it
    does alone -- its own envs, agent, exploration, generators, replay ring, episode log, UnderActGuard and hook -- then, if the cadence says train (the same
    for all: equal plans, equally full rings), the gradient steps behind that vector step run for ALL trials through one `LearnerGroup`
    (iqn/group_train.py: three launches per gradient step instead of one to three per trial); then every trial finishes the step -- target copy on its own
    cadence, resets, counters, evaluation points, log.  The order of launches per agent is `vec_step`'s, and every learner is bit for bit what it is alone,
    so each seed's directory holds what `run_trial` writes, with the same contents.  The device is synchronised once per vector step (see the loop).  `on_step`: None or one hook per trial; the other arguments as
    `run_trial`'s.  Returns the trial directories (`return_agents`: and the agents).
    `stack_envs`: the collect phase is shared too -- the seeds' envs are the rows of ONE handle (`stacked_train_env`) and per vector step there is one
    act launch at the common exploration rate, one env step, one append into all rings, one reset launch in front (iqn/group_collect.py: `CollectorGroup`)
    instead of one of each per seed; every seed then finishes the step on its own rows (`VecLoop.collect_given`).  Every seed's files stay what `run_trial`
    writes.  Needs n_step = 1 and per-row taus.  `sync_every_step`: the device synchronisation per vector step (None: on with per-seed envs, off with stacked ones -- see the loop; results do not depend on it)."""
    import torch
    from .iqn.agent import VecLoop
    from .iqn.group_train import LearnerGroup
    if torch_train:
        raise ValueError(TOGETHER_REFUSALS["torch_train"])
    if shared or world > 1:
        raise ValueError(TOGETHER_REFUSALS["shared" if shared else "world"])
    trials = list(trials)
    if len(group_trials(trials)) != 1:
        raise ValueError("trials that train together differ only in their seed, and are at most 64 (group_trials)")
    if stack_envs:
        if kwargs.get("n_step", 1) != 1:
            raise ValueError(TOGETHER_REFUSALS["stack_n_step"])
        if kwargs.get("shared_taus", False):
            raise ValueError(TOGETHER_REFUSALS["stack_shared_taus"])
    if kwargs.get("per"):
        raise ValueError(PER_REFUSALS["together"])
    if kwargs.get("munchausen"):
        raise ValueError(MUNCHAUSEN_REFUSALS["together"])
    if kwargs.get("target_rule", "max") != "max":
        raise ValueError(TARGET_RULE_REFUSALS["together"])
    hooks = list(on_step) if on_step is not None else [None] * len(trials)
    stacked, views = None, [None] * len(trials)
    if stack_envs:
        from .iqn.group_collect import CollectorGroup
        from .marinenav_env.vec_env import StackedRows
        env_kw = {k: kwargs[k] for k in ("env_budget", "batch", "replay", "grad_steps", "total_grad_steps", "n_evals", "reference", "precision") if k in kwargs}
        stacked, n_rows = stacked_train_env(device, trials, n_envs, **env_kw)
        views = [StackedRows(stacked, g, n_rows) for g in range(len(trials))]
    runs = [TrialRun(device, p, n_envs, on_step=h, train_env=v, **kwargs) for p, h, v in zip(trials, hooks, views)]
    plan = runs[0].plan
    assert all(r.plan == plan for r in runs)
    loops, group, collectors = [], None, None
    try:
        for r in runs:
            loops.append(VecLoop(r.agent, **r.learn_args))
        group = LearnerGroup([r.agent for r in runs])
        if stack_envs:      # (behind the LearnerGroup: the fused trainer it makes re-allocates the networks' parameters into its flat buffers)
            collectors = CollectorGroup([r.agent for r in runs], stacked)
            obs, cvar = stacked.obs, runs[0].learn_args["cvar"]
        G = runs[0].agent.grad_steps_per_update
        for it in range(plan["vector_steps"]):
            if stack_envs:
                eps = loops[0].eps_now()
                assert all(lp.eps_now() == eps for lp in loops), "the seeds of a group explore at one rate"
                actions = collectors.act(obs, eps, cvar)
                next_obs, reward, done, info = stacked.step(actions)
                collectors.append(obs, actions, reward, next_obs, done)
                obs = stacked.reset_done()
                dues = [lp.collect_given(it, obs[v.rows], reward[v.rows], done[v.rows], info[v.rows]) for lp, v in zip(loops, views)]
            else:
                dues = [lp.collect(it) for lp in loops]
            assert all(d.train == dues[0].train for d in dues), "the seeds of a group train on one cadence"
            losses = group.train_many(G) if dues[0].train else None
            for k, lp in enumerate(loops):
                lp.finish(it, None if losses is None else losses[k])
            # The host must not run ahead of the device here.  With the launches of several seeds -- each env with a reset stream of its own -- queued many vector
            # steps deep, the lockstep loop measured 4.1 ms per vector step for five seeds; with the queue drained once per vector step 1.25 ms (one seed alone:
            # 0.68 ms).  One synchronisation per vector step of ALL seeds; it changes no result.  The stacked loop has ONE env handle and issues its collect on
            # one stream: there the synchronisation only costs (five seeds: 1 005 -> 965 us per vector step at n = 80, 317 -> 281 us at n = 4 096, ranges
            # apart; profiles/iqn_group_collect_bench.txt), so it runs without.
            if sync_every_step if sync_every_step is not None else not stack_envs:
                torch.cuda.synchronize(device)
        for lp in loops:
            lp.end()
    finally:
        for lp in loops:
            lp.close()
        if group is not None:
            group.close()
        if collectors is not None:
            collectors.close()
    dirs = [r.conclude() for r in runs]
    if stacked is not None:
        stacked.close()
    return (dirs, [r.agent for r in runs]) if return_agents else dirs


def _worker_device(requested, i, n_gpu):
    """Device of pool worker i: `-D cuda:K` pins every worker to GPU K; `-D cuda` or no -D spreads them, worker i on GPU i modulo the
    visible GPUs; anything else (`-D cpu`) is passed through."""
    if requested is None or requested == "cuda":
        return f"cuda:{i % max(1, n_gpu)}"
    return requested


def _trial_worker(device, params, n_envs, kw, sharers=1):
    """One trial in a pool worker.  `sharers`: how many workers run on this worker's GPU at a time.  The one-launch gradient step needs every one of its
    workgroups resident at once and plans for the whole device; two such launches of two processes on one GPU would starve each other (bounded waits run
    out, the step is skipped): with company, the worker plans for its share of the CUs (mn_iqn_train_set_cu_limit -> the two- / three-launch forms, same
    results); whether the episode resets still find room beside the act kernel is checked by the loop's own first steps (iqn/agent.py: UnderActGuard)."""
    import torch
    dev = torch.device(device)
    if dev.type == "cuda" and dev.index is not None:      # (an un-indexed or non-CUDA device has no current-device to set)
        torch.cuda.set_device(dev)
    if sharers > 1 and dev.type == "cuda":
        from . import _capi
        cus = torch.cuda.get_device_properties(dev).multi_processor_count
        _capi.lib().mn_iqn_train_set_cu_limit(max(8, cus // sharers - 8))
    return run_trial(device, params, n_envs, verbose=False, **kw)


def main(argv=None):
    ap = argparse.ArgumentParser(description="Train IQN model (batched MI355X path)")
    ap.add_argument("-C", "--config-file", dest="config_file", type=open, required=True)
    ap.add_argument("-D", "--device", dest="device", type=str, default=None)
    ap.add_argument("-P", "--num-procs", dest="num_procs", type=int, default=1,
                    help="train_IQN_model.py:24-30: run the trials of the config grid (seeds) in this many worker processes at a time; "
                         "worker i uses GPU i modulo the visible GPUs (several seeds on one MI355X share it).  Not combinable with torch.distributed.run")
    ap.add_argument("--n-envs", type=int, default=None, help="environments per GPU (default 4096: see the module docstring; 65536 = the bench's configuration; "
                                                             "with --env-budget reference: env steps per vector step, default 80)")
    ap.add_argument("--batch", type=int, default=None, help="default 256 (--env-budget reference: 32, the reference's)")
    ap.add_argument("--replay", type=int, default=None, help="replay ring rows, default 100 000 (--env-budget reference: 1 000 000, the reference's)")
    ap.add_argument("--env-budget", default="learner", choices=["learner", "reference"],
                    help="learner (default): the reference's learner budget in big batches over many more env steps -- the fast mode; reference: the reference's own "
                         "experiment -- total_timesteps env steps, one batch-32 gradient step per 4 of them, its target / evaluation cadence and evaluation timesteps "
                         "(deferred evaluations, episode log on) -- the drop-in mode; an explicit value that contradicts it is an error")
    ap.add_argument("--episode-log", nargs="?", const=True, default=None, choices=["full"],
                    help="training_log.npz: one summary row of the training episodes per evaluation interval, from a device-side log (one small launch per vector "
                         "step, no host synchronisation); `--episode-log full`: training_episodes.npz with every episode's record too.  Default: off (on with "
                         "--env-budget reference)")
    ap.add_argument("--dry-run", action="store_true", help="print the plan of every trial as JSON and exit (no GPU needed)")
    ap.add_argument("--shared-learner", action="store_true")
    ap.add_argument("--grad-steps", type=int, default=None,
                    help="gradient steps per vector step (default: 16 per 65 536 envs, i.e. learner ~ half of the GPU time)")
    ap.add_argument("--total-grad-steps", type=int, default=None,
                    help="learner budget (default: the reference's sample count, total_timesteps / 4 * 32 / batch)")
    ap.add_argument("--n-evals", type=int, default=None, help="evaluation points over the run (default: min(30, total_timesteps / eval_freq))")
    ap.add_argument("--cvar", type=float, default=1.0, help="CVaR level of the acting policy while training (configs[4]: 0.5)")
    ap.add_argument("--torch-train", action="store_true", help="gradient step through PyTorch instead of the fused HIP kernels")
    ap.add_argument("--precision", default="f64", choices=["f64", "mixed"],
                    help="env kernels: f64 (default; strict 1e-5 parity, free next to the IQN act kernel) or mixed")
    ap.add_argument("--exchange", default="collective", choices=["collective", "mailbox"],
                    help="with --shared-learner: how the ranks' gradients meet -- one RCCL all-reduce per gradient step, or the exchange inside the step's own launch")
    ap.add_argument("--shared-taus", action="store_true", help="acting: one set of 32 taus per act launch instead of per env (opt-in, ~11 %% shorter runs)")
    ap.add_argument("--eval-one-launch", action="store_true",
                    help="evaluations: every episode in one mn_rollout_iqn launch instead of one Python iteration per step (same results)")
    ap.add_argument("--eval-deferred", action="store_true",
                    help="evaluations: a point only keeps the policy of the moment; all pending points run later as ONE mn_rollout_iqn_groups launch on tau streams of "
                         "their own (iqn/deferred_eval.py).  With --n-evals 300: the reference's evaluation density")
    ap.add_argument("--together", action="store_true",
                    help="train the trials that differ only in their seed in lockstep in one process, up to 64 at a time: their gradient steps share three launches per "
                         "step (forward / backward, reduction, clip + Adam with the seed as a grid dimension: mn_iqn_group_train_step); every seed's files equal the "
                         "sequential run's.  Not with --torch-train, --shared-learner, -P > 1 or torch.distributed.run; a trial without companions runs as without "
                         "the option")
    ap.add_argument("--stack-envs", action="store_true",
                    help="with --together: the seeds' envs are the rows of ONE env handle and a vector step is one act launch, one env step, one replay append and one "
                         "reset launch for all of them (mn_iqn_actor_group_act / _append) instead of one of each per seed; every seed's files stay equal to the "
                         "sequential run's.  Not with --shared-taus")
    ap.add_argument("--checkpoint-every", type=int, default=None, metavar="K",
                    help="behind every K-th vector step write checkpoint.pt into the trial's directory (atomically; the previous one is kept as checkpoint.prev.pt): the "
                         "env handle's snapshot (mn_state_save), the replay ring, the agent, the loop, the evaluations and the episode log.  Off by default: the loop "
                         "then does nothing it did not do before")
    ap.add_argument("--stop-after", type=int, default=None, metavar="K",
                    help="end every trial behind vector step K with a checkpoint written at that step; exit status 0 (a time-limited session: continue with --resume).  With "
                         "several seeds EVERY seed runs to its vector step K, one after the other (or in its -P worker), before the process ends.  A K at or beyond the "
                         "plan's vector steps stops nothing: the trial completes")
    ap.add_argument("--resume", default=None, metavar="TRAINING_DIR",
                    help="continue the run in save_dir/training_<time>: per seed, skip it if it is complete, continue from its checkpoint.pt (checkpoint.prev.pt if that "
                         "is unreadable) or start it if it has none.  Give the command line of the original run: another plan is refused.  The files written equal "
                         "those of the uninterrupted run byte for byte.  With --dry-run: print where every seed would continue")
    ap.add_argument("--run-name", default=None, metavar="NAME", help="name the run directory training_NAME instead of training_<start time>")
    ap.add_argument("--reference", nargs="*", default=None, metavar="KEY=VALUE",
                    help="with --env-budget reference: overrides of the reference's constants (learning_starts, target_update_interval, exploration_fraction, replay) "
                         "for runs at toy size")
    ap.add_argument("--max-eval-steps", type=int, default=1000, help="step limit of an evaluation episode (default 1000, the reference's)")
    ap.add_argument("--eval-worlds", type=int, default=None, metavar="N", help="evaluate on the first N of the 30 evaluation worlds (runs at toy size)")
    ap.add_argument("--n-step", type=int, default=1, help="the agent's n-step returns (default 1, the reference's scripts)")
    ap.add_argument("--n-step-mode", choices=("reference", "episode"), default="reference",
                    help="with --n-step > 1: 'reference' = the reference's sliding window, which does not restart at episode ends (default); 'episode' = the standard "
                         "n-step transition, cut at the window's first episode end (return up to it, its next state, done = 1)")
    ap.add_argument("--per", action="store_true",
                    help="proportional prioritized experience replay (opt-in): rows are drawn in proportion to (mean |TD error| + 1e-6) ** alpha by an exact device-side "
                         "sampler, the loss is weighted by importance weights whose exponent beta runs from --per-beta0 to 1 over the run's gradient steps; "
                         "single learner (not with --together or --shared-learner)")
    ap.add_argument("--per-alpha", type=float, default=0.6, help="with --per: the priority exponent (default 0.6)")
    ap.add_argument("--per-beta0", type=float, default=0.4, help="with --per: the importance exponent at the first gradient step (default 0.4)")
    ap.add_argument("--munchausen", action="store_true",
                    help="the Munchausen target (opt-in; Vieillard et al. 2020): a soft-max policy over the target network's mean quantiles replaces the hard max, its "
                         "entropy enters the target and the scaled, clipped log-policy of the action taken is added to the reward; single learner (not with "
                         "--together, --shared-learner or --per)")
    ap.add_argument("--m-alpha", type=float, default=0.9, help="with --munchausen: the weight of the log-policy bonus (default 0.9)")
    ap.add_argument("--m-tau", type=float, default=0.03, help="with --munchausen: the entropy temperature (default 0.03)")
    ap.add_argument("--m-clip", type=float, default=-1.0, help="with --munchausen: the lower clip bound of the log-policy bonus (default -1)")
    ap.add_argument("--target-rule", choices=("max", "mean", "double"), default="max",
                    help="which action the TD target bootstraps from: max (default; the reference's max over actions per quantile sample), mean (the IQN paper's "
                         "one greedy action per next state, the argmax of the target network's mean quantiles) or double (Double-IQN: the local network chooses, the "
                         "target network values); mean and double: single learner (not with --together, --shared-learner, --per or --munchausen)")
    ap.add_argument("--dump-final-state", default=None, metavar="FILE",
                    help="behind the last vector step, torch.save the state_dict()s of the agent, its replay ring and the train env of the LAST trial run to FILE (tests)")
    args = ap.parse_args(argv)
    checkpointing = args.checkpoint_every is not None or args.stop_after is not None or args.resume is not None
    if checkpointing:
        refused = [k for k, on in (("together", args.together or args.stack_envs), ("shared", args.shared_learner), ("world", int(os.environ.get("WORLD_SIZE", "1")) > 1)) if on]
        if refused:
            raise SystemExit("train_iqn: " + CHECKPOINT_REFUSALS[refused[0]])
        if (args.checkpoint_every is not None and args.checkpoint_every < 1) or (args.stop_after is not None and args.stop_after < 1):
            raise SystemExit("train_iqn: --checkpoint-every and --stop-after count vector steps: at least 1")
    if args.per:
        refused = [k for k, on in (("together", args.together or args.stack_envs), ("shared", args.shared_learner)) if on]
        if refused:
            raise SystemExit("train_iqn: " + PER_REFUSALS[refused[0]])
        if not (args.per_alpha >= 0 and 0 <= args.per_beta0 <= 1):
            raise SystemExit("train_iqn: --per-alpha is at least 0 and --per-beta0 lies in [0, 1]")
    if args.munchausen:
        refused = [k for k, on in (("together", args.together or args.stack_envs), ("shared", args.shared_learner), ("per", args.per)) if on]
        if refused:
            raise SystemExit("train_iqn: " + MUNCHAUSEN_REFUSALS[refused[0]])
        if not (0 < args.m_tau < float("inf") and args.m_clip <= 0 and 0 <= args.m_alpha < float("inf")):
            raise SystemExit("train_iqn: --m-tau is above 0, --m-clip at most 0 and --m-alpha at least 0")
    if args.target_rule != "max":
        refused = [k for k, on in (("together", args.together or args.stack_envs), ("shared", args.shared_learner), ("per", args.per),
                                   ("munchausen", args.munchausen)) if on]
        if refused:
            raise SystemExit("train_iqn: " + TARGET_RULE_REFUSALS[refused[0]])
    reference = None
    if args.reference is not None:
        if args.env_budget != "reference":
            raise SystemExit("train_iqn: --reference overrides belong to --env-budget reference")
        try:
            reference = {k: (float(v) if k == "exploration_fraction" else int(v)) for k, v in (kv.split("=", 1) for kv in args.reference)}
        except ValueError:
            raise SystemExit("train_iqn: --reference takes KEY=VALUE pairs with numeric values")
    if args.dump_final_state is not None and args.together:
        raise SystemExit("train_iqn: --dump-final-state dumps one trial's state; the lockstep loop of --together has none to dump")
    if args.stack_envs and not args.together:
        raise SystemExit("train_iqn: " + TOGETHER_REFUSALS["stack_envs"])
    if args.stack_envs and args.shared_taus:
        raise SystemExit("train_iqn: " + TOGETHER_REFUSALS["stack_shared_taus"])
    if args.together:
        refused = [k for k, on in (("torch_train", args.torch_train), ("shared", args.shared_learner), ("procs", args.num_procs > 1),
                                   ("world", int(os.environ.get("WORLD_SIZE", "1")) > 1)) if on]
        if refused:
            raise SystemExit("train_iqn: " + TOGETHER_REFUSALS[refused[0]])
    params = json.load(args.config_file)
    stamp = args.run_name
    if args.resume is not None:
        rdir = os.path.abspath(args.resume)
        if not os.path.isdir(rdir) or not os.path.basename(rdir).startswith("training_"):
            raise SystemExit(f"train_iqn: --resume takes a run directory, save_dir/training_<time>; {args.resume!r} is none")
        stamp = os.path.basename(rdir)[len("training_"):]
        for p in trial_params(params):
            if os.path.realpath(os.path.join(p["save_dir"], "training_" + stamp)) != os.path.realpath(rdir):
                raise SystemExit(f"train_iqn: --resume {args.resume}: the config's save_dir ({p['save_dir']!r}) does not lead to that directory")
    # run_trial's keyword arguments, built here so that --dry-run --resume checks a checkpoint against exactly what the run itself would be given
    kw = dict(batch=args.batch, replay=args.replay, grad_steps=args.grad_steps, torch_train=args.torch_train,
              total_grad_steps=args.total_grad_steps, n_evals=args.n_evals, cvar=args.cvar, precision=args.precision,
              exchange=args.exchange, shared_taus=args.shared_taus, eval_one_launch=args.eval_one_launch, eval_deferred=args.eval_deferred,
              env_budget=args.env_budget, episode_log=args.episode_log)
    # (only what was asked for is passed on: without these options run_trial is called as ever)
    if reference is not None:
        kw["reference"] = reference
    if args.max_eval_steps != 1000:
        kw["max_eval_steps"] = args.max_eval_steps
    if args.eval_worlds is not None:
        kw["eval_worlds"] = args.eval_worlds
    if args.n_step != 1:
        kw["n_step"] = args.n_step
    if args.n_step_mode != "reference":
        kw["n_step_mode"] = args.n_step_mode
    if args.per:
        kw["per"] = dict(alpha=args.per_alpha, beta0=args.per_beta0)
    if args.munchausen:
        kw["munchausen"] = dict(alpha=args.m_alpha, tau=args.m_tau, clip=args.m_clip)
    if args.target_rule != "max":
        kw["target_rule"] = args.target_rule
    if checkpointing:
        kw.update(checkpoint_every=args.checkpoint_every, stop_after=args.stop_after, resume=args.resume is not None)
    if args.dump_final_state is not None:
        kw["dump_final_state"] = args.dump_final_state
    run_args = run_shaping_args(**kw)
    if args.dry_run:
        n_envs, batch, replay = resolve_budget_args(args.env_budget, args.n_envs, args.batch, args.replay)
        for p in trial_params(params):
            try:
                plan = plan_cadence(p["total_timesteps"], p["eval_freq"], n_envs, batch, grad_steps_per_vector_step=args.grad_steps,
                                    total_grad_steps=args.total_grad_steps, n_evals=args.n_evals, budget=args.env_budget, reference=reference)
                if args.env_budget == "reference" and replay is not None and replay != plan["replay"]:
                    raise ValueError(f"env_budget='reference' keeps the reference's replay ring ({plan['replay']} rows); {replay} contradicts it")
            except ValueError as e:
                raise SystemExit(f"train_iqn: {e}")
            print(json.dumps(dict(seed=p["seed"], n_envs=n_envs, batch=batch, replay=plan.get("replay", replay), env_budget=args.env_budget,
                                  eval_deferred=args.eval_deferred or args.env_budget == "reference",
                                  episode_log=(args.env_budget == "reference") if args.episode_log is None else args.episode_log, plan=plan)))
            if args.resume is not None:      # where this seed would continue (reads its checkpoint on the host; the same checks as the run itself)
                try:
                    shape = trial_shape(plan, n_envs, 1, batch, plan.get("replay", replay))
                    what, state, name = resume_point(trial_dir(dict(p, training_time=stamp)), shape, run_args)
                except ValueError as e:
                    raise SystemExit(f"train_iqn: {e}")
                print(json.dumps(dict(seed=p["seed"], resume=what, vector_step=None if state is None else int(state["vector_step"]), checkpoint=name,
                                      vector_steps=plan["vector_steps"])))
        if args.together:
            trials = trial_params(params)
            stacked = lambda g: dict(stacked_env_rows=len(g) * n_envs, rows_per_seed=n_envs) if args.stack_envs and len(g) > 1 else {}
            print(json.dumps(dict(together=[dict(group=k, seeds=[trials[i]["seed"] for i in g], grouped_gradient_launches=len(g) > 1, **stacked(g))
                                            for k, g in enumerate(group_trials(trials))])))
        return
    import torch
    world = int(os.environ.get("WORLD_SIZE", "1")); rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    # the reference's -D takes "cpu" / "cuda" (train_IQN_model.py:33-40); here: "cuda" = this rank's GPU, "cuda:K" = that GPU, anything else is refused
    # by the package itself (no CPU path: VecMarineNavEnv raises)
    device = f"cuda:{local}" if args.device in (None, "cuda") else args.device
    if torch.device(device).type == "cuda":
        torch.cuda.set_device(torch.device(device))
    if world > 1:
        import torch.distributed as dist
        dist.init_process_group("nccl", device_id=torch.device(device))
    if stamp is None:
        stamp = datetime.now().strftime("%Y-%m-%d-%H-%M-%S")
    trials = trial_params(params)
    for p in trials:
        p["training_time"] = stamp
    if args.num_procs > 1:
        # train_IQN_model.py:173-179: a Pool of workers, one trial each.  `spawn`: every worker gets its own HIP context
        if world > 1:
            raise SystemExit("--num-procs runs independent trials; do not combine it with torch.distributed.run")
        import multiprocessing as mp
        n_gpu = max(1, torch.cuda.device_count())
        with mp.get_context("spawn").Pool(processes=args.num_procs) as pool:
            devs = [_worker_device(args.device, i, n_gpu) for i in range(len(trials))]
            # workers that can be on one GPU at a time: the pool runs `num_procs` trials at once, worker i on devs[i]
            sharers = max(1, max(sum(1 for d in devs[:args.num_procs] if d == x) for x in set(devs[:args.num_procs]))) if trials else 1
            jobs = [pool.apply_async(_trial_worker, (devs[i], p, args.n_envs, kw, sharers)) for i, p in enumerate(trials)]
            pool.close()
            for j in jobs:
                j.get()
            pool.join()
        return
    if args.together:
        import time
        for g in group_trials(trials):
            t0 = time.time()
            if len(g) > 1:
                seeds = [trials[i]["seed"] for i in g]
                print(f"[train_iqn] seeds {seeds} train together: three launches per gradient step for the {len(g)} of them", flush=True)
                dirs = run_trials_together(device, [trials[i] for i in g], args.n_envs, verbose=True, stack_envs=args.stack_envs, **kw)
                print(f"[train_iqn] seeds {seeds}: {time.time() - t0:.1f} s -> {os.path.dirname(dirs[0])}", flush=True)
            else:
                run_trial(device, trials[g[0]], args.n_envs, verbose=True, **kw)
        return
    for p in trials:
        run_trial(device, p, args.n_envs, rank, world, args.shared_learner, verbose=True, **kw)
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
