"""The scenario behind tests/golden/step_bits_parent.npz, shared by its recorder (`python tests/step_bits_scenario.py`, run once on the build BEFORE
the step kernel's loads were reordered) and by tests/test_step_bits_parent_gpu.py, which replays it through every form of the step on the current build
and compares raw bits.

37 envs (not a multiple of any lane group per wavefront), 8 cores / 10 obstacles, seed 5, 12 vector steps with `reset_done` after each; env e takes
action (e + t) % 9 at step t, so every step sees all nine actions; max_episode_steps = 5 with episode clocks staggered by e % 5, so episodes end (and
worlds are regenerated) in every step from the second on.  Two parameter cases per precision:
  "default": the default parameters;
  "S3":      tests/params_sets.py's S3 (sonar_range 6, sonar_angle pi: other beam tables, wedge filter off).  The outermost beams are +-pi/2 off the
             heading, so with theta = 0 (even envs) beam 10 and with theta = pi (odd envs) beam 0 is within 1e-3 of the vertical and is cast exactly
             vertically (robot.py:135-143); every env starts 3 m below its first obstacle's rim so that this beam hits.
The ring is 64 rows (< 2 x 37: the 37 rows of a step wrap around its end every second step)."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "step_bits_parent.npz")
N, SEED, T, RING = 37, 5, 12, 64
CASES = [(prec, case) for prec in ("f64", "mixed") for case in ("default", "S3")]
ENV_KEYS = ("obs", "reward", "done", "info", "state", "ep_t", "tot_t", "obs_next")
RING_KEYS = ("ring_states", "ring_next_states", "ring_actions", "ring_rewards", "ring_dones")


def actions(t):
    return ((np.arange(N) + t) % 9).astype(np.int32)


def make_env(precision, case, step_lanes=0, rollout_lanes=0):
    """The env of one case, reset, posed and with its episode clocks staggered.  Returns (env, first observation tensor)."""
    import torch
    from distributional_rl_navigation_amd.marinenav_env.vec_env import VecMarineNavEnv
    sys.path.insert(0, HERE)
    import params_sets
    env = VecMarineNavEnv(N, seed=SEED, device="cuda:0", precision=precision, step_lanes=step_lanes, rollout_lanes=rollout_lanes)
    spec = dict(num_cores=8, num_obs=10, max_episode_steps=5)
    if case == "S3":
        spec.update(dict(params_sets.STEP_SETS)["S3"])
    params_sets.vec_env_set(env, spec)
    env.reset()
    s, ep, tot = env.get_state()
    if case == "S3":
        w = env.get_worlds()
        for e in range(N):
            ox, oy, r = w[e]["obstacles"][0]
            up = e % 2 == 0       # theta = 0: beam 10 points along world +y; theta = pi: beam 0 does
            s[e, 0], s[e, 1], s[e, 2] = ox, oy - r - 3.0, 0.0 if up else np.pi
            s[e, 3:] = 0.0
    env.set_state(s, (np.arange(N) % 5).astype(np.int32), tot)
    if case == "S3":      # the observation the first transition starts from: any row will do, but it must be the same in every replay
        env.obs.copy_(torch.from_numpy(np.arange(N * 26, dtype=np.float32).reshape(N, 26) / 64).to(env.obs.device))
    return env, env.obs


def raw(x):
    """Raw bits of a tensor / array as an unsigned integer numpy array."""
    a = x.detach().cpu().numpy() if hasattr(x, "detach") else np.asarray(x)
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize]).copy()


def run_loop(precision, case, step_lanes=0, append=False):
    """T x (step | step_append, reset_done).  Returns {key: [T, ...] raw bits}."""
    import torch
    from distributional_rl_navigation_amd.iqn.replay_buffer import ReplayBuffer
    env, obs = make_env(precision, case, step_lanes=step_lanes)
    buf = ReplayBuffer(RING, 32, "cuda:0", seed=0, gamma=0.99) if append else None
    out = {k: [] for k in ENV_KEYS + (RING_KEYS if append else ())}
    for t in range(T):
        a = torch.from_numpy(actions(t)).to("cuda:0")
        if append:
            ptr = buf.ptr
            o, r, d, i = env.step_append(a, obs, buf)
            rows = torch.from_numpy((ptr + np.arange(N)) % RING).to("cuda:0")
            for k, x in zip(RING_KEYS, (buf.states, buf.next_states, buf.actions, buf.rewards, buf.dones)):
                out[k].append(raw(x[rows]))
        else:
            o, r, d, i = env.step(a)
        s, ep, tot = env.get_state()
        for k, x in zip(ENV_KEYS[:7], (o, r, d, i, s, ep, tot)):
            out[k].append(raw(x))
        obs = env.reset_done()
        out["obs_next"].append(raw(obs))
    env.close()
    return {k: np.stack(v) for k, v in out.items()}


def run_rollout(precision, case, rollout_lanes=0):
    """The same T steps as ONE mn_rollout launch with the actions given.  Returns the traces and the final observations / state as raw bits."""
    import torch
    env, _ = make_env(precision, case, rollout_lanes=rollout_lanes)
    a = torch.from_numpy(np.stack([actions(t) for t in range(T)])).to("cuda:0")
    tr = env.rollout(T, actions=a, trace=("obs", "reward", "done", "info"))
    out = {k: raw(tr[k]) for k in ("obs", "reward", "done", "info")}
    out["final_obs"] = raw(tr["final_obs"])
    s, ep, tot = env.get_state()
    out["state"], out["ep_t"], out["tot_t"] = raw(s), raw(ep), raw(tot)
    env.close()
    return out


def snapped_hits(z, precision):
    """How often the S3 case reports a hit of an exactly vertical beam: robot-frame hit point (t sin theta, t cos theta) with theta = 0 or pi, i.e.
    x exactly +-0 and y != 0 (an unsnapped beam pi/2 off the heading has x = t cos(pi/2) = 6e-17 t)."""
    obs = z[f"{precision}/S3/obs"].view(np.float32).reshape(T, N, 13, 2)
    outer = obs[:, :, [2, 12], :]
    return int(((outer[..., 0] == 0) & (outer[..., 1] != 0)).sum())


def record(path=FIXTURE):
    z = {}
    for prec, case in CASES:
        for k, v in run_loop(prec, case, append=True).items():
            z[f"{prec}/{case}/{k}"] = v
    for prec in ("f64", "mixed"):
        assert snapped_hits(z, prec) > 0, "the S3 case must exercise a snapped beam"
        for case in ("default", "S3"):      # a clock that starts at k runs out at step 5 - k and every 6 steps from there: every env ends at least once
            assert (z[f"{prec}/{case}/done"].sum(axis=0) >= 1).all()
    np.savez_compressed(path, **z)
    print("wrote", path, os.path.getsize(path), "bytes;", {p: snapped_hits(z, p) for p in ("f64", "mixed")}, "snapped hits")


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(HERE))
    record(*sys.argv[1:2])
