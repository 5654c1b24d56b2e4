"""Batched marinenav_env on one MI355X: host mirror of the reference's MarineNavEnv
(marinenav_env/envs/marinenav_env.py) over the C-ABI in include/marinenav_hip.h.

All per-step data stays in HBM as torch tensors; this class only owns buffers and forwards raw
device pointers + the current HIP stream to the hand-written gfx950 kernels.
"""
import ctypes as C

import numpy as np
import torch

from .. import _capi
from .._capi import MAX_CORES, MAX_OBS, OBS_DIM, INFO_STRINGS
from ..episodes import trace_buffers

_ATTR_TO_PARAM = {
    # MarineNavEnv attribute (marinenav_env.py:40-73) -> mn_params field
    "width": "width", "height": "height", "r": "core_r", "v_rel_max": "v_rel_max", "p": "p",
    "clear_r": "clear_r", "goal_dis": "goal_dis", "timestep_penalty": "timestep_penalty",
    "collision_penalty": "collision_penalty", "goal_reward": "goal_reward", "discount": "discount",
    "num_cores": "num_cores", "num_obs": "num_obs", "min_start_goal_dis": "min_start_goal_dis",
    "reset_start_and_goal": "reset_start_and_goal", "random_reset_state": "random_reset_state",
    "set_boundary": "set_boundary", "init_theta": "init_theta", "init_speed": "init_speed",
}


def _ptr(t):
    return C.c_void_p(t.data_ptr())


def _np_ptr(a, ctype):
    return a.ctypes.data_as(C.POINTER(ctype))


def shard_seeds(n_envs, seed=0, first_index=0):
    """Default per-env seeds of a shard: env i of the shard is global env `first_index + i` and is seeded with
    `seed + first_index + i` (mod 2^32, np.random.RandomState's seed range), so rank r of a multi-GPU run
    (first_index = r * n_envs) generates exactly the worlds of rows [r n, (r+1) n) of a one-GPU run."""
    if n_envs <= 0 or first_index < 0:
        raise ValueError("shard_seeds: n_envs must be positive and first_index non-negative")
    return ((np.arange(int(n_envs), dtype=np.uint64) + np.uint64(int(seed) % (1 << 32)) + np.uint64(int(first_index)))
            & np.uint64(0xFFFFFFFF)).astype(np.uint32)


def stacked_seeds(n_envs, seeds):
    """Per-env seeds of a STACKED env: the rows of `len(seeds)` envs of `n_envs` rows each, one after the other -- rows [g n, (g + 1) n) are seeded as
    `VecMarineNavEnv(n_envs, seed=seeds[g])` seeds its own (`shard_seeds`), so they generate that env's worlds bit for bit."""
    return np.concatenate([shard_seeds(n_envs, s) for s in seeds])


class StackedRows:
    """The rows [g n, (g + 1) n) of a stacked `VecMarineNavEnv` -- one seed's envs among those of G seeds that share ONE handle (`stacked_seeds`) -- as
    the train env of that seed's loop (`iqn.agent.VecLoop` with `collect_given`, `IQNAgent.vec_finish`): `n_envs`, `discount`, the seed's slice of the
    stacked `reset()` (which runs once, at the first view that asks), `join_reset`.  The stacked env is stepped, reset and closed by its owner, once for all
    views: `close` here does nothing."""

    def __init__(self, stacked, group, n_envs):
        self.stacked, self.group, self.n_envs = stacked, int(group), int(n_envs)
        if self.n_envs < 1 or self.group < 0 or (self.group + 1) * self.n_envs > stacked.n_envs:
            raise ValueError(f"StackedRows: rows [{self.group * self.n_envs}, {(self.group + 1) * self.n_envs}) are not rows of an env of {stacked.n_envs}")
        self.device = stacked.device

    @property
    def discount(self):
        return self.stacked.discount

    @property
    def rows(self):
        return slice(self.group * self.n_envs, (self.group + 1) * self.n_envs)

    def reset(self):
        st = self.stacked
        if not getattr(st, "_stack_was_reset", False):
            st.reset()
            st._stack_was_reset = True
        return st.obs[self.rows]

    def join_reset(self):
        self.stacked.join_reset()

    def close(self):
        pass


class VecMarineNavEnv:
    """n_envs independent MarineNavEnv instances stepped by one kernel launch.

    Env i is seeded with ``seeds[i]`` (default ``seed + first_index + i``) exactly like
    ``MarineNavEnv(seed=...)`` (marinenav_env.py:27,75-78): the same seed reproduces the
    reference's worlds bit for bit.
    """

    def __init__(self, n_envs, seed=0, seeds=None, schedule=None, device="cuda:0", precision="mixed",
                 timestep_scale=1.0, first_index=0, params=None, step_lanes=0, rollout_lanes=0, obs64=False):
        if not torch.cuda.is_available():
            raise _capi.MarineNavHipError("VecMarineNavEnv needs a ROCm GPU (MI355X); there is no CPU fallback")
        self.L = _capi.lib()
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _capi.MarineNavHipError(f"VecMarineNavEnv(device={device!r}): the env kernels are HIP kernels for gfx950 -- there is no CPU path (the reference's "
                                          "`-D cpu` has no counterpart here; the CPU restatement under oracle/ is test infrastructure)")
        torch.cuda.set_device(self.device)
        self.n_envs = int(n_envs)
        self.params = params if params is not None else _capi.default_params()
        self.params.precision = _capi.PRECISION_F64 if precision in ("f64", "float64", 0) else _capi.PRECISION_MIXED
        self.precision = "f64" if self.params.precision == _capi.PRECISION_F64 else "mixed"
        self.params.step_lanes = int(step_lanes)
        self.params.rollout_lanes = int(rollout_lanes)
        h = C.c_void_p()
        rc = self.L.mn_create(self.n_envs, C.byref(self.params), C.byref(h))
        if rc:
            raise _capi.MarineNavHipError(f"mn_create failed ({rc}): {self.L.mn_last_error(None).decode()}")
        self.h = h
        self.first_index = int(first_index)
        self.obs_noise = None      # set_obs_noise
        self.obs64_enabled = False
        if obs64:      # float64 copies of observations / rewards (parity checks, the n = 1 facade); off in the training loop
            self.enable_obs64(True)
        if seeds is None:
            seeds = shard_seeds(self.n_envs, seed, first_index)
        self.seed(seeds)
        self.schedule = None
        if schedule is not None:
            self.set_schedule(schedule, timestep_scale)
        dev = self.device
        # observations are double-buffered: step() writes the half that does NOT hold the
        # observations returned by the previous step()/reset(), so (obs_t, obs_t+1) are both
        # resident for the replay append without a copy
        self._obs_bufs = [torch.zeros(self.n_envs, OBS_DIM, dtype=torch.float32, device=dev) for _ in range(2)]
        self._cur = 0
        self.obs = self._obs_bufs[0]
        self.reward = torch.zeros(self.n_envs, dtype=torch.float32, device=dev)
        self.done = torch.zeros(self.n_envs, dtype=torch.uint8, device=dev)
        self.info = torch.zeros(self.n_envs, dtype=torch.uint8, device=dev)
        self._terminal_obs = None
        self.late_rows = None      # reset_done(under_next_act=True)
        self.reset_under_act_max = self.RESET_UNDER_ACT_MAX_DEFAULT
        self.reset_launches = [0, 0]      # ... how many of those calls the library ran [in front of, under] the next act kernel
        self.reset_owed = False           # ... and whether the last one left its resets to the next act call (`eps` given: mn_reset_done_next_act)
        self.resets_owed = 0              # how many did (they count in reset_launches[0]: such a reset runs in front of the act kernel, inside its preparation launch)
        self.reset_owed_max_rows = self.RESET_OWED_MAX_ROWS_DEFAULT

    # ---- lifecycle ---------------------------------------------------------------------------
    def close(self):
        if getattr(self, "h", None) is not None and self.h:
            torch.cuda.synchronize(self.device)
            self.L.mn_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _stream(self):
        return _capi.stream_ptr(self.device)

    def _check(self, rc):
        _capi.check(rc, self.h)

    # ---- configuration -----------------------------------------------------------------------
    def seed(self, seeds):
        """MarineNavEnv.seed (marinenav_env.py:75-78) per env."""
        s = np.ascontiguousarray(np.broadcast_to(np.asarray(seeds, dtype=np.uint32), (self.n_envs,)))
        self._check(self.L.mn_seed(self.h, _np_ptr(s, C.c_uint32), self._stream()))
        self.seeds = s
        return list(s)

    def set_schedule(self, schedule, timestep_scale=1.0):
        """`schedule` ctor argument (marinenav_env.py:27,89-98); None clears it."""
        if schedule is None:
            self._check(self.L.mn_set_schedule(self.h, 0, None, None, None, None, 1.0))
            self.schedule = None
            return
        ts = np.ascontiguousarray(schedule["timesteps"], dtype=np.int64)
        nc = np.ascontiguousarray(schedule["num_cores"], dtype=np.int32)
        no = np.ascontiguousarray(schedule["num_obstacles"], dtype=np.int32)
        md = np.ascontiguousarray(schedule["min_start_goal_dis"], dtype=np.float64)
        self._check(self.L.mn_set_schedule(self.h, len(ts), _np_ptr(ts, C.c_int64), _np_ptr(nc, C.c_int32),
                                           _np_ptr(no, C.c_int32), _np_ptr(md, C.c_double), float(timestep_scale)))
        self.schedule = schedule

    def set_attrs(self, **kw):
        """Attribute writes of the reference (`env.num_cores = 4`, `env.robot.N = 5`, ...)."""
        for k, v in kw.items():
            if k in _ATTR_TO_PARAM:
                setattr(self.params, _ATTR_TO_PARAM[k], type(getattr(self.params, _ATTR_TO_PARAM[k]))(v))
            elif k in ("N", "dt", "max_speed", "robot_r", "sonar_range", "sonar_angle"):
                setattr(self.params, k, type(getattr(self.params, k))(v))
            elif k in ("v_range", "obs_r_range", "a", "w"):
                arr = getattr(self.params, k)
                for i, x in enumerate(v):
                    arr[i] = float(x)
            else:
                raise AttributeError(f"unknown env attribute {k}")
        self._check(self.L.mn_set_params(self.h, C.byref(self.params)))

    def set_start_goal(self, start, goal, env_idx=-1):
        s = (C.c_double * 2)(float(start[0]), float(start[1]))
        g = (C.c_double * 2)(float(goal[0]), float(goal[1]))
        torch.cuda.synchronize(self.device)
        self._check(self.L.mn_set_start_goal(self.h, int(env_idx), s, g))

    # ---- gym-shaped batched API --------------------------------------------------------------
    def get_state_space_dimension(self):
        return OBS_DIM

    def get_action_space_dimension(self):
        return _capi.NUM_ACTIONS

    @property
    def discount(self):
        return self.params.discount

    def reset(self, mask=None):
        """MarineNavEnv.reset for every env (or the masked ones).  Returns obs [n,26] f32 (device)."""
        m = None
        if mask is not None:
            m = mask.to(device=self.device, dtype=torch.uint8).contiguous()
        self._check(self.L.mn_reset(self.h, _ptr(m) if m is not None else None, _ptr(self.obs), self._stream()))
        return self.obs

    def step(self, actions):
        """MarineNavEnv.step for every env; no auto-reset (like the reference).
        Returns (obs [n,26] f32, reward [n] f32, done [n] u8, info [n] u8 code) -- device tensors
        owned by the env; reward/done/info are overwritten by the next call, obs by the one after."""
        self._cur ^= 1
        self.obs = self._obs_bufs[self._cur]
        a = actions
        if a.dtype != torch.int32 or not a.is_contiguous() or a.device != self.device:
            a = a.to(device=self.device, dtype=torch.int32).contiguous()
        self._check(self.L.mn_step(self.h, _ptr(a), _ptr(self.obs), _ptr(self.reward), _ptr(self.done), _ptr(self.info),
                                   self._stream()))
        return self.obs, self.reward, self.done, self.info

    def step_append(self, actions, prev_obs, replay):
        """`step` + `replay.add` for every env in ONE launch (C-ABI mn_step_append): the transition
        (prev_obs[i], actions[i], reward, obs, done) of env i is written straight into the device ring of `replay`
        (iqn.replay_buffer.ReplayBuffer) by the step kernel.  `prev_obs` must be the tensor the last step()/reset()
        returned (the other half of the observation double buffer)."""
        self._cur ^= 1
        self.obs = self._obs_bufs[self._cur]
        a = actions
        if a.dtype != torch.int32 or not a.is_contiguous() or a.device != self.device:
            a = a.to(device=self.device, dtype=torch.int32).contiguous()
        assert prev_obs.data_ptr() != self.obs.data_ptr() and prev_obs.is_contiguous() and prev_obs.dtype == torch.float32
        self._check(self.L.mn_step_append(self.h, _ptr(a), _ptr(prev_obs), _ptr(self.obs), _ptr(self.reward), _ptr(self.done),
                                          _ptr(self.info), _ptr(replay.states), _ptr(replay.next_states), _ptr(replay.actions),
                                          _ptr(replay.rewards), _ptr(replay.dones), int(replay.ptr), int(replay.capacity),
                                          self._stream()))
        replay.advance(self.n_envs)
        return self.obs, self.reward, self.done, self.info

    def rollout(self, n_steps, actions=None, action_seed=0, first_step=0, trace=("obs", "reward", "done")):
        """`n_steps` vector steps with auto-reset in ONE launch (C-ABI mn_rollout): uniformly random actions drawn inside
        the kernel (counter-based: seed, step index, global env index = first_index + i), or `actions` [n_steps, n] i32.
        Bit-identical to n_steps x (step, reset_done).  Returns a dict with the final `obs` [n,26] (what the next act
        would see) and the requested traces: obs [T,n,26], reward [T,n], done [T,n] u8, info [T,n] u8, action [T,n] i32."""
        T, n, dev = int(n_steps), self.n_envs, self.device
        key = (T, tuple(sorted(trace)))
        bufs = getattr(self, "_rollout_bufs", None)
        if bufs is None or bufs[0] != key:
            bufs = self._rollout_bufs = (key, trace_buffers(T, n, dev, trace, fill=False))      # (with auto-reset every row is written)
        tr = bufs[1]
        a = None
        if actions is not None:
            a = actions.to(device=dev, dtype=torch.int32).contiguous()
            assert a.shape == (T, n)
        p = lambda k: _ptr(tr[k]) if k in tr else None
        self._check(self.L.mn_rollout(self.h, T, _ptr(a) if a is not None else None, int(action_seed), int(first_step),
                                      int(self.first_index), _ptr(self.obs), p("obs"), p("reward"), p("done"), p("info"), p("action"),
                                      self._stream()))
        out = dict(tr)
        out["final_obs"] = self.obs
        return out

    POLICIES = {"APF": 1, "BA": 2}      # MN_POLICY_APF / MN_POLICY_BA (include/marinenav_hip.h)

    def rollout_policy(self, n_steps, policy, trace=("reward", "done", "info", "action")):
        """Every env's CURRENT episode under the classical baseline `policy` ("APF" = APF.py:17-78, "BA" = BA.py:14-155) for up to
        `n_steps` steps in ONE launch (C-ABI mn_rollout_policy): the policy is evaluated on the device on each step's observation row.
        No resets: a finished env idles (reward 0, done 1, terminal info, action -1 in the traces).  Step for step identical to the
        loop (planners.planner_act_batch, step).  Returns the requested traces + `final_obs` (terminal observations where finished).  "traj" among the
        traces (f64 envs): [n_steps][n][N][2], every step's sub-step positions while the env is alive (NaN behind its end) -- the loop's `get_trajectory()`."""
        T, n, dev = int(n_steps), self.n_envs, self.device
        code = int(self.POLICIES[policy])      # (a wrong name raises before anything is attached)
        tr = trace_buffers(T, n, dev, trace, n_substeps=int(self.params.N))
        p = lambda k: _ptr(tr[k]) if k in tr else None
        self.set_trajectory_trace(tr.get("traj"))
        self._check(self.L.mn_rollout_policy(self.h, T, code, _ptr(self.obs), p("obs"), p("reward"), p("done"), p("info"),
                                             p("action"), self._stream()))
        out = dict(tr)
        out["final_obs"] = self.obs
        return out

    def random_actions(self, action_seed, step):
        """The actions `rollout(action_seed=...)` takes at step index `step` (int32 [n] on the device)."""
        a = torch.empty(self.n_envs, dtype=torch.int32, device=self.device)
        self._check(self.L.mn_random_actions(int(action_seed), int(step), int(self.first_index), self.n_envs, _ptr(a), self._stream()))
        return a

    def reset_done(self, keep_terminal_obs=False, under_next_act=False, eps=None, n_rows=None, fallback=False):
        """The caller-side `if done: state = env.reset()` (agent.py:152-170) for the whole batch.
        Overwrites the rows of finished envs in ``self.obs`` with their first observation; with
        keep_terminal_obs the pre-reset observations are preserved in ``self.terminal_obs``.
        `under_next_act` (mn_reset_done_async): the reset runs on the handle's own stream, off the caller's critical path; ``self.late_rows``
        = (done flags, "row is final" words, tick) is what the next act launch needs to take the finished envs' rows last
        (`fused_act(..., late_rows=env.take_late_rows())`).  Until `join_reset()` -- or the next step / reset of this env -- the rows of
        finished envs in ``self.obs`` must not be read by anything else on the caller's stream.
        `eps` (with `under_next_act`; mn_reset_done_next_act): the eps of the caller's next act call of `n_rows` rows (default: every env), and `fallback`: the
        caller's check of the under-act arrangement has failed (never under the act kernel).  The library may then OWE the reset (``self.reset_owed``):
        nothing is launched, and the next `fused_act(..., late_env=self)` runs it inside its preparation launch (set_reset_owed_max_rows has the rule);
        anything else that touches the env settles it with a plain reset launch first."""
        if keep_terminal_obs:
            if self._terminal_obs is None:
                self._terminal_obs = torch.empty_like(self.obs)
            self._terminal_obs.copy_(self.obs)
        self.reset_owed = False
        if under_next_act and eps is not None:
            ready, tick, place = C.c_void_p(), C.c_uint32(), C.c_int32()
            self._check(self.L.mn_reset_done_next_act(self.h, _ptr(self.obs), self._stream(), C.c_float(float(eps)), int(self.n_envs if n_rows is None else n_rows),
                                                      int(bool(fallback)), C.byref(ready), C.byref(tick), C.byref(place)))
            self.late_rows = (self.done, ready.value, tick.value) if ready.value else None
            self.reset_owed = place.value == _capi.RESET_OWED
            self.resets_owed += int(self.reset_owed)
            if not fallback:      # (reset_launches counts the calls of a loop that asks for resets under the act kernel, as before)
                self.reset_launches[1 if ready.value else 0] += 1
        elif under_next_act:
            ready, tick = C.c_void_p(), C.c_uint32()
            self._check(self.L.mn_reset_done_async(self.h, _ptr(self.obs), self._stream(), C.byref(ready), C.byref(tick)))
            # (the library runs it in front after all -- ready NULL -- while many episodes end per vector step: set_reset_under_act_max)
            self.late_rows = (self.done, ready.value, tick.value) if ready.value else None
            self.reset_launches[1 if ready.value else 0] += 1
        else:
            self.late_rows = None
            self._check(self.L.mn_reset_done(self.h, _ptr(self.obs), self._stream()))
        return self.obs

    RESET_UNDER_ACT_MAX_DEFAULT = 5000      # = MN_RESET_UNDER_ACT_MAX_DEFAULT (include/marinenav_hip.h)

    def set_reset_under_act_max(self, max_resets=None):
        """`reset_done(under_next_act=True)` goes under the act kernel only while the decaying peak of the episodes started per reset launch is at most this
        (None: the library's default, 5000; 2**31 - 1: always, -1: never).  Returns that peak as of the last launch seen (-1: none yet)."""
        last = C.c_int64()
        self.reset_under_act_max = self.RESET_UNDER_ACT_MAX_DEFAULT if max_resets is None else int(max_resets)
        self._check(self.L.mn_set_reset_under_act_max(self.h, self.reset_under_act_max, C.byref(last)))
        return last.value

    RESET_OWED_MAX_ROWS_DEFAULT = 500      # = MN_RESET_OWED_MAX_ROWS_DEFAULT (include/marinenav_hip.h)

    def set_reset_owed_max_rows(self, max_rows=None):
        """`reset_done(under_next_act=True, eps=...)` leaves the reset to the next act call's preparation launch while that call evaluates at most this many
        rows, (1 - eps) n_rows, and wherever the reset would otherwise run in front of the act kernel (None: the library's default, 500; -1: never; 2**31 - 1:
        always, except while `set_reset_under_act_max(2**31 - 1)` forces every reset under the act kernel)."""
        self.reset_owed_max_rows = self.RESET_OWED_MAX_ROWS_DEFAULT if max_rows is None else int(max_rows)
        self._check(self.L.mn_set_reset_owed_max_rows(self.h, self.reset_owed_max_rows))

    def take_owed_reset(self):
        """True once if the last `reset_done(under_next_act=True, eps=...)` left its resets to the next act call (which then acts through mn_iqn_act_rng_env)."""
        owed, self.reset_owed = getattr(self, "reset_owed", False), False
        return owed

    def debug_side_delay_us(self, us):
        """Test hook (mn_debug_side_delay_us): every reset launch under the act kernel is held back by `us` microseconds on the handle's own stream."""
        self._check(self.L.mn_debug_side_delay_us(self.h, int(us)))

    def debug_read(self, field):
        """Test hook (mn_debug_read): a raw device array of the handle as a numpy array, padding included -- "mt" [npad, 624] u32, "mt_pos" [npad] i32, and the
        compact tables "qcx" "qcy" [8, npad] i32, "qcg" [8, npad] f32, "qox" "qoy" [10, npad] i32, "qor" [10, npad] f32."""
        npad = (self.n_envs + 255) // 256 * 256
        code, shape, dt = {"mt": (0, (npad, 624), np.uint32), "mt_pos": (1, (npad,), np.int32), "qcx": (2, (MAX_CORES, npad), np.int32),
                           "qcy": (3, (MAX_CORES, npad), np.int32), "qcg": (4, (MAX_CORES, npad), np.float32), "qox": (5, (MAX_OBS, npad), np.int32),
                           "qoy": (6, (MAX_OBS, npad), np.int32), "qor": (7, (MAX_OBS, npad), np.float32)}[field]
        out = np.zeros(shape, dt)
        self._check(self.L.mn_debug_read(self.h, code, out.ctypes.data_as(C.c_void_p), out.nbytes))
        return out

    def take_late_rows(self):
        """The pending `reset_done(under_next_act=True)`'s late rows for ONE act launch (None if there is none)."""
        lr, self.late_rows = getattr(self, "late_rows", None), None
        return lr

    def join_reset(self):
        """Everything enqueued on the current stream from here on runs after a pending `reset_done(under_next_act=True)`; an owed one is launched here."""
        self.late_rows = None
        self.reset_owed = False
        self._check(self.L.mn_reset_join(self.h, self._stream()))

    @property
    def terminal_obs(self):
        return self._terminal_obs

    def step_autoreset(self, actions, keep_terminal_obs=False):
        """step + reset_done.  Returns (obs_for_next_act, reward, done, info)."""
        self.step(actions)
        self.reset_done(keep_terminal_obs)
        return self.obs, self.reward, self.done, self.info

    def last_done_count(self):
        out = C.c_int32()
        self._check(self.L.mn_last_done_count(self.h, self._stream(), C.byref(out)))
        return out.value

    # ---- worlds ------------------------------------------------------------------------------
    def load_worlds(self, worlds, first_env=0, repeat=1):
        """reset_with_eval_config (marinenav_env.py:467-555) for consecutive envs.  `worlds` is a
        list of dicts with keys cores [n,4]=(x,y,clockwise,Gamma), obstacles [n,3]=(x,y,r), start,
        goal, init_theta, init_speed.  Returns the first observations of those envs.  `repeat` > 1: the list that many times in a row (what
        `worlds * repeat` loads, without walking the list again for every copy)."""
        cnt = len(worlds)
        ncs = np.zeros(cnt, np.int32); nos = np.zeros(cnt, np.int32)
        cxy = np.zeros((cnt, MAX_CORES, 2)); cw = np.zeros((cnt, MAX_CORES), np.int32); gm = np.zeros((cnt, MAX_CORES))
        oxy = np.zeros((cnt, MAX_OBS, 2)); orr = np.zeros((cnt, MAX_OBS))
        st = np.zeros((cnt, 2)); gl = np.zeros((cnt, 2)); th = np.zeros(cnt); sp = np.zeros(cnt)
        for i, w in enumerate(worlds):
            c = np.asarray(w["cores"], dtype=np.float64).reshape(-1, 4)
            o = np.asarray(w["obstacles"], dtype=np.float64).reshape(-1, 3)
            if len(c) > MAX_CORES or len(o) > MAX_OBS:
                raise ValueError("world exceeds device capacity (8 cores, 10 obstacles)")
            ncs[i], nos[i] = len(c), len(o)
            cxy[i, :len(c)] = c[:, :2]; cw[i, :len(c)] = c[:, 2] != 0; gm[i, :len(c)] = c[:, 3]
            oxy[i, :len(o)] = o[:, :2]; orr[i, :len(o)] = o[:, 2]
            st[i] = w["start"]; gl[i] = w["goal"]; th[i] = w["init_theta"]; sp[i] = w["init_speed"]
        if repeat > 1:
            cnt *= int(repeat)
            ncs, nos, cxy, cw, gm, oxy, orr, st, gl, th, sp = (np.ascontiguousarray(np.concatenate([x] * int(repeat)))
                                                               for x in (ncs, nos, cxy, cw, gm, oxy, orr, st, gl, th, sp))
        d = C.c_double
        self._check(self.L.mn_load_worlds(self.h, int(first_env), cnt, _np_ptr(ncs, C.c_int32), _np_ptr(cxy, d),
                                          _np_ptr(cw, C.c_int32), _np_ptr(gm, d), _np_ptr(nos, C.c_int32), _np_ptr(oxy, d),
                                          _np_ptr(orr, d), _np_ptr(st, d), _np_ptr(gl, d), _np_ptr(th, d), _np_ptr(sp, d),
                                          _ptr(self.obs), self._stream()))
        return self.obs[first_env:first_env + cnt]

    @staticmethod
    def world_from_eval_config(cfg):
        """One entry of eval_config.json (episode_data schema, marinenav_env.py:557-622) -> world dict."""
        e, r = cfg["env"], cfg["robot"]
        nc, no = len(e["cores"]["positions"]), len(e["obstacles"]["positions"])
        cores = np.zeros((nc, 4)); obst = np.zeros((no, 3))
        if nc:
            cores[:, :2] = e["cores"]["positions"]; cores[:, 2] = e["cores"]["clockwise"]; cores[:, 3] = e["cores"]["Gamma"]
        if no:
            obst[:, :2] = e["obstacles"]["positions"]; obst[:, 2] = e["obstacles"]["r"]
        return dict(cores=cores, obstacles=obst, start=e["start"], goal=e["goal"],
                    init_theta=r["init_theta"], init_speed=r["init_speed"])

    def get_worlds(self, first_env=0, count=None):
        cnt = self.n_envs - first_env if count is None else count
        ncs = np.zeros(cnt, np.int32); nos = np.zeros(cnt, np.int32)
        cxy = np.zeros((cnt, MAX_CORES, 2)); cw = np.zeros((cnt, MAX_CORES), np.int32); gm = np.zeros((cnt, MAX_CORES))
        oxy = np.zeros((cnt, MAX_OBS, 2)); orr = np.zeros((cnt, MAX_OBS))
        st = np.zeros((cnt, 2)); gl = np.zeros((cnt, 2)); th = np.zeros(cnt); sp = np.zeros(cnt)
        d = C.c_double
        torch.cuda.synchronize(self.device)
        self._check(self.L.mn_get_worlds(self.h, int(first_env), cnt, _np_ptr(ncs, C.c_int32), _np_ptr(cxy, d),
                                         _np_ptr(cw, C.c_int32), _np_ptr(gm, d), _np_ptr(nos, C.c_int32), _np_ptr(oxy, d),
                                         _np_ptr(orr, d), _np_ptr(st, d), _np_ptr(gl, d), _np_ptr(th, d), _np_ptr(sp, d)))
        out = []
        for i in range(cnt):
            c = np.concatenate([cxy[i, :ncs[i]], cw[i, :ncs[i], None].astype(np.float64), gm[i, :ncs[i], None]], axis=1)
            o = np.concatenate([oxy[i, :nos[i]], orr[i, :nos[i], None]], axis=1)
            out.append(dict(cores=c, obstacles=o, n_cores=int(ncs[i]), n_obs=int(nos[i]), start=st[i].copy(),
                            goal=gl[i].copy(), init_theta=float(th[i]), init_speed=float(sp[i])))
        return out

    # ---- queries: ask a world without stepping it --------------------------------------------
    def _query_env(self, env, n_queries):
        """(index tensor or None, env0) of a query call: `env` is one world for every query (int) or an int tensor / array [Q]."""
        if isinstance(env, (int, np.integer)):
            return None, int(env)
        idx = torch.as_tensor(env).to(device=self.device, dtype=torch.int32).contiguous()
        if idx.shape != (n_queries,):
            raise ValueError(f"env must be an int or hold one index per query ({n_queries}), got shape {tuple(idx.shape)}")
        return idx, 0

    def velocity_at(self, xy, env=0):
        """MarineNavEnv.get_velocity (marinenav_env.py:422-455) at the points `xy` [Q, 2] of world `env` (an int, or one index per
        point): float64 [Q, 2] on the device (C-ABI mn_query_velocity).  Reads the world tables only; nothing in the env changes."""
        p = torch.as_tensor(xy).to(device=self.device, dtype=torch.float64).reshape(-1, 2).contiguous()
        q = p.shape[0]
        idx, env0 = self._query_env(env, q)
        v = torch.empty(q, 2, dtype=torch.float64, device=self.device)
        self._check(self.L.mn_query_velocity(self.h, _ptr(idx) if idx is not None else None, env0, _ptr(p), q, _ptr(v), self._stream()))
        return v

    def observation_at(self, states, env=0, velocity=None, dtype=torch.float32, return_flags=False):
        """get_observation() (marinenav_env.py:273-326) of a robot in `states` -- [Q, 6] = x, y, theta, speed, velocity_x, velocity_y (the
        columns of get_state), or [Q, 4] = x, y, theta, speed -- in world `env` (an int, or one index per state); host arrays are copied.
        velocity="given" reports the velocity of columns 4-5 (a state after a step); "current" sets it to speed (cos theta, sin theta) +
        the current at (x, y), like a robot placed there by reset (robot.py:79-87); default: "current" for [Q, 4], "given" for [Q, 6].
        Returns the rows [Q, 26] as `dtype` (float32: the cast of the float64 row) on the device, with return_flags also uint8 [Q]:
        _capi.QUERY_FLAG_COLLISION | _OUTSIDE | _GOAL, independent bits; _BAD_ENV: the index was no env, the row is NaN.  C-ABI
        mn_query_observation: float64 arithmetic on the master tables whatever the env's precision; nothing in the env changes."""
        st = torch.as_tensor(states).to(device=self.device, dtype=torch.float64)
        if st.dim() != 2 or st.shape[1] not in (4, 6):
            raise ValueError(f"states must be [Q, 4] or [Q, 6], got {tuple(st.shape)}")
        if velocity is None:
            velocity = "current" if st.shape[1] == 4 else "given"
        if velocity not in ("current", "given"):
            raise ValueError(f"velocity must be 'current' or 'given', got {velocity!r}")
        if st.shape[1] == 4:
            if velocity == "given":
                raise ValueError("velocity='given' needs states [Q, 6] (columns 4-5 are the velocity)")
            st = torch.cat([st, st.new_zeros(st.shape[0], 2)], dim=1)
        st = st.contiguous()
        if dtype not in (torch.float32, torch.float64):
            raise ValueError("dtype must be torch.float32 or torch.float64")
        q = st.shape[0]
        idx, env0 = self._query_env(env, q)
        obs = torch.empty(q, OBS_DIM, dtype=dtype, device=self.device)
        flags = torch.empty(q, dtype=torch.uint8, device=self.device) if return_flags else None
        mode = _capi.QUERY_VELOCITY_FROM_CURRENT if velocity == "current" else _capi.QUERY_VELOCITY_GIVEN
        self._check(self.L.mn_query_observation(self.h, _ptr(idx) if idx is not None else None, env0, _ptr(st), mode, q,
                                                _ptr(obs) if dtype == torch.float32 else None, _ptr(obs) if dtype == torch.float64 else None,
                                                _ptr(flags) if flags is not None else None, self._stream()))
        return (obs, flags) if return_flags else obs

    ROLLOUT_TRACES = ("reward", "done", "info", "action", "state", "traj")

    def rollout_at(self, states, actions, lengths=None, env=0, episode_timesteps=None, trace=(), dtype=torch.float32):
        """Open-loop rollouts of robots placed by hand (C-ABI mn_query_rollout: one HIP launch, float64 in the reference's own arithmetic
        whatever the env's precision; nothing in the env changes, no random number is drawn).  `states` [Q, 6] or [Q, 4] as in observation_at (a
        step ignores the velocity columns), in world `env` (an int, or one index per query).  `actions` (int): [H] -- one sequence shared by every
        query --, or [Q, H] -- a sequence per query; for one action per query held over H steps use `actions[:, None].expand(Q, H)` or
        `constant_rollout_at`.  `lengths` [Q]: query q runs at most lengths[q] <= H steps (default H); every query stops at the step that ends its
        episode.  `episode_timesteps` [Q] or an int: the counter before the first step (default 0).
        Returns a dict of device tensors: `state` [Q, 6] float64, `obs` [Q, 26] `dtype`, `reward` [Q] float64 (the last step's), `done`, `info` [Q]
        uint8, `steps` [Q] int32, and per name in `trace` (ROLLOUT_TRACES) `<name>_trace` in the episode launches' [H][Q] layout (reward float64,
        undiscounted; state [H][Q][6]; traj [H][Q][N][2]) -- episodes.tally takes reward / done / info / action as they are.  Behind a query's last
        step the rows hold reward 0, done 1, the last info code, action -1.  A query with an index that is no env, a non-finite state or
        |theta| >= 1e6, or an action outside [0, 9) is poisoned alone: NaN floats, done 1, info _capi.QUERY_FLAG_BAD_ENV / QUERY_INFO_BAD_STATE."""
        act = torch.as_tensor(actions).to(device=self.device, dtype=torch.int32)
        if act.dim() not in (1, 2):
            raise ValueError(f"actions must be [H] or [Q, H], got {tuple(act.shape)}")
        mode = _capi.QUERY_ACTIONS_SHARED if act.dim() == 1 else _capi.QUERY_ACTIONS_PER_QUERY
        return self._rollout_query(states, act.contiguous(), mode, int(act.shape[-1]), lengths, env, episode_timesteps, trace, dtype)

    def constant_rollout_at(self, states, actions, horizon, lengths=None, env=0, episode_timesteps=None, trace=(), dtype=torch.float32):
        """rollout_at with ONE action per query, `actions` [Q], held for `horizon` steps (an action fan)."""
        act = torch.as_tensor(actions).to(device=self.device, dtype=torch.int32).reshape(-1).contiguous()
        return self._rollout_query(states, act, _capi.QUERY_ACTIONS_CONSTANT, int(horizon), lengths, env, episode_timesteps, trace, dtype)

    def step_at(self, states, actions, env=0, episode_timesteps=None, dtype=torch.float32):
        """The what-if step: MarineNavEnv.step (marinenav_env.py:199-262) of a robot in `states` [Q, 6] or [Q, 4] taking `actions` [Q] (or one int
        for all) in world `env`, as rollout_at with H = 1.  Returns dict(state [Q, 6] float64, obs [Q, 26] `dtype`, reward [Q] float64, done,
        info [Q] uint8)."""
        if isinstance(actions, (int, np.integer)):
            act = torch.tensor([int(actions)], dtype=torch.int32, device=self.device)
            out = self._rollout_query(states, act, _capi.QUERY_ACTIONS_SHARED, 1, None, env, episode_timesteps, (), dtype)
        else:
            act = torch.as_tensor(actions).to(device=self.device, dtype=torch.int32).reshape(-1).contiguous()
            out = self._rollout_query(states, act, _capi.QUERY_ACTIONS_CONSTANT, 1, None, env, episode_timesteps, (), dtype)
        del out["steps"]
        return out

    def _rollout_query(self, states, act, mode, horizon, lengths, env, episode_timesteps, trace, dtype):
        st = torch.as_tensor(states).to(device=self.device, dtype=torch.float64)
        if st.dim() != 2 or st.shape[1] not in (4, 6):
            raise ValueError(f"states must be [Q, 4] or [Q, 6], got {tuple(st.shape)}")
        if st.shape[1] == 4:
            st = torch.cat([st, st.new_zeros(st.shape[0], 2)], dim=1)
        st = st.contiguous()
        if dtype not in (torch.float32, torch.float64):
            raise ValueError("dtype must be torch.float32 or torch.float64")
        q, dev = st.shape[0], self.device
        if horizon < 0 or horizon > _capi.QUERY_MAX_STEPS:
            raise ValueError(f"the horizon must be in [0, {_capi.QUERY_MAX_STEPS}], got {horizon}")
        want = {_capi.QUERY_ACTIONS_SHARED: (horizon,), _capi.QUERY_ACTIONS_CONSTANT: (q,), _capi.QUERY_ACTIONS_PER_QUERY: (q, horizon)}[mode]
        if tuple(act.shape) != want:
            raise ValueError(f"actions must have shape {want} for {q} states, got {tuple(act.shape)}")
        unknown = [k for k in trace if k not in self.ROLLOUT_TRACES]
        if unknown:
            raise ValueError(f"unknown trace {unknown}: rollout_at traces are {self.ROLLOUT_TRACES}")
        idx, env0 = self._query_env(env, q)

        def per_query(v, name):
            if v is None:
                return None
            if isinstance(v, (int, np.integer)):
                return torch.full((q,), int(v), dtype=torch.int32, device=dev)
            t = torch.as_tensor(v).to(device=dev, dtype=torch.int32).contiguous()
            if t.shape != (q,):
                raise ValueError(f"{name} must hold one value per query ({q}), got shape {tuple(t.shape)}")
            return t
        ep = per_query(episode_timesteps, "episode_timesteps")
        ln = per_query(lengths, "lengths")
        out = dict(state=torch.empty(q, 6, dtype=torch.float64, device=dev), obs=torch.empty(q, OBS_DIM, dtype=dtype, device=dev),
                   reward=torch.empty(q, dtype=torch.float64, device=dev), done=torch.empty(q, dtype=torch.uint8, device=dev),
                   info=torch.empty(q, dtype=torch.uint8, device=dev), steps=torch.empty(q, dtype=torch.int32, device=dev))
        n_sub = int(self.params.N)
        shapes = dict(reward=((horizon, q), torch.float64), done=((horizon, q), torch.uint8), info=((horizon, q), torch.uint8),
                      action=((horizon, q), torch.int32), state=((horizon, q, 6), torch.float64), traj=((horizon, q, n_sub, 2), torch.float64))
        tr = {k: torch.empty(shapes[k][0], dtype=shapes[k][1], device=dev) for k in trace}
        p = lambda t: _ptr(t) if t is not None else None
        self._check(self.L.mn_query_rollout(
            self.h, p(idx), env0, _ptr(st), p(ep), mode, _ptr(act), horizon, p(ln), q, _ptr(out["state"]),
            _ptr(out["obs"]) if dtype == torch.float32 else None, _ptr(out["obs"]) if dtype == torch.float64 else None, _ptr(out["reward"]),
            _ptr(out["done"]), _ptr(out["info"]), _ptr(out["steps"]), p(tr.get("reward")), p(tr.get("done")), p(tr.get("info")), p(tr.get("action")),
            p(tr.get("state")), p(tr.get("traj")), self._stream()))
        for k, v in tr.items():
            out[k + "_trace"] = v
        return out

    def time_field(self, envs, nx, ny, speed=None, clearance=0.0, goals=None, max_sweeps=None, want_dir=True, want_sweeps=True):
        """Minimum-time-to-goal fields (C-ABI mn_time_field: one HIP launch, one workgroup per field; float64 on the master tables whatever the env's
        precision; nothing in the env changes).  `envs`: one world index (int: one field) or an int tensor / array [F], one world per field.  For every
        cell of the nx x ny grid over the map -- centre ((i + 0.5) width / nx, (j + 0.5) height / ny) -- the least travel time to the goal of a
        vehicle of constant speed `speed` through the water (default: the parameters' max_speed), carried by the current and kept
        r + robot_r + `clearance` away from every obstacle's centre, over the 16-direction stencil of include/marinenav_hip.h.  `goals` [F, 2]:
        another goal per field than the world's own.  `max_sweeps`: default 4 (nx + ny); raise it if a status says TIME_FIELD_NOT_CONVERGED.
        Returns device tensors (T [F, ny, nx] float64 -- +inf where the goal cannot be reached, NaN for a field whose world index or goal is bad --,
        dir [F, ny, nx] uint8 -- the stencil direction of the first move, 255 at sources, blocked and unreachable cells --, status [F] int32
        (_capi.TIME_FIELD_*), sweeps [F] int32); dir / sweeps are None with want_dir / want_sweeps off."""
        nx, ny = int(nx), int(ny)
        if isinstance(envs, (int, np.integer)):
            idx, env0, n = None, int(envs), 1
        else:
            idx = torch.as_tensor(envs).to(device=self.device, dtype=torch.int32).reshape(-1).contiguous()
            env0, n = 0, idx.shape[0]
        g = None
        if goals is not None:
            g = goals if torch.is_tensor(goals) else torch.from_numpy(np.array(goals, dtype=np.float64))      # (a list would pass through float32)
            g = g.to(device=self.device, dtype=torch.float64).contiguous()
            if g.shape != (n, 2):
                raise ValueError(f"goals must be [{n}, 2] (one goal per field), got {tuple(g.shape)}")
        nb = int(self.L.mn_time_field_workspace_bytes(nx, ny, n))
        cells = nx * ny if nb >= 0 else 0      # (a refused grid: the call below says why, and nothing is allocated for it)
        T = torch.empty(n, ny if cells else 0, nx if cells else 0, dtype=torch.float64, device=self.device)
        d = torch.empty(T.shape, dtype=torch.uint8, device=self.device) if want_dir else None
        status = torch.empty(n, dtype=torch.int32, device=self.device)
        sweeps = torch.empty(n, dtype=torch.int32, device=self.device) if want_sweeps else None
        ws = torch.empty(max(nb, 0) // 8, dtype=torch.float64, device=self.device)
        p = lambda t: _ptr(t) if t is not None and t.numel() else None
        self._check(self.L.mn_time_field(self.h, p(idx), env0, p(g), n, nx, ny, float(speed) if speed is not None else 0.0, float(clearance),
                                         int(max_sweeps) if max_sweeps is not None else 4 * (nx + ny), p(T), p(d), p(status), p(sweeps), p(ws),
                                         self._stream()))
        return T, d, status, sweeps

    # ---- the field pilot: follow a time field under the real dynamics -------------------------
    PILOT_WANTS = ("action", "scores", "steps", "infos", "flags")

    def _pilot_fields(self, fields, horizon):
        T = fields["T"] if isinstance(fields, dict) else fields
        T = torch.as_tensor(T).to(device=self.device, dtype=torch.float64)
        if T.dim() == 2:
            T = T[None]
        if T.dim() != 3:
            raise ValueError(f"fields must be [ny, nx] or [F, ny, nx], got {tuple(T.shape)}")
        return T.contiguous(), int(horizon)

    def pilot_act(self, states, fields, env=0, field_of_query=None, horizon=2, episode_timesteps=None, want=("action", "scores")):
        """The field pilot's action for robots placed by hand (C-ABI mn_pilot_act: one HIP launch, a row of 16 lanes per query; float64 in the
        what-if step's arithmetic whatever the env's precision; nothing in the env changes).  `states` [Q, 6] or [Q, 4] as in rollout_at, in world
        `env` (an int, or one index per query); `fields`: T [F, ny, nx] (or [ny, nx]) float64 as `time_field` returns it, query q on field
        `field_of_query[q]` (default: field 0); `episode_timesteps` [Q] or an int (default 0).  For each of the nine actions the robot is stepped up
        to `horizon` (1..16) times and its landing point scored with the interpolated field (include/marinenav_hip.h, "Field pilot"); the least
        (score, horizon - steps, action) wins.  Returns a dict with the names in `want` (PILOT_WANTS): action [Q] int32, scores [Q, 9] float64, steps
        [Q, 9] int32, infos [Q, 9] uint8, flags [Q] uint8.  A poisoned query (world or field index out of range, a BAD_ENV field, a state that is
        not finite) gets action -1, NaN scores and its flag (_capi.QUERY_FLAG_BAD_ENV, PILOT_FLAG_BAD_FIELD, QUERY_INFO_BAD_STATE)."""
        st = torch.as_tensor(states).to(device=self.device, dtype=torch.float64)
        if st.dim() != 2 or st.shape[1] not in (4, 6):
            raise ValueError(f"states must be [Q, 4] or [Q, 6], got {tuple(st.shape)}")
        if st.shape[1] == 4:
            st = torch.cat([st, st.new_zeros(st.shape[0], 2)], dim=1)
        st = st.contiguous()
        unknown = [k for k in want if k not in self.PILOT_WANTS]
        if unknown or not want:
            raise ValueError(f"want must name some of {self.PILOT_WANTS}, got {tuple(want)}")
        T, H = self._pilot_fields(fields, horizon)
        q, dev = st.shape[0], self.device
        idx, env0 = self._query_env(env, q)

        def per_query(v, name):
            if v is None:
                return None
            if isinstance(v, (int, np.integer)):
                return torch.full((q,), int(v), dtype=torch.int32, device=dev)
            t = torch.as_tensor(v).to(device=dev, dtype=torch.int32).contiguous()
            if t.shape != (q,):
                raise ValueError(f"{name} must hold one value per query ({q}), got shape {tuple(t.shape)}")
            return t
        ep = per_query(episode_timesteps, "episode_timesteps")
        fq = per_query(field_of_query, "field_of_query")
        shapes = dict(action=((q,), torch.int32), scores=((q, 9), torch.float64), steps=((q, 9), torch.int32), infos=((q, 9), torch.uint8),
                      flags=((q,), torch.uint8))
        out = {k: torch.empty(shapes[k][0], dtype=shapes[k][1], device=dev) for k in want}
        p = lambda t: _ptr(t) if t is not None else None
        self._check(self.L.mn_pilot_act(self.h, p(idx), env0, _ptr(st), p(ep), _ptr(T), p(fq), T.shape[0], T.shape[2], T.shape[1], H, q,
                                        p(out.get("action")), p(out.get("scores")), p(out.get("steps")), p(out.get("infos")), p(out.get("flags")),
                                        self._stream()))
        return out

    def rollout_pilot(self, n_steps, fields, field_of_env=None, horizon=2, trace=("reward", "done", "info", "action")):
        """Every env's CURRENT episode under the field pilot for up to `n_steps` steps in ONE launch (C-ABI mn_rollout_pilot; float64 envs only):
        rollout_policy's contract -- no resets, a finished env idles (reward 0, done 1, terminal info, action -1), "traj" among the traces records
        the sub-step positions -- with the pilot of `pilot_act` as the policy.  `fields`: T [F, ny, nx]; env i follows field `field_of_env[i]`, or
        field i by default (then F must be the number of envs).  Bit for bit the loop (get_state, pilot_act, step).  Returns the requested traces
        + `final_obs`."""
        T, n, dev = int(n_steps), self.n_envs, self.device
        F, H = self._pilot_fields(fields, horizon)
        fe = None
        if field_of_env is not None:
            fe = torch.as_tensor(field_of_env).to(device=dev, dtype=torch.int32).contiguous()
            if fe.shape != (n,):
                raise ValueError(f"field_of_env must hold one field index per env ({n}), got shape {tuple(fe.shape)}")
        tr = trace_buffers(T, n, dev, trace, n_substeps=int(self.params.N))
        p = lambda k: _ptr(tr[k]) if k in tr else None
        self.set_trajectory_trace(tr.get("traj"))
        self._check(self.L.mn_rollout_pilot(self.h, T, _ptr(F), _ptr(fe) if fe is not None else None, F.shape[0], F.shape[2], F.shape[1], H,
                                            _ptr(self.obs), p("obs"), p("reward"), p("done"), p("info"), p("action"), self._stream()))
        out = dict(tr)
        out["final_obs"] = self.obs
        return out

    # ---- state accessors (tests, checkpoints) ------------------------------------------------
    def get_state(self, first_env=0, count=None):
        cnt = self.n_envs - first_env if count is None else count
        s = np.zeros((cnt, 6)); ep = np.zeros(cnt, np.int32); tot = np.zeros(cnt, np.int64)
        torch.cuda.synchronize(self.device)
        self._check(self.L.mn_get_state(self.h, int(first_env), cnt, _np_ptr(s, C.c_double), _np_ptr(ep, C.c_int32),
                                        _np_ptr(tot, C.c_int64)))
        return s, ep, tot

    def set_state(self, state=None, episode_timesteps=None, total_timesteps=None, first_env=0):
        cnt = len(state) if state is not None else (len(episode_timesteps) if episode_timesteps is not None else len(total_timesteps))
        s = np.ascontiguousarray(state, dtype=np.float64) if state is not None else None
        ep = np.ascontiguousarray(episode_timesteps, dtype=np.int32) if episode_timesteps is not None else None
        tot = np.ascontiguousarray(total_timesteps, dtype=np.int64) if total_timesteps is not None else None
        torch.cuda.synchronize(self.device)
        self._check(self.L.mn_set_state(self.h, int(first_env), cnt,
                                        _np_ptr(s, C.c_double) if s is not None else None,
                                        _np_ptr(ep, C.c_int32) if ep is not None else None,
                                        _np_ptr(tot, C.c_int64) if tot is not None else None))

    # ---- snapshots: mark a point, go on, come back (C-ABI mn_state_save / mn_state_load) ------
    def state_bytes(self):
        return int(self.L.mn_state_bytes(self.h))

    def save_state(self, out=None):
        """Everything a later call on the handle reads -- pose, episode constants, counters, both sets of world tables, every env's RNG stream, the done-queue
        and the handle's host-side words -- packed by ONE launch into a uint8 device tensor (`out`, or a new one).  An owed reset is launched first and a reset
        under the act kernel joined, as by `join_reset()`.  The observation buffers are this object's, not the handle's: `state_dict()` has those too."""
        nb = self.state_bytes()
        if out is None:
            out = torch.empty(nb, dtype=torch.uint8, device=self.device)
        assert out.dtype == torch.uint8 and out.is_contiguous() and out.device == self.device and out.numel() >= nb
        self.late_rows = None
        self.reset_owed = False
        self._check(self.L.mn_state_save(self.h, _ptr(out), int(out.numel()), self._stream()))
        return out

    def load_state(self, blob):
        """Put a `save_state()` blob of this env -- or of another one with the same n_envs, precision, params and schedule -- back: from here on the handle
        behaves exactly as the saved one would have.  Anything else is refused (MarineNavHipError names the first difference) and changes nothing."""
        b = blob.to(device=self.device, dtype=torch.uint8).contiguous()
        self._check(self.L.mn_state_load(self.h, _ptr(b), int(b.numel()), self._stream()))
        self.late_rows = None
        self.reset_owed = False
        self._loaded_blob = b      # (the unpack launch may still be reading it)

    def state_dict(self):
        """The env as CPU tensors and plain numbers: the handle's blob (`save_state`, copied to the host), both observation buffers and which one is current,
        the last reward / done / info rows and the host counters.  `load_state_dict` of it into an env built with the same arguments continues bit for bit."""
        blob = self.save_state()
        sd = dict(n_envs=self.n_envs, precision=self.precision, blob=blob.cpu(), obs_bufs=[b.cpu() for b in self._obs_bufs], cur=int(self._cur),
                  reward=self.reward.cpu(), done=self.done.cpu(), info=self.info.cpu(),
                  terminal_obs=None if self._terminal_obs is None else self._terminal_obs.cpu(),
                  reset_launches=list(self.reset_launches), resets_owed=int(self.resets_owed), reset_under_act_max=int(self.reset_under_act_max),
                  reset_owed_max_rows=int(self.reset_owed_max_rows))
        return sd

    def load_state_dict(self, sd):
        if int(sd["n_envs"]) != self.n_envs or sd["precision"] != self.precision:
            raise _capi.MarineNavHipError(f"load_state_dict: the state is of {sd['n_envs']} envs in precision {sd['precision']!r}, this env has {self.n_envs} in "
                                          f"{self.precision!r}")
        self.load_state(sd["blob"])      # first: a refused blob leaves this object as it was
        for dst, src in zip(self._obs_bufs, sd["obs_bufs"]):
            dst.copy_(src)
        self._cur = int(sd["cur"])
        self.obs = self._obs_bufs[self._cur]
        self.reward.copy_(sd["reward"]); self.done.copy_(sd["done"]); self.info.copy_(sd["info"])
        if sd.get("terminal_obs") is not None:
            if self._terminal_obs is None:
                self._terminal_obs = torch.empty_like(self.obs)
            self._terminal_obs.copy_(sd["terminal_obs"])
        self.reset_launches = list(sd["reset_launches"])
        self.resets_owed = int(sd["resets_owed"])
        self.reset_under_act_max = int(sd["reset_under_act_max"])      # (the handle's own copies of the two thresholds came with the blob)
        self.reset_owed_max_rows = int(sd["reset_owed_max_rows"])
        torch.cuda.synchronize(self.device)

    def enable_obs64(self, on=True):
        """Keep float64 copies of every later step's / reset's observation rows and rewards (`get_obs64`, `get_reward64`; f64 handles).
        Off by default: the training loop never reads them (C-ABI mn_enable_obs64)."""
        torch.cuda.synchronize(self.device)
        self._check(self.L.mn_enable_obs64(self.h, 1 if on else 0))
        self.obs64_enabled = bool(on)

    def get_obs64(self, first_env=0, count=None):
        cnt = self.n_envs - first_env if count is None else count
        out = np.zeros((cnt, OBS_DIM))
        torch.cuda.synchronize(self.device)
        self._check(self.L.mn_get_obs64(self.h, int(first_env), cnt, _np_ptr(out, C.c_double)))
        return out

    def get_reward64(self, first_env=0, count=None):
        cnt = self.n_envs - first_env if count is None else count
        out = np.zeros(cnt)
        torch.cuda.synchronize(self.device)
        self._check(self.L.mn_get_reward64(self.h, int(first_env), cnt, _np_ptr(out, C.c_double)))
        return out

    def enable_trajectory(self, max_substeps=None):
        """Record the per-sub-step positions of every step (robot.trajectory, marinenav_env.py:211-212); f64 handles."""
        self._check(self.L.mn_enable_trajectory(self.h, int(self.params.N if max_substeps is None else max_substeps)))

    def set_trajectory_trace(self, traj):
        """Attach `traj` ([T][n][N][2] float64 on the device; C-ABI mn_set_trajectory_trace) to the NEXT episode launch of this env (rollout_policy,
        iqn.fused_act.rollout_iqn, DQNPolicy.rollout), which records every step's sub-step positions into it and detaches it; None detaches.  f64 envs."""
        if traj is None:
            self._check(self.L.mn_set_trajectory_trace(self.h, None, 0, 0))
            return
        assert traj.is_contiguous() and traj.dtype == torch.float64 and traj.shape[1:] == (self.n_envs, int(self.params.N), 2)
        self._check(self.L.mn_set_trajectory_trace(self.h, _ptr(traj), int(traj.shape[0]), int(self.params.N)))

    # ---- observation noise (obs_noise.py; C-ABI mn_set_obs_noise / mn_env_perturb_obs) --------
    def set_obs_noise(self, noise, first_index=None):
        """Attach an `obs_noise.ObsNoise` to this env (None detaches): `perturb` applies it, and the episode launches -- rollout_policy (f64 envs),
        iqn.fused_act.rollout_iqn's acting form, DQNPolicy.rollout -- feed their policy the perceived rows while every output stays the clean one.  It
        stays attached until replaced or detached.  step() and every other stepping call keep returning clean observations.  Row i is global env
        `first_index + i` in the noise key (default: the env's own first_index, as the seeds follow it)."""
        if noise is None:
            self._check(self.L.mn_set_obs_noise(self.h, None, 0))
        else:
            spec = noise.c_struct()
            self._check(self.L.mn_set_obs_noise(self.h, C.byref(spec), int(self.first_index if first_index is None else first_index)))
        self.obs_noise = noise

    def perturb(self, obs, out=None):
        """What the robot perceives of `obs` [n, 26] (the rows this env's last step() / reset() returned): the attached description under the key
        (seed, first_index + i, the env's episode_timesteps), one launch; a copy when nothing is attached.  `out` may be `obs` itself."""
        assert obs.is_contiguous() and obs.dtype == torch.float32 and obs.shape == (self.n_envs, OBS_DIM) and obs.device == self.device
        if out is None:
            out = torch.empty_like(obs)
        assert out.is_contiguous() and out.dtype == torch.float32 and out.shape == obs.shape and out.device == self.device
        self._check(self.L.mn_env_perturb_obs(self.h, _ptr(obs), _ptr(out), self._stream()))
        return out

    def get_trajectory(self, first_env=0, count=None):
        """[count, N, 2] positions after each of the N sub-steps of the last step()."""
        cnt = self.n_envs - first_env if count is None else count
        out = np.zeros((cnt, int(self.params.N), 2))
        torch.cuda.synchronize(self.device)
        self._check(self.L.mn_get_trajectory(self.h, int(first_env), cnt, int(self.params.N), _np_ptr(out, C.c_double)))
        return out

    def peek_next_double(self, first_env=0, count=None):
        cnt = self.n_envs - first_env if count is None else count
        out = np.zeros(cnt)
        torch.cuda.synchronize(self.device)
        self._check(self.L.mn_peek_next_double(self.h, int(first_env), cnt, _np_ptr(out, C.c_double)))
        return out

    # ---- profiling hook ----------------------------------------------------------------------
    def profile_begin(self, max_launches):
        self._check(self.L.mn_profile_begin(self.h, int(max_launches)))

    def profile_end(self):
        ms = C.c_double(); n = C.c_int32()
        self._check(self.L.mn_profile_end(self.h, self._stream(), C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def profile_reset_end(self):
        """Mean duration / count of the mn_reset_done launches recorded since profile_begin (call before profile_end)."""
        ms = C.c_double(); n = C.c_int32()
        self._check(self.L.mn_profile_reset_end(self.h, self._stream(), C.byref(ms), C.byref(n)))
        return ms.value, n.value

    @staticmethod
    def info_string(code):
        return INFO_STRINGS[int(code)]
