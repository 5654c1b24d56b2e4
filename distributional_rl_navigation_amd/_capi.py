"""ctypes binding of libmarinenav_hip.so (include/marinenav_hip.h).

There is no CPU fallback: if the gfx950 library is missing or no GPU is visible the product path
raises.  The oracle under /oracle is test infrastructure and is never imported from here.
"""
import ctypes as C
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libmarinenav_hip.so")

MAX_CORES, MAX_OBS, NUM_BEAMS, OBS_DIM, NUM_ACTIONS, MAX_STAGES = 8, 10, 11, 26, 9, 8
PRECISION_F64, PRECISION_MIXED = 0, 1
RESET_IN_FRONT, RESET_UNDER_ACT, RESET_OWED = 0, 1, 2      # mn_reset_placement / mn_reset_done_next_act (include/marinenav_hip.h)
QUERY_VELOCITY_GIVEN, QUERY_VELOCITY_FROM_CURRENT = 0, 1
QUERY_FLAG_COLLISION, QUERY_FLAG_OUTSIDE, QUERY_FLAG_GOAL, QUERY_FLAG_BAD_ENV = 1, 2, 4, 128
QUERY_ACTIONS_SHARED, QUERY_ACTIONS_CONSTANT, QUERY_ACTIONS_PER_QUERY = 0, 1, 2      # mn_query_rollout
QUERY_INFO_BAD_STATE, QUERY_MAX_STEPS = 64, 65536
RENDER_MAX_LEVELS, RENDER_MAX_LIC_STEPS, RENDER_MAX_HALF_WIDTH = 32, 64, 8      # mn_render_worlds / mn_render_draw
RENDER_SEGMENT, RENDER_DISC, RENDER_RING = 0, 1, 2
TIME_FIELD_MAX_CELLS, TIME_FIELD_NO_DIR = 16384, 255      # mn_time_field
TIME_FIELD_OK, TIME_FIELD_NOT_CONVERGED, TIME_FIELD_NO_SOURCE, TIME_FIELD_BAD_ENV = 0, 1, 2, 3
PILOT_MAX_HORIZON, PILOT_FLAG_BAD_FIELD = 16, 32      # mn_pilot_act / mn_rollout_pilot
RENDER_RECT, RENDER_MARKER, RENDER_GLYPH, RENDER_SECTOR = 4, 5, 6, 7      # (3 is unassigned)
RENDER_MARKER_SQUARE, RENDER_MARKER_PLUS, RENDER_MARKER_CROSS = 0, 1, 2
INFO_STRINGS = ("normal", "out of boundary", "too long episode", "collision", "reach goal")


class MnParams(C.Structure):
    _fields_ = [
        ("width", C.c_double), ("height", C.c_double), ("core_r", C.c_double), ("v_rel_max", C.c_double),
        ("p", C.c_double), ("v_range", C.c_double * 2), ("obs_r_range", C.c_double * 2), ("clear_r", C.c_double),
        ("goal_dis", C.c_double), ("timestep_penalty", C.c_double), ("collision_penalty", C.c_double),
        ("goal_reward", C.c_double), ("discount", C.c_double), ("min_start_goal_dis", C.c_double),
        ("init_theta", C.c_double), ("init_speed", C.c_double), ("dt", C.c_double), ("robot_r", C.c_double),
        ("max_speed", C.c_double), ("a", C.c_double * 3), ("w", C.c_double * 3), ("sonar_range", C.c_double),
        ("sonar_angle", C.c_double), ("num_cores", C.c_int32), ("num_obs", C.c_int32),
        ("reset_start_and_goal", C.c_int32), ("random_reset_state", C.c_int32), ("set_boundary", C.c_int32),
        ("max_episode_steps", C.c_int32), ("N", C.c_int32), ("num_beams", C.c_int32), ("precision", C.c_int32),
        ("step_lanes", C.c_int32), ("rollout_lanes", C.c_int32),
    ]


class MnDqnLearner(C.Structure):
    """mn_dqn_learner: the device pointers of one DQN learner of a group (mn_dqn_group_create)."""
    _fields_ = [(n, C.c_void_p) for n in ("ring_states", "ring_next_states", "ring_actions", "ring_rewards", "ring_dones", "rng_state", "params_local",
                                          "params_target", "grad", "exp_avg", "exp_avg_sq", "step")]


DQN_MAX_LEARNERS = 64      # MN_DQN_MAX_LEARNERS


class MnRenderStyle(C.Structure):
    """mn_render_style: how mn_render_worlds colours a world (include/marinenav_hip.h); colours are r << 16 | g << 8 | b."""
    _fields_ = [("v_max", C.c_double), ("hpx", C.c_double), ("marker_r", C.c_double), ("n_levels", C.c_int32), ("lic", C.c_int32),
                ("lic_steps", C.c_int32), ("lic_floor", C.c_int32), ("seed", C.c_uint32), ("outside", C.c_uint32), ("obstacle", C.c_uint32),
                ("marker", C.c_uint32), ("max_workgroups", C.c_int32), ("reserved", C.c_int32), ("palette", C.c_uint32 * 32)]


class MnRenderPrim(C.Structure):
    """mn_render_prim: one primitive of mn_render_draw, 48 bytes."""
    _fields_ = [("x0", C.c_double), ("y0", C.c_double), ("x1", C.c_double), ("y1", C.c_double), ("image_first", C.c_int32), ("image_last", C.c_int32),
                ("color_z", C.c_uint32), ("kind", C.c_uint16), ("half_width_px", C.c_uint16)]


class MnIqnLearner(C.Structure):
    """mn_iqn_learner: the device pointers of one IQN learner of a group (mn_iqn_group_create)."""
    _fields_ = [(n, C.c_void_p) for n in ("ring_states", "ring_next_states", "ring_actions", "ring_rewards", "ring_dones", "rng_state", "params_local",
                                          "params_target", "workspace", "grad", "loss", "exp_avg", "exp_avg_sq", "step", "idx_out", "taus_out")]


IQN_MAX_LEARNERS = 64      # MN_IQN_MAX_LEARNERS


class MnIqnActor(C.Structure):
    """mn_iqn_actor: the handles and device pointers of one IQN actor of a group (mn_iqn_actor_group_create); `weights` is a HOST array of 14 device pointers."""
    _fields_ = [(n, C.c_void_p) for n in ("ctx", "weights", "rng_state", "draws", "ring_states", "ring_next_states", "ring_actions", "ring_rewards", "ring_dones")]


IQN_MAX_ACTORS = 64      # MN_IQN_MAX_ACTORS


class MnDqnActor(C.Structure):
    """mn_dqn_actor: the device pointers of one DQN actor of a group (mn_dqn_actor_group_create); `weights` is a HOST array of 18 device pointers."""
    _fields_ = [("weights", C.c_void_p), ("image", C.c_void_p), ("seed", C.c_uint64)] + [(n, C.c_void_p) for n in (
        "ring_states", "ring_next_states", "ring_actions", "ring_rewards", "ring_dones")]


DQN_MAX_ACTORS = 64      # MN_DQN_MAX_ACTORS

PER_MASS_ONE, PER_BLOCK, PER_MAX_CAPACITY, PER_MAX_BATCH = 1 << 16, 1024, 1 << 20, 1024      # MN_PER_* (mn_per_append / _sample / _update)
NSTEP_MAX, NSTEP_REFERENCE, NSTEP_EPISODE = 16, 0, 1      # MN_NSTEP_MAX, MN_NSTEP_REFERENCE, MN_NSTEP_EPISODE (mn_replay_append_nstep)


class MnNstepGamma(C.Structure):
    """mn_nstep_gamma: float32(gamma ** a) for a = 0 .. MN_NSTEP_MAX - 1, passed to mn_replay_append_nstep by value."""
    _fields_ = [("g", C.c_float * NSTEP_MAX)]


class MarineNavHipError(RuntimeError):
    pass


def build(force=False):
    """Compile libmarinenav_hip.so for gfx950 with hipcc (cross-compiles without a GPU)."""
    csrc = os.path.join(_HERE, "csrc")
    cmd = ["make", "-C", csrc] + (["-B"] if force else [])
    subprocess.check_call(cmd, stdout=subprocess.DEVNULL)
    return LIB_PATH


_lib = None

# (name, restype, argtypes) for every symbol include/marinenav_hip.h declares
_vp, _i32, _i64, _dbl = C.c_void_p, C.c_int32, C.c_int64, C.c_double
_pd, _pi32, _pi64, _pu8, _pu32, _pf = (C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_int64),
                                         C.c_void_p, C.POINTER(C.c_uint32), C.c_void_p)
SIGNATURES = [
    ("mn_default_params", C.c_int, [C.POINTER(MnParams)]),
    ("mn_create", C.c_int, [_i32, C.POINTER(MnParams), C.POINTER(_vp)]),
    ("mn_destroy", C.c_int, [_vp]),
    ("mn_last_error", C.c_char_p, [_vp]),
    ("mn_num_envs", _i32, [_vp]),
    ("mn_set_params", C.c_int, [_vp, C.POINTER(MnParams)]),
    ("mn_get_params", C.c_int, [_vp, C.POINTER(MnParams)]),
    ("mn_seed", C.c_int, [_vp, _pu32, _vp]),
    ("mn_set_schedule", C.c_int, [_vp, _i32, _pi64, _pi32, _pi32, _pd, _dbl]),
    ("mn_set_start_goal", C.c_int, [_vp, _i32, _pd, _pd]),
    ("mn_reset", C.c_int, [_vp, _pu8, _pf, _vp]),
    ("mn_step", C.c_int, [_vp, _vp, _pf, _pf, _pu8, _pu8, _vp]),
    ("mn_step_append", C.c_int, [_vp, _vp, _pf, _pf, _pf, _pu8, _pu8, _pf, _pf, _vp, _pf, _pf, _i64, _i64, _vp]),
    ("mn_build_info", _i32, []),
    ("mn_rollout", C.c_int, [_vp, _i32, _vp, C.c_uint64, C.c_uint64, C.c_uint64, _pf, _pf, _pf, _pu8, _pu8, _vp, _vp]),
    ("mn_random_actions", C.c_int, [C.c_uint64, C.c_uint64, C.c_uint64, _i32, _vp, _vp]),
    ("mn_reset_done", C.c_int, [_vp, _pf, _vp]),
    ("mn_reset_done_async", C.c_int, [_vp, _pf, _vp, C.POINTER(_vp), C.POINTER(C.c_uint32)]),
    ("mn_reset_placement", _i32, [C.c_float, _i32, _i64, _i32, _i32, _i32]),
    ("mn_reset_done_next_act", C.c_int, [_vp, _pf, _vp, C.c_float, _i32, _i32, C.POINTER(_vp), C.POINTER(C.c_uint32), _pi32]),
    ("mn_set_reset_owed_max_rows", C.c_int, [_vp, _i32]),
    ("mn_reset_is_owed", _i32, [_vp]),
    ("mn_reset_join", C.c_int, [_vp, _vp]),
    ("mn_set_reset_under_act_max", C.c_int, [_vp, _i32, C.POINTER(C.c_int64)]),
    ("mn_debug_side_delay_us", C.c_int, [_vp, _i32]),
    ("mn_debug_read", C.c_int, [_vp, _i32, _vp, _i64]),
    ("mn_load_worlds", C.c_int, [_vp, _i32, _i32, _pi32, _pd, _pi32, _pd, _pi32, _pd, _pd, _pd, _pd, _pd, _pd, _pf, _vp]),
    ("mn_get_worlds", C.c_int, [_vp, _i32, _i32, _pi32, _pd, _pi32, _pd, _pi32, _pd, _pd, _pd, _pd, _pd, _pd]),
    ("mn_query_velocity", C.c_int, [_vp, _vp, _i32, _vp, _i64, _vp, _vp]),
    ("mn_query_observation", C.c_int, [_vp, _vp, _i32, _vp, _i32, _i64, _vp, _vp, _vp, _vp]),
    ("mn_query_rollout", C.c_int, [_vp, _vp, _i32, _vp, _vp, _i32, _vp, _i32, _vp, _i64] + [_vp] * 14),
    ("mn_render_worlds", C.c_int, [_vp, _vp, _i32, _i32, _i32, _i32, _pd, C.POINTER(MnRenderStyle), _vp, _vp]),
    ("mn_render_draw", C.c_int, [_vp, _i32, _i32, _i32, _pd, _vp, _i64, _vp]),
    ("mn_render_font", C.c_int, [_vp]),
    ("mn_time_field_workspace_bytes", _i64, [_i32, _i32, _i64]),
    ("mn_time_field", C.c_int, [_vp, _vp, _i32, _vp, _i64, _i32, _i32, C.c_double, C.c_double, _i32, _vp, _vp, _vp, _vp, _vp, _vp]),
    ("mn_pilot_act", C.c_int, [_vp, _vp, _i32, _vp, _vp, _vp, _vp, _i64, _i32, _i32, _i32, _i64, _vp, _vp, _vp, _vp, _vp, _vp]),
    ("mn_rollout_pilot", C.c_int, [_vp, _i32, _vp, _vp, _i64, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    ("mn_get_state", C.c_int, [_vp, _i32, _i32, _pd, _pi32, _pi64]),
    ("mn_set_state", C.c_int, [_vp, _i32, _i32, _pd, _pi32, _pi64]),
    ("mn_state_bytes", _i64, [_vp]),
    ("mn_state_save", C.c_int, [_vp, _vp, _i64, _vp]),
    ("mn_state_load", C.c_int, [_vp, _vp, _i64, _vp]),
    ("mn_enable_obs64", C.c_int, [_vp, _i32]),
    ("mn_get_obs64", C.c_int, [_vp, _i32, _i32, _pd]),
    ("mn_get_reward64", C.c_int, [_vp, _i32, _i32, _pd]),
    ("mn_enable_trajectory", C.c_int, [_vp, _i32]),
    ("mn_get_trajectory", C.c_int, [_vp, _i32, _i32, _i32, _pd]),
    ("mn_set_trajectory_trace", C.c_int, [_vp, _vp, _i32, _i32]),
    ("mn_obs_perturb", C.c_int, [_vp, _vp, _i64, C.c_uint64, _vp, _vp, _vp]),      # spec: POINTER(obs_noise.MnObsNoise), passed with byref
    ("mn_set_obs_noise", C.c_int, [_vp, _vp, C.c_uint64]),
    ("mn_env_perturb_obs", C.c_int, [_vp, _vp, _vp, _vp]),
    ("mn_peek_next_double", C.c_int, [_vp, _i32, _i32, _pd]),
    ("mn_last_done_count", C.c_int, [_vp, _vp, _pi32]),
    ("mn_profile_begin", C.c_int, [_vp, _i32]),
    ("mn_profile_end", C.c_int, [_vp, _vp, _pd, _pi32]),
    ("mn_profile_reset_end", C.c_int, [_vp, _vp, _pd, _pi32]),
    ("mn_iqn_create", C.c_int, [C.POINTER(_vp)]),
    ("mn_iqn_destroy", C.c_int, [_vp]),
    ("mn_iqn_weights_changed", C.c_int, [_vp]),
    ("mn_iqn_set_variant", C.c_int, [_vp, _i32]),
    ("mn_iqn_set_greedy_rows", C.c_int, [_vp, _i32]),
    ("mn_iqn_set_few_rows_max", C.c_int, [_vp, _i32]),
    ("mn_iqn_few_rows_launches", C.c_int, [_vp, C.POINTER(C.c_int64)]),
    ("mn_iqn_set_grid", C.c_int, [_vp, _i32]),
    ("mn_iqn_set_tau_mode", C.c_int, [_vp, _i32]),
    ("mn_iqn_set_late_rows", C.c_int, [_vp, _vp, _vp, C.c_uint32, _i32]),
    ("mn_iqn_late_timeouts", C.c_int, [_vp, _vp, C.POINTER(C.c_uint32)]),
    ("mn_iqn_late_timeouts_peek", C.c_int, [_vp, C.POINTER(C.c_uint32)]),
    ("mn_iqn_set_late_bound_ms", C.c_int, [_vp, C.c_double]),
    ("mn_iqn_train_workspace_init", C.c_int, [_vp, _i32, _vp]),
    ("mn_iqn_train_step", C.c_int, [_vp, _vp, _vp, _vp, _vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _i32, C.c_float, _i32,
                                    _dbl, _dbl, _dbl, _dbl, _dbl, _vp]),
    ("mn_rollout_policy", C.c_int, [_vp, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    ("mn_planner_act", C.c_int, [_vp, _i32, _i32, _pd, _pd, _vp, _vp]),
    ("mn_rollout_iqn", C.c_int, [_vp, _vp, C.POINTER(C.c_void_p), _i32, _vp, C.c_float, _i32] + [_vp] * 10),
    ("mn_rollout_iqn_rows", C.c_int, [_vp, _vp, C.POINTER(C.c_void_p), _i32, _vp, C.c_float, _i32] + [_vp] * 12),
    ("mn_rollout_iqn_eval", C.c_int, [_vp, _vp, C.POINTER(C.c_void_p), _i32, _vp, C.c_float, _i32] + [_vp] * 14),
    ("mn_iqn_image_floats", _i32, []),
    ("mn_iqn_export_image", C.c_int, [_vp, C.POINTER(C.c_void_p), _vp, _vp]),
    ("mn_rollout_iqn_groups", C.c_int, [_vp, _vp, _i64, _i32, _i32, _i32] + [_vp] * 14),
    ("mn_rollout_dqn", C.c_int, [_vp, C.POINTER(C.c_void_p), _vp, _i32, _i32] + [_vp] * 8),
    ("mn_dqn_image_floats", C.c_int64, []),
    ("mn_dqn_export_image", C.c_int, [C.POINTER(C.c_void_p), _vp, _vp]),
    ("mn_rollout_dqn_groups", C.c_int, [_vp, _vp, _i64, _i32, _i32, _i32] + [_vp] * 8),
    ("mn_dqn_act", C.c_int, [_vp, C.POINTER(C.c_void_p), _vp, _i32, _vp, _vp, _i32, _vp]),
    ("mn_dqn_train_workspace_floats", C.c_int64, [_i32]),
    ("mn_dqn_train_step", C.c_int, [_vp] * 5 + [_i64] + [_vp] * 11 + [_i32, C.c_float] + [_dbl] * 5 + [_vp]),
    ("mn_dqn_train_steps_workspace_floats", C.c_int64, [_i32, _i32]),
    ("mn_dqn_train_steps", C.c_int, [_vp] * 5 + [_i64] + [_vp] * 11 + [_i32, _i32, C.c_float] + [_dbl] * 5 + [_vp]),
    ("mn_dqn_train_steps_parts", C.c_int, [_vp] * 5 + [_i64] + [_vp] * 11 + [_i32, _i32, C.c_float] + [_dbl] * 5 + [_i32, _vp]),
    ("mn_dqn_group_create", C.c_int, [C.POINTER(MnDqnLearner), _i32, C.POINTER(_vp)]),
    ("mn_dqn_group_destroy", C.c_int, [_vp]),
    ("mn_dqn_group_train_step", C.c_int, [_vp, _i64, _vp, _vp, _vp, _vp, _i32, C.c_float] + [_dbl] * 5 + [_vp]),
    ("mn_dqn_group_train_steps", C.c_int, [_vp, _i64, _vp, _vp, _vp, _vp, _i32, _i32, C.c_float] + [_dbl] * 5 + [_vp]),
    ("mn_iqn_group_create", C.c_int, [C.POINTER(MnIqnLearner), _i32, _i32, C.POINTER(_vp)]),
    ("mn_iqn_group_destroy", C.c_int, [_vp]),
    ("mn_iqn_group_train_step", C.c_int, [_vp, _i64, _vp, _vp, _vp, C.c_float] + [_dbl] * 5 + [_vp]),
    ("mn_iqn_actor_group_create", C.c_int, [C.POINTER(MnIqnActor), _i32, _i32, C.POINTER(_vp)]),
    ("mn_iqn_actor_group_destroy", C.c_int, [_vp]),
    ("mn_iqn_actor_group_act", C.c_int, [_vp, _vp, C.c_float, C.c_float, _vp, _vp]),
    ("mn_iqn_actor_group_append", C.c_int, [_vp] * 6 + [_i64, _i64, _vp]),
    ("mn_dqn_act_rng", C.c_int, [_vp, C.POINTER(C.c_void_p), _vp, _i32, C.c_uint64, C.c_uint64, C.c_float, _vp, _vp, _vp, _i32, _vp]),
    ("mn_dqn_actor_group_create", C.c_int, [C.POINTER(MnDqnActor), _i32, _i32, C.POINTER(_vp)]),
    ("mn_dqn_actor_group_destroy", C.c_int, [_vp]),
    ("mn_dqn_actor_group_set_grid", C.c_int, [_vp, _i32]),
    ("mn_dqn_actor_group_act", C.c_int, [_vp, _vp, C.c_float, C.c_uint64, C.POINTER(C.c_uint64), _vp, _vp]),
    ("mn_dqn_actor_group_append", C.c_int, [_vp] * 6 + [_i64, _i64, _vp]),
    ("mn_xchg_create", C.c_int, [_i32, _i32, C.POINTER(_vp)]),
    ("mn_xchg_export", C.c_int, [_vp, _vp]),
    ("mn_xchg_import", C.c_int, [_vp, _i32, _vp]),
    ("mn_xchg_attach", C.c_int, [_vp, _vp, _i32, _vp]),
    ("mn_iqn_train_exchange", C.c_int, [_vp, _vp, _vp, _i32, C.c_float, _vp]),
    ("mn_xchg_memory_kind", C.c_int, [_vp]),
    ("mn_xchg_set_timeout_ms", C.c_int, [_vp, _i64]),
    ("mn_iqn_train_plan", C.c_int, [_i32, _i32, _i32]),
    ("mn_iqn_train_set_cu_limit", C.c_int, [_i32]),
    ("mn_iqn_train_workspace_status_word", C.c_int64, [_i32]),
    ("mn_iqn_train_step_xchg", C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _i32, C.c_float,
                                         _i32, _dbl, _dbl, _dbl, _dbl, _dbl, C.c_float, _vp]),
    ("mn_xchg_status", C.c_int, [_vp, _pi32]),
    ("mn_xchg_last_error", C.c_char_p, [_vp]),
    ("mn_xchg_destroy", C.c_int, [_vp]),
    ("mn_probe_mfma_clock", C.c_int, [C.c_double, _pd, _vp]),
    ("mn_iqn_refresh", C.c_int, [_vp, C.POINTER(C.c_void_p), _vp]),
    ("mn_iqn_act", C.c_int, [_vp, _vp, _vp, C.POINTER(C.c_void_p), _vp, _vp, C.c_float, _vp, _vp, _i32, _i32, _vp]),
    ("mn_iqn_act_rng", C.c_int, [_vp, _vp, C.POINTER(C.c_void_p), _vp, _vp, _vp, C.c_float, C.c_float, _vp, _vp, _vp, _i32, _i32, _vp]),
    ("mn_iqn_last_greedy_rows", C.c_int, [_vp, _vp, _pi32, _i32, _pi32]),
    ("mn_iqn_act_rng_env", C.c_int, [_vp, _vp, _vp, C.POINTER(C.c_void_p), _vp, _vp, _vp, C.c_float, C.c_float, _vp, _vp, _vp, _i32, _i32, _vp]),
    ("mn_replay_append", C.c_int, [_vp] * 10 + [_i64, _i64, _i64, _vp]),
    ("mn_replay_append_nstep", C.c_int, [_vp] * 10 + [_i64, _i32, MnNstepGamma, _i32] + [_vp] * 5 + [_i64, _i64, _i64, _vp]),
    ("mn_episode_log", C.c_int, [_vp, _vp, _vp, _i32, _dbl, _i64, C.c_float] + [_vp] * 9 + [_i64, _vp, _vp]),
    ("mn_iqn_train_workspace_floats", C.c_int64, [_i32]),
    ("mn_iqn_train_workspace_misplaced_word", C.c_int64, [_i32]),
    ("mn_iqn_sample", C.c_int, [_i64, _i32, _vp, _vp, _vp, _i32, _vp]),
    ("mn_iqn_train_grad", C.c_int, [_vp] * 13 + [_i32, _i32, C.c_float, _vp]),
    ("mn_iqn_train_grad_per", C.c_int, [_vp] * 13 + [_i32, _i32, C.c_float, _vp, _vp, _vp]),
    ("mn_iqn_train_grad_munch", C.c_int, [_vp] * 14 + [_i32, _i32, C.c_float, C.c_float, C.c_float, C.c_float, _vp, _vp]),
    ("mn_iqn_train_grad_rule", C.c_int, [_vp] * 14 + [_i32, _i32, C.c_float, _i32, _vp, _vp, _vp]),
    ("mn_per_append", C.c_int, [_vp, _vp, _vp, _i64, _i64, _i64, _vp]),
    ("mn_per_sample", C.c_int, [_vp, _vp, _i64, _i64, _i32, C.c_float] + [_vp] * 5),
    ("mn_per_update", C.c_int, [_vp] * 5 + [_i32, C.c_float, C.c_float, _i64, _vp]),
    ("mn_iqn_train_grad_sampled", C.c_int, [_vp] * 5 + [_i64] + [_vp] * 8 + [_i32, _i32, C.c_float, _i32, _vp]),
    ("mn_iqn_train_adam", C.c_int, [_vp] * 6 + [_i32] + [C.c_double] * 5 + [C.c_float, _i32, _vp]),
    ("mn_iqn_train_set_mode", C.c_int, [_i32]),
    ("mn_iqn_profile_begin", C.c_int, [_vp, _i32]),
    ("mn_iqn_profile_end", C.c_int, [_vp, _vp, _pd, _pi32]),
]


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise MarineNavHipError(
                f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(hipcc --offload-arch=gfx950).  There is no CPU fallback.")
        L = C.CDLL(LIB_PATH)
        for name, res, args in SIGNATURES:
            fn = getattr(L, name)      # AttributeError if the header and the library disagree
            fn.restype, fn.argtypes = res, args
        if L.mn_build_info() != 0:
            raise MarineNavHipError(f"{LIB_PATH} is an ablation build (mn_build_info() != 0); the package only runs the full kernels")
        _lib = L
    return _lib


def default_params():
    p = MnParams()
    rc = lib().mn_default_params(C.byref(p))
    if rc:
        raise MarineNavHipError("mn_default_params failed")
    return p


def check(rc, handle=None):
    if rc != 0:
        msg = lib().mn_last_error(handle)
        raise MarineNavHipError(f"libmarinenav_hip error {rc}: {msg.decode() if msg else ''}")


def stream_ptr(device):
    """The calling thread's current HIP stream on `device` as a ctypes pointer -- what every per-step entry point takes.  torch.cuda.current_stream() builds a Stream
    object per call (~4 us, five times per vector step); the raw accessor returns the handle itself."""
    import torch
    idx = device.index if device.index is not None else torch.cuda.current_device()
    try:
        return C.c_void_p(torch._C._cuda_getCurrentRawStream(idx))
    except AttributeError:      # (another torch build)
        return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)

