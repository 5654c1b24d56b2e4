/*
 * marinenav_hip.h -- C-ABI of libmarinenav_hip.so, the MI355X (gfx950) batched marinenav_env.
 *
 * The reference (RobustFieldAutonomyLab/Distributional_RL_Navigation) is pure Python and has no
 * FFI layer; its boundary for this path is the Python class MarineNavEnv
 * (marinenav_env/envs/marinenav_env.py:25-627).  Each entry point below names the reference
 * method(s) it replaces for a batch of `n_envs` independent environments.  A reference
 * maintainer binds these with ctypes; the package's own binding is
 * distributional_rl_navigation_amd/_capi.py.
 *
 * Conventions
 *  - Every function returns 0 on success or a negative mn_status; mn_last_error() gives text.
 *    No C++ exceptions cross the boundary.
 *  - `*_dev` pointers are DEVICE pointers owned by the caller (e.g. torch.Tensor.data_ptr());
 *    `*_host` pointers are host memory.  The library never frees caller memory and never
 *    allocates in mn_step / mn_reset_done / mn_reset.
 *  - Environment state (robot pose, world tables, MT19937 streams) lives in device memory
 *    owned by the handle (allocated in mn_create, released in mn_destroy).
 *  - `stream` is a hipStream_t passed as void* (NULL = default stream).  Kernels are launched
 *    on it with no implicit synchronisation; host<->device accessors (get / set / load) are
 *    synchronous with respect to that handle's previous work on the NULL stream only, so call
 *    them after synchronising your stream.
 *  - One handle per GPU per process; a handle is not re-entrant across threads.
 *    A handle is bound to the HIP device that was current at mn_create(); entry points called while another
 *    device is current return MN_ERR_INVALID (mn_destroy switches to the owning device itself).
 */
#ifndef MARINENAV_HIP_H
#define MARINENAV_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MN_MAX_CORES 8      /* curriculum maximum, train_IQN_model.py:86-90 */
#define MN_MAX_OBS 10       /* curriculum maximum, train_IQN_model.py:86-90 */
#define MN_NUM_BEAMS 11     /* robot.py:9 */
#define MN_OBS_DIM 26       /* 2 + 2 + 2*11, marinenav_env.py:80-81 */
#define MN_NUM_ACTIONS 9    /* robot.py:55-56 */
#define MN_MAX_STAGES 8     /* curriculum stages held on device */

typedef enum mn_status {
    MN_OK = 0,
    MN_ERR_INVALID = -1,   /* bad argument */
    MN_ERR_HIP = -2,       /* a HIP runtime call failed (text in mn_last_error) */
    MN_ERR_NO_DEVICE = -3, /* no gfx950 device visible */
    MN_ERR_ALLOC = -4,
    MN_ERR_PEER = -5       /* mn_xchg_export / mn_xchg_import: the runtime refused to export this rank's mailbox or to map a peer's (no IPC between the processes --
                              HSA_ENABLE_IPC_MODE_LEGACY=0 missing? -- or no peer access between the devices); text in mn_xchg_last_error */
} mn_status;

/* info codes written by mn_step; strings at marinenav_env.py:243,246,250,254,257 */
enum { MN_INFO_NORMAL = 0, MN_INFO_OUT_OF_BOUNDARY = 1, MN_INFO_TOO_LONG = 2, MN_INFO_COLLISION = 3, MN_INFO_REACH_GOAL = 4 };

/* arithmetic of the step/observation kernels */
enum {
    MN_PRECISION_F64 = 0,   /* everything float64: whole-episode parity with the reference */
    MN_PRECISION_MIXED = 1  /* f64 pose integration + f64->f32 relative geometry, f32 field/sonar:
                               single-step outputs within 1e-5 of the reference */
};

/* Scalar attributes of MarineNavEnv.__init__ (marinenav_env.py:40-73), Robot.__init__
 * (robot.py:25-50) and Sonar.__init__ (robot.py:5-12).  Uniform over the batch. */
typedef struct mn_params {
    double width, height;            /* :40-41 */
    double core_r;                   /* :42 self.r */
    double v_rel_max, p;             /* :43-44 */
    double v_range[2];               /* :45 */
    double obs_r_range[2];           /* :46 */
    double clear_r;                  /* :47 */
    double goal_dis;                 /* :54 */
    double timestep_penalty;         /* :55 */
    double collision_penalty;        /* :59 */
    double goal_reward;              /* :60 */
    double discount;                 /* :61 (host-side only) */
    double min_start_goal_dis;       /* :64 */
    double init_theta, init_speed;   /* :51-52, used when random_reset_state == 0 */
    double dt;                       /* robot.py:28 */
    double robot_r;                  /* robot.py:33 */
    double max_speed;                /* robot.py:34 */
    double a[3], w[3];               /* robot.py:35-36 */
    double sonar_range, sonar_angle; /* robot.py:7-8 */
    int32_t num_cores, num_obs;      /* :62-63, requested world size when no schedule is set */
    int32_t reset_start_and_goal;    /* :48 */
    int32_t random_reset_state;      /* :50 */
    int32_t set_boundary;            /* :73 */
    int32_t max_episode_steps;       /* 1000, :244 */
    int32_t N;                       /* robot.py:29 sub-steps per action */
    int32_t num_beams;               /* robot.py:9, must equal MN_NUM_BEAMS */
    int32_t precision;               /* MN_PRECISION_* */
    int32_t step_lanes;              /* lanes per env in the step kernel: 0 = auto (up to 128 K envs 2, or 4 in mn_step_append; else 1), or 1, 2, 4, 8.
                                        Results do not depend on it (fixed summation tree): a performance knob only */
    int32_t rollout_lanes;           /* the same for mn_rollout: 0 = auto (16 up to 4 096 envs, 8 up to 16 K, 4 up to 64 K, else 2), or 2, 4, 8, 16 */
} mn_params;

typedef struct mn_handle mn_handle;

/* Build flags of the loaded library.  The shipped libmarinenav_hip.so returns 0: its kernels have no switch that
 * removes work.  libmarinenav_hip_ablation.so (make ablation; profiling scripts only) returns MN_BUILD_ABLATION. */
#define MN_BUILD_ABLATION 1
int32_t mn_build_info(void);

/* Fills *p with the reference defaults (marinenav_env.py:40-73, robot.py:5-50). */
int mn_default_params(mn_params *p);

/* MarineNavEnv.__init__ for n_envs environments (marinenav_env.py:27-73).  RNG streams are
 * seeded with seed 0..n_envs-1 until mn_seed is called. */
int mn_create(int32_t n_envs, const mn_params *p, mn_handle **out);
int mn_destroy(mn_handle *h);
const char *mn_last_error(const mn_handle *h); /* h may be NULL for create-time errors */
int32_t mn_num_envs(const mn_handle *h);

/* Attribute writes such as `env.num_cores = 4`, `env.set_boundary = True`, `env.robot.N = 5`
 * (train_IQN_model.py:131-140, run_experiments.py:197-207). */
int mn_set_params(mn_handle *h, const mn_params *p);
int mn_get_params(const mn_handle *h, mn_params *p);

/* MarineNavEnv.seed (marinenav_env.py:75-78): env i <- np.random.RandomState(seeds_host[i])
 * (MT19937, legacy init_genrand seeding). */
int mn_seed(mn_handle *h, const uint32_t *seeds_host, void *stream);

/* Curriculum `schedule` constructor argument (marinenav_env.py:27,89-98;
 * train_IQN_model.py:86-90).  n_stages == 0 clears it.  The stage is looked up with
 * floor(total_timesteps[i] * timestep_scale): scale 1 reproduces the reference for one env,
 * scale n_envs makes the curriculum advance with aggregate experience. */
int mn_set_schedule(mn_handle *h, int32_t n_stages, const int64_t *timesteps, const int32_t *num_cores,
                    const int32_t *num_obstacles, const double *min_start_goal_dis, double timestep_scale);

/* env.start / env.goal attribute writes (train_IQN_model.py:133-134); env_idx < 0 = all envs. */
int mn_set_start_goal(mn_handle *h, int32_t env_idx, const double start[2], const double goal[2]);

/* MarineNavEnv.reset (marinenav_env.py:86-186) for the envs with mask_dev[i] != 0 (NULL = all):
 * curriculum lookup, start/goal, vortex cores, obstacles by bounded rejection sampling from the
 * env's own MT19937 stream (bit-exact draw order), robot pose, first observation.
 * Writes obs rows [i][26] (float32) of the reset envs into obs_dev (other rows untouched). */
int mn_reset(mn_handle *h, const uint8_t *mask_dev, float *obs_dev, void *stream);

/* MarineNavEnv.step (marinenav_env.py:199-262) for all envs: N sub-steps of
 * get_velocity (:422-465) + Robot.update_state (robot.py:102-123), get_observation (:273-326,
 * robot.py:125-198), reward and termination ladder (:220-257), counters (:259-260).
 * actions_dev[n] int32 in [0,9); obs_dev [n][26] f32 (terminal observation for finished envs);
 * reward_dev [n] f32; done_dev [n] u8; info_dev [n] u8 (MN_INFO_*).  No auto-reset. */
int mn_step(mn_handle *h, const int32_t *actions_dev, float *obs_dev, float *reward_dev, uint8_t *done_dev,
            uint8_t *info_dev, void *stream);

/* mn_step plus ReplayBuffer.add (thirdparty/IQN/replay_buffer.py:26-34, as called at agent.py:124) for every env, in
 * the SAME launch: the transition (prev_obs_dev[i] = the observation actions_dev[i] was chosen from, action, reward,
 * obs_dev[i] = terminal observation for finished envs, done) of env i goes to ring slot (ptr + i - first) mod capacity,
 * first = max(0, n_envs - capacity) (deque(maxlen): only the newest `capacity` rows survive; envs below `first` are
 * not stored).  Ring layout as mn_replay_append.  prev_obs_dev and obs_dev must be different buffers.  The caller
 * advances ptr by min(n_envs, capacity). */
int mn_step_append(mn_handle *h, const int32_t *actions_dev, const float *prev_obs_dev, float *obs_dev, float *reward_dev,
                   uint8_t *done_dev, uint8_t *info_dev, float *ring_states, float *ring_next_states,
                   int64_t *ring_actions, float *ring_rewards, float *ring_dones, int64_t ptr, int64_t capacity,
                   void *stream);

/* T = n_steps consecutive vector steps in ONE launch -- the loop `for t: a = policy(); env.step(a); if done: env.reset()`
 * (agent.py:113-170 without the learner) for every env, for policies that do not look at the observation: the uniform
 * random policy of BASELINE configs[1] (actions_dev == NULL: env i takes, at step t, the action
 * mn_random_actions(action_seed, first_step_index + t, first_env_index + i) -- a counter-based draw, uniform over the 9
 * actions) or a pre-drawn action tensor actions_dev [n_steps][n_envs] i32.  Environment state stays in registers
 * between steps and an env that finishes is reset at once by its own wavefront (same world generation, same RNG stream
 * positions as mn_reset_done), so the result is BIT-IDENTICAL to n_steps x (mn_step, mn_reset_done) with the same
 * actions.  Outputs (device pointers; every trace may be NULL):
 *   obs_dev          [n][26] f32       : what obs_dev holds after the last (mn_step, mn_reset_done) pair -- the observation
 *                                        each env continues from (first observation of the new episode where it just finished)
 *   obs_trace_dev    [n_steps][n][26]  : the observation each step returned (terminal observation for a finished env)
 *   reward_trace_dev [n_steps][n] f32, done_trace_dev / info_trace_dev [n_steps][n] u8, action_trace_dev [n_steps][n] i32
 * first_env_index = this handle's offset in a sharded run (rank * n_envs), so shards draw the actions of their slice.
 * Afterwards nothing is pending for mn_reset_done and mn_last_done_count reports 0.  (Envs a preceding mn_step flagged
 * done are NOT reset by this call: finish the mn_step / mn_reset_done pair before switching to mn_rollout.) */
int mn_rollout(mn_handle *h, int32_t n_steps, const int32_t *actions_dev, uint64_t action_seed, uint64_t first_step_index,
               uint64_t first_env_index, float *obs_dev, float *obs_trace_dev, float *reward_trace_dev,
               uint8_t *done_trace_dev, uint8_t *info_trace_dev, int32_t *action_trace_dev, void *stream);
/* EPISODES under an observation-reading policy in ONE launch (the classical baselines of run_experiments.py:100-190,
 * 213-282).  policy = MN_POLICY_APF (APF_agent.act, APF.py:17-78) or MN_POLICY_BA (BA_agent.act, BA.py:14-155), evaluated on the device on
 * the float32 observation row each step produces (tables a / w = the handle's robot parameters).  Every env runs its CURRENT episode --
 * starting from the observation in obs_dev -- for up to n_steps steps; an env that finishes is NOT reset: it idles, its traces read
 * reward 0 / done 1 / its terminal info code / action -1 from then on, obs_dev keeps its terminal observation.  Step for step
 * bit-identical to a loop of (mn_planner_act, mn_step).  Traces as mn_rollout ([n_steps][n] ...; any may be NULL). */
#define MN_POLICY_APF 1
#define MN_POLICY_BA 2
int mn_rollout_policy(mn_handle *h, int32_t n_steps, int32_t policy, float *obs_dev, float *obs_trace_dev, float *reward_trace_dev,
                      uint8_t *done_trace_dev, uint8_t *info_trace_dev, int32_t *action_trace_dev, void *stream);
/* One policy step of the same device functions for n observation rows [n][26] f32 -> actions [n] i32; a[3], w[3]: HOST arrays, the
 * robot's acceleration / angular-velocity tables (robot.py:35-36).  MN_ERR_INVALID, without a launch: a NULL argument, n <= 0, an unknown
 * policy, an obs_dev that is not 8-byte aligned (the rows are loaded as float2) or an actions_dev that is not 4-byte aligned. */
int mn_planner_act(const float *obs_dev, int32_t n, int32_t policy, const double *a, const double *w, int32_t *actions_dev, void *stream);
/* The action draws of mn_rollout for one step: actions_dev[i] = action of env (first_env_index + i) at step step_index. */
int mn_random_actions(uint64_t action_seed, uint64_t step_index, uint64_t first_env_index, int32_t n, int32_t *actions_dev,
                      void *stream);

/* The caller-side `if done: state = train_env.reset()` (thirdparty/IQN/agent.py:152-170), batched:
 * resets exactly the envs the LAST mn_step flagged done and overwrites their rows of obs_dev
 * (which may or may not be the buffer given to mn_step). */
int mn_reset_done(mn_handle *h, float *obs_dev, void *stream);
/* The same reset OFF the caller's critical path: launched on a stream the handle owns (behind an event recorded on `stream`), so it runs
 * under whatever the caller enqueues on `stream` next.  In the training loop that is the act kernel of the next vector step
 * (agent.py:113-124: `state = next_state` / `env.reset()` then `act(state)`), which depends on the reset only through the rows of the
 * finished envs: tell it which they are and how to recognise a finished row -- mn_iqn_set_late_rows(ctx, <the step's done_dev>, *ready_out,
 * *tick_out, n) -- and it takes those rows last, each after `(*ready_out)[e] == *tick_out` (written by the reset wavefront behind its
 * write-through row).  Results are those of mn_reset_done, bit for bit.  `stream` is joined again (everything enqueued later waits for the
 * reset launch to end) by mn_reset_join or by the next mn_step / mn_step_append / mn_reset_done[_async] on it; every other entry point of
 * the handle waits for it on the host.  Between this call and the join the caller must not read obs_dev rows of finished envs except
 * through such an act launch.
 * Beside the act kernel's workgroups a CU has room for FOUR reset wavefronts (one per SIMD: 96 registers each; the kernel that runs there reads the env's
 * MT19937 row in place instead of copying it into LDS), which run several times slower there: that hides the resets of a few thousand episodes per vector
 * step (alone, such a launch is a latency chain that leaves most of the chip idle; measured cross-over 6 000 - 7 800 steadily arriving per 65 536-env step, depending on the box),
 * not a burst of tens of thousands.  The call therefore launches under the act kernel only while the decaying peak of the episodes started per reset
 * launch -- peak <- max(count, 7/8 peak), kept by the launches themselves and read by the host from a mapped word without synchronising -- is at most
 * `under_act_max` (mn_set_reset_under_act_max: default MN_RESET_UNDER_ACT_MAX_DEFAULT; 0x7fffffff always, -1 never); otherwise it is mn_reset_done on
 * `stream` and *ready_out is NULL (no late rows).  mn_set_reset_under_act_max also reports that peak as of the last launch seen (-1: none yet).
 * mn_debug_side_delay_us (test hook): a kernel that sleeps `us` microseconds in front of every such launch on the handle's stream, i.e. a reset
 * launch that does not run beside the act kernel -- what the callers' fallback (late-row timeouts -> resets in front) is tested with. */
#define MN_RESET_UNDER_ACT_MAX_DEFAULT 5000
int mn_reset_done_async(mn_handle *h, float *obs_dev, void *stream, const uint32_t **ready_out, uint32_t *tick_out);
int mn_reset_join(mn_handle *h, void *stream);
int mn_set_reset_under_act_max(mn_handle *h, int32_t under_act_max, int64_t *last_seen);
int mn_debug_side_delay_us(mn_handle *h, int32_t us);
/* Test hook: the first `bytes` bytes of a raw device array of the handle, padding included (rows are padded to a multiple of 256 envs): MN_DEBUG_MT the
 * MT19937 rows [npad][624] u32, MN_DEBUG_MT_POS their positions [npad] i32, MN_DEBUG_QCX .. MN_DEBUG_QOR the compact tables of the mixed-precision step
 * kernel ([8][npad] cores: x, y as i32 fixed point, signed Gamma f32; [10][npad] obstacles: x, y, radius).  Waits for the device. */
#define MN_DEBUG_MT 0
#define MN_DEBUG_MT_POS 1
#define MN_DEBUG_QCX 2
#define MN_DEBUG_QCY 3
#define MN_DEBUG_QCG 4
#define MN_DEBUG_QOX 5
#define MN_DEBUG_QOY 6
#define MN_DEBUG_QOR 7
#define MN_DEBUG_N_FIELDS 8
int mn_debug_read(mn_handle *h, int32_t field, void *out, int64_t bytes);

/* mn_reset_done_async for a caller that knows its next act call: `eps` and `n_rows` of that call (eps < 0: unknown) and whether its own check of the
 * under-act arrangement has failed (`fallback` != 0: never under the act kernel).  *placement_out says where the reset of the last step's finished envs runs:
 *   MN_RESET_IN_FRONT  launched here on `stream` (mn_reset_done);
 *   MN_RESET_UNDER_ACT launched here on the handle's own stream, *ready_out / *tick_out as mn_reset_done_async;
 *   MN_RESET_OWED      NOTHING is launched: the handle records that those envs await their reset, and the caller's next act call, made through
 *                      mn_iqn_act_rng_env with this handle, runs the resets INSIDE its preparation launch -- reset wavefronts first in the grid, the call's
 *                      draws (and the pack of a stale weight image) beside them -- and its act kernel without late rows: no second stream, no events.
 *                      Every other entry point that reads or writes the handle's state settles the debt first with a plain reset launch (on its stream; the
 *                      entry points that synchronise with the host wait for it), so the results are those of MN_RESET_IN_FRONT whatever the caller does next.
 * mn_reset_placement is the rule, a pure function of (eps, n_rows, peak = the decaying episode peak or -1, under_act_max, owed_max_rows, fallback):
 *   under_act_max == 0x7fffffff (forced: the callers' preflight)      -> UNDER_ACT
 *   owed_max_rows < 0 (mn_set_reset_owed_max_rows; off)                -> as mn_reset_done_async
 *   fallback, under_act_max < 0, peak unknown or above under_act_max   -> OWED (where mn_reset_done_async would go in front)
 *   else: the act launch evaluates about (1 - eps) n_rows rows; at most owed_max_rows of them -- too short a launch to pay for two cross-stream
 *   events -- -> OWED, more (or eps unknown) -> UNDER_ACT.
 * MN_RESET_OWED_MAX_ROWS_DEFAULT = 500 rows: at 65 536 envs and ~300 episode ends per step the owed arm wins by 9.4 us per vector step at ~430 rows; at 3 277
 * rows (eps 0.95) only by 1.6 us, which is inside the run-to-run spread sessions on this hardware have seen (up to 2.3 us), and it loses 6.6 us at 13 107
 * (eps 0.8), where the act kernel is long enough to hide a reset launch beside it (profiles/reset_in_prep.txt).  Nothing was measured between 430 and 3 277
 * rows, nor with thousands of episode ends per step, so the default stays just above the last point that is clearly won. */
#define MN_RESET_IN_FRONT 0
#define MN_RESET_UNDER_ACT 1
#define MN_RESET_OWED 2
#ifndef MN_RESET_OWED_MAX_ROWS_DEFAULT
#define MN_RESET_OWED_MAX_ROWS_DEFAULT 500
#endif
int32_t mn_reset_placement(float eps, int32_t n_rows, int64_t peak, int32_t under_act_max, int32_t owed_max_rows, int32_t fallback);
int mn_reset_done_next_act(mn_handle *h, float *obs_dev, void *stream, float eps, int32_t n_rows, int32_t fallback, const uint32_t **ready_out,
                           uint32_t *tick_out, int32_t *placement_out);
int mn_set_reset_owed_max_rows(mn_handle *h, int32_t owed_max_rows);
/* 1 while a reset is owed (mn_reset_done_next_act chose MN_RESET_OWED and nothing has settled it yet), else 0 */
int32_t mn_reset_is_owed(const mn_handle *h);

/* MarineNavEnv.reset_with_eval_config (marinenav_env.py:467-555), world + pose fields, for `count`
 * consecutive envs starting at first_env.  Host arrays, row-major:
 *   n_cores[count], cores_xy[count][MN_MAX_CORES][2], clockwise[count][MN_MAX_CORES],
 *   gamma[count][MN_MAX_CORES], n_obs[count], obs_xy[count][MN_MAX_OBS][2], obs_r[count][MN_MAX_OBS],
 *   start[count][2], goal[count][2], init_theta[count], init_speed[count].
 * Does not touch the RNG streams.  Resets episode_timesteps, places the robot at `start` and
 * writes the first observation rows into obs_dev if it is not NULL. */
int mn_load_worlds(mn_handle *h, int32_t first_env, int32_t count, const int32_t *n_cores, const double *cores_xy,
                   const int32_t *clockwise, const double *gamma, const int32_t *n_obs, const double *obs_xy,
                   const double *obs_r, const double *start, const double *goal, const double *init_theta,
                   const double *init_speed, float *obs_dev, void *stream);

/* MarineNavEnv.episode_data (marinenav_env.py:557-622), world + pose fields; same layouts. */
int mn_get_worlds(mn_handle *h, int32_t first_env, int32_t count, int32_t *n_cores, double *cores_xy,
                  int32_t *clockwise, double *gamma, int32_t *n_obs, double *obs_xy, double *obs_r, double *start,
                  double *goal, double *init_theta, double *init_speed);

/* Queries: ask a world without stepping it.  Both read only the handle's float64 master tables (cores, obstacles, goal, the
 * placed counts) and the parameters -- tables a handle of either precision keeps -- compute in float64 throughout, and write
 * NOTHING into the handle: robot state, counters, RNG rows, observation / trajectory buffers and the done queue stay as they are.
 * The answers therefore do not depend on the handle's precision.  Query q is evaluated in world env_of_query_dev[q] ([n_queries]
 * i32 on the device), or every query in world env0 if env_of_query_dev is NULL.  n_queries = 0 returns MN_OK without a launch.
 * MN_ERR_INVALID (with a message in mn_last_error): NULL handle, n_queries < 0, env0 outside [0, n_envs) when no index array is
 * given, an unknown velocity_mode, and with n_queries > 0 a NULL input or every output NULL.  An index outside [0, n_envs) INSIDE env_of_query_dev is
 * not visible to the host: that query reads no table, its float outputs are NaN and its flags are MN_QUERY_FLAG_BAD_ENV alone
 * (mn_query_velocity has no flags: NaN only); the other queries of the call are unaffected and the call returns MN_OK.
 * Both calls join a pending mn_reset_done_async on `stream`.
 *
 * mn_query_velocity: MarineNavEnv.get_velocity(x, y) (marinenav_env.py:422-455), the current at xy_dev [n_queries][2] f64, into
 *   v_dev [n_queries][2] f64.
 * mn_query_observation: get_observation() (marinenav_env.py:273-326 with robot.py:125-198) of a robot in state
 *   state_dev [n_queries][6] f64 = x, y, theta, speed, velocity_x, velocity_y (the columns of mn_get_state).
 *   MN_QUERY_VELOCITY_GIVEN takes columns 4-5 as the robot's velocity (a state after a step); MN_QUERY_VELOCITY_FROM_CURRENT
 *   ignores them and uses speed (cos theta, sin theta) + current(x, y), as Robot.reset_state does (robot.py:79-87: a robot
 *   placed at a pose).  Outputs, each may be NULL: obs_dev [n_queries][26] f32 (the float32 cast of the float64 row; 8-byte aligned),
 *   obs64_dev [n_queries][26] f64, flags_dev [n_queries] u8.  The flag bits are independent of each other (they are not the
 *   termination ladder of mn_step): COLLISION by the reference's rule -- only the obstacle with the nearest centre is tested,
 *   d <= r + robot_r (marinenav_env.py:329-336) --, OUTSIDE [0, width] x [0, height], GOAL within goal_dis of the goal. */
enum { MN_QUERY_VELOCITY_GIVEN = 0, MN_QUERY_VELOCITY_FROM_CURRENT = 1 };
enum { MN_QUERY_FLAG_COLLISION = 1, MN_QUERY_FLAG_OUTSIDE = 2, MN_QUERY_FLAG_GOAL = 4, MN_QUERY_FLAG_BAD_ENV = 128 };
int mn_query_velocity(mn_handle *h, const int32_t *env_of_query_dev, int32_t env0, const double *xy_dev,
                      int64_t n_queries, double *v_dev, void *stream);
int mn_query_observation(mn_handle *h, const int32_t *env_of_query_dev, int32_t env0, const double *state_dev,
                         int32_t velocity_mode, int64_t n_queries, float *obs_dev, double *obs64_dev,
                         uint8_t *flags_dev, void *stream);

/* What-if steps and open-loop rollouts: MarineNavEnv.step (marinenav_env.py:199-262 with robot.py:102-123) of a robot placed by hand, n_steps
 * times, under actions the caller names -- env_visualizer.one_step / visualize_control(action_sequence), a stored episode of
 * *_evaluations.npz, the nine-action fan of a pose.  A query like the two above: it reads the float64 master tables only, computes in
 * float64 in the reference's own order of operations whatever the handle's precision, writes NOTHING into the handle, draws no random
 * number and runs no policy; world selection (env_of_query_dev / env0), n_queries = 0 and the joined mn_reset_done_async are as above.
 * n_steps = 1 is the what-if step.
 *   state_dev [n_queries][6] f64 = x, y, theta, speed, velocity_x, velocity_y: the start of query q.  A step ignores columns 4-5 (it
 *     overwrites the velocity before it reads it); a query that runs no step reports them as they are.
 *   episode_timesteps_dev [n_queries] i32: the counter before the first step (NULL = 0); step t of a query sees it + t.
 *   actions_dev (i32), by action_mode: MN_QUERY_ACTIONS_SHARED [n_steps], one sequence for every query; MN_QUERY_ACTIONS_CONSTANT
 *     [n_queries], query q holds actions_dev[q] for all its steps; MN_QUERY_ACTIONS_PER_QUERY [n_queries][n_steps].
 *   n_steps_of_query_dev [n_queries] i32 (NULL = n_steps): query q runs min(max(it, 0), n_steps) steps, fewer if a step ends its
 *     episode (done).  0 <= n_steps <= MN_QUERY_MAX_STEPS.
 * Outputs per query, each may be NULL: state_out_dev [n_queries][6] f64 (columns 4-5: the velocity the last sub-step moved with),
 * obs_dev [n_queries][26] f32 (8-byte aligned) / obs64_dev f64: the observation of that state, reward_dev [n_queries] f64: the last
 * step's reward (0 if no step ran), done_dev / info_dev [n_queries] u8 (MN_INFO_*), steps_dev [n_queries] i32: steps run.
 * Traces, each may be NULL, [n_steps][n_queries] as the episode launches lay theirs out: reward_trace_dev f64, done_trace_dev u8,
 * info_trace_dev u8, action_trace_dev i32, state_trace_dev [n_steps][n_queries][6] f64 (the state after the step),
 * traj_trace_dev [n_steps][n_queries][N][2] f64 (the position after each sub-step, marinenav_env.py:211-212).  Every row is written:
 * behind a query's last step reward 0, done 1, its last info code, action -1, its last state, NaN positions.  Rewards are not
 * discounted.
 * Not visible to the host, and confined to their own query (the call returns MN_OK): an index outside [0, n_envs) inside
 * env_of_query_dev -- no table is read, no step runs (steps 0), float outputs NaN, done 1, info MN_QUERY_FLAG_BAD_ENV; a state about to
 * be stepped with a non-finite x, y, theta or speed or |theta| >= 1e6 (the reference wraps the heading in a loop), or an action outside
 * [0, 9) -- that step counts as run, float outputs NaN, done 1, info MN_QUERY_INFO_BAD_STATE.
 * MN_ERR_INVALID: as above, an unknown action_mode, n_steps outside [0, MN_QUERY_MAX_STEPS], n_steps > 0 with actions_dev NULL. */
enum { MN_QUERY_ACTIONS_SHARED = 0, MN_QUERY_ACTIONS_CONSTANT = 1, MN_QUERY_ACTIONS_PER_QUERY = 2 };
enum { MN_QUERY_INFO_BAD_STATE = 64 };
#define MN_QUERY_MAX_STEPS 65536
int mn_query_rollout(mn_handle *h, const int32_t *env_of_query_dev, int32_t env0, const double *state_dev,
                     const int32_t *episode_timesteps_dev, int32_t action_mode, const int32_t *actions_dev, int32_t n_steps,
                     const int32_t *n_steps_of_query_dev, int64_t n_queries, double *state_out_dev, float *obs_dev,
                     double *obs64_dev, double *reward_dev, uint8_t *done_dev, uint8_t *info_dev, int32_t *steps_dev,
                     double *reward_trace_dev, uint8_t *done_trace_dev, uint8_t *info_trace_dev, int32_t *action_trace_dev,
                     double *state_trace_dev, double *traj_trace_dev, void *stream);

/* Pictures on the device: flow images of worlds the handle holds, and primitives (trails, discs, rings) drawn over them.  The rules below are
 * csrc/mn_render_body.h's, a __host__ __device__ body on top of the query body: every operation is an IEEE float64 add, multiply, divide, square
 * root, floor or comparison, or integer arithmetic (no trigonometric function, contraction off), so host and device give the same pixel words.
 *
 * Pixel word and view.  A pixel is a uint32 z << 24 | r << 16 | g << 8 | b; z is the draw order, the larger z wins, and every write that may be
 * contested is an integer atomic max on the word: the result does not depend on the order of arrival.  view = {x0, y0, x1, y1} in world units over
 * an image of width x height pixels ([n_images][height][width] words), sx = (x1 - x0) / width, sy = (y1 - y0) / height; the centre of pixel (row r,
 * column c) is x = x0 + (c + 0.5) sx, y = y1 - (r + 0.5) sy: row 0 is the top.
 *
 * mn_render_worlds: image i shows world env_of_image_dev[i] ([n_images] i32 on the device), or every image world env0 if that is NULL.  It reads only
 * the float64 master tables (cores, obstacles, start, goal, the placed counts) and the parameters, like the queries, computes in float64 whatever the
 * handle's precision and writes NOTHING into the handle.  The launch owns every pixel: whole words, plain stores.  Per pixel, by the pixel's centre:
 *   field (z = 0): outside [0, width] x [0, height] of the params: style.outside.  Otherwise (vx, vy) = get_velocity at the centre (the arithmetic of
 *     mn_query_velocity), speed = sqrt(vx vx + vy vy), t = speed / v_max * n_levels, level = n_levels - 1 if t is not finite or t >= n_levels, else
 *     (int)floor(t); the colour is palette[level].
 *   LIC (style.lic != 0): noise of pixel (c, r): h = c * 0x9E3779B1 ^ r * 0x85EBCA77 ^ seed * 0xC2B2AE3D (uint32); h ^= h >> 15; h *= 0x2C1B3C6D;
 *     h ^= h >> 12; h *= 0x297A2D39; h ^= h >> 15; noise = h >> 24.  The streamline starts at the centre in continuous pixel coordinates
 *     (u, v) = (c + 0.5, r + 0.5); the first sample is the pixel's own noise; then up to lic_steps Euler steps with sign s = +1 and, from the centre
 *     again, up to lic_steps with s = -1.  A step: the velocity at the world point (x0 + u sx, y1 - v sy); stop this direction if the speed is not a
 *     finite number above zero; u = u + s (hpx vx / speed), v = v - s (hpx vy / speed); stop if floor(u) is outside [0, width) or floor(v) outside
 *     [0, height), else add the noise of pixel (floor(u), floor(v)).  g = (2 sum + count) / (2 count) in integers over the count samples taken; each
 *     colour channel c becomes c * (lic_floor + (255 - lic_floor) * g / 255) / 255, in integers, in this order.
 *   obstacles (z = 1): obstacle k covers a centre with dx dx + dy dy <= r r (dx = x - ox): style.obstacle.
 *   markers (z = 2, style.marker_r > 0): the start is the disc of marker_r world units; the goal is that disc plus the ring rin^2 <= d^2 <= goal_dis^2,
 *     rin = goal_dis - max(sx, sy), one pixel wide (rin <= 0: the whole disc of goal_dis): style.marker.
 * A world index outside [0, n_envs) inside env_of_image_dev is not visible to the host: that image is style.outside everywhere, the others are
 * unaffected and the call returns MN_OK.  style.max_workgroups bounds the grid (0: 2048); more tiles than that take the stride loop.
 *
 * mn_render_draw takes no handle.  It draws prims_dev [n_prims] into every image of each record's inclusive range [image_first, image_last], cut to
 * [0, n_images), with atomic max of color_z (the whole word: z << 24 | rgb).  Primitives that share a z have the colours the caller gave them, and
 * max still decides.  half_width_px above MN_RENDER_MAX_HALF_WIDTH counts as that.  A record with a non-finite number where its kind reads one, an
 * empty image range, an out-of-range parameter or an unknown kind draws nothing; nothing a record holds makes the kernel read or write outside the images.
 *   MN_RENDER_SEGMENT: endpoints (x0, y0), (x1, y1) in world units; in pixel units a = ((x0 - view.x0) / sx, (view.y1 - y0) / sy), b alike, d = b - a
 *     (a, b or d not finite: nothing -- a NaN row is how a polyline breaks).  The segment is clipped (Liang-Barsky, t0 = 0, t1 = 1, the edges in the
 *     order u-low, u-high, v-low, v-high: p = -du, du, -dv, dv; q = au - lo, hi - au, ...; p == 0: q < 0 rejects; r = q / p; p < 0: r > t1 rejects,
 *     r > t0 sets t0; p > 0: r < t0 rejects, r < t1 sets t1) to the image rectangle grown by m = half_width_px + 1 on every side, and its new ends
 *     a + t0 d, a + t1 d are clamped into that rectangle, component by component, so a coordinate of 1e300 cannot spin a lane:
 *     n = (int)ceil(max(|du|, |dv|)) of the clipped segment is at most max(width, height) + 2 m.  Samples p_k = a + (d k) / n, k = 0..n (n = 0: a
 *     alone); each stamps the (2 half_width_px + 1)^2 pixels around (floor(p_k.u), floor(p_k.v)) that lie inside the image.
 *   MN_RENDER_DISC: every pixel whose centre has dx dx + dy dy <= x1 x1 around (x0, y0) (x1 < 0: nothing).
 *   MN_RENDER_RING: every pixel whose centre has x1 x1 <= dx dx + dy dy <= y1 y1 (x1 < 0 or y1 < x1: nothing).
 *   MN_RENDER_RECT: the filled axis-aligned rectangle with corners (x0, y0), (x1, y1) in world units, in any order: every pixel whose centre lies in
 *     the closed rectangle [min x, max x] x [min y, max y].  The pixels are looked for in a box cut to the image in float64 before any conversion to
 *     an integer, as for a disc: a corner at 1e300 is fine.
 *   MN_RENDER_MARKER: a pixel-sized mark at the world point (x0, y0).  With a as for a segment, the anchor pixel is (cu, cv) = (floor(a.u),
 *     floor(a.v)); |a.u| or |a.v| above 2^20 (tested in float64; a NaN too): nothing.  half_width_px is the arm h (above MN_RENDER_MAX_HALF_WIDTH
 *     counts as that), x1 the shape: 0 square, 1 plus, 2 cross, any other value nothing; y1 the stroke t = (int)y1 clamped to [0, h] (not finite:
 *     nothing).  Pixel (cu + du, cv + dv) with |du|, |dv| <= h is taken if: square, always; plus, |du| <= t or |dv| <= t; cross,
 *     ||du| - |dv|| <= t.  Cut to the image.
 *   MN_RENDER_GLYPH: one character of the fixed 5 x 7 font (csrc/mn_render_font.h; mn_render_font copies it out), pixel-sized, anchored at the world
 *     point (x0, y0) by the MARKER rules.  (floor(x1), floor(y1)) is the offset in pixels of the cell's top-left pixel (L, T) from the anchor pixel;
 *     each must be finite and within +-2^20, else nothing.  half_width_px = code | scale << 8: code 33..126 (anything else, the space 32 included,
 *     draws nothing), scale 1..8 (anything else: nothing).  Bit (i, j) of the glyph -- column i = 0..4 from the left, row j = 0..6 from the top; bit
 *     4 - i of row byte j of the font -- covers the scale x scale block of columns [L + i scale, L + (i + 1) scale) and rows [T + j scale,
 *     T + (j + 1) scale), cut to the image.
 *   MN_RENDER_SECTOR: a wedge of a disc (the sonar's field of view).  Centre (x0, y0); (x1, y1) is the point of the arc on the sector's middle
 *     direction, m = (x1 - x0, y1 - y0); half_width_px = q gives the cosine of the half angle, c = q / 16384 - 1 (q above 32768: nothing).  A pixel
 *     centre with d = centre - (x0, y0) is inside if d.d <= m.m and (d.d == 0 or d.m >= (c sqrt(d.d)) sqrt(m.m)), in world units, with
 *     d.d = dx dx + dy dy and d.m = dx mx + dy my.  m.m == 0 or not finite (also by overflow): nothing.  The box is the disc's of radius sqrt(m.m).
 *
 * Both calls make ONE launch on `stream`, allocate nothing and never wait on the host.  MN_ERR_INVALID, without a launch: a NULL handle, style,
 * view, pixel or primitive pointer (prims_dev may be NULL when n_prims is 0, which returns MN_OK at once); n_prims < 0; n_images, width or height < 1 or
 * width * height * n_images >= 2^31; a view with x1 <= x0, y1 <= y0 or a non-finite entry; n_levels outside [1, MN_RENDER_MAX_LEVELS]; lic_steps outside
 * [0, MN_RENDER_MAX_LIC_STEPS]; lic_floor outside [0, 255]; v_max <= 0 or NaN; max_workgroups < 0; env0 outside [0, n_envs) without an index array. */
#define MN_RENDER_MAX_LEVELS 32
#define MN_RENDER_MAX_LIC_STEPS 64
#define MN_RENDER_MAX_HALF_WIDTH 8
enum { MN_RENDER_SEGMENT = 0, MN_RENDER_DISC = 1, MN_RENDER_RING = 2, MN_RENDER_RECT = 4, MN_RENDER_MARKER = 5, MN_RENDER_GLYPH = 6,
       MN_RENDER_SECTOR = 7 };      /* 3 is unassigned and draws nothing */
typedef struct mn_render_style {
    double v_max;            /* the speed of the top level */
    double hpx;              /* LIC step in pixels */
    double marker_r;         /* world units; <= 0: no markers */
    int32_t n_levels;        /* 1 .. MN_RENDER_MAX_LEVELS */
    int32_t lic;             /* 0: the plain field colour */
    int32_t lic_steps;       /* 0 .. MN_RENDER_MAX_LIC_STEPS, each way */
    int32_t lic_floor;       /* 0 .. 255: the brightness of noise 0 */
    uint32_t seed;
    uint32_t outside, obstacle, marker;      /* r << 16 | g << 8 | b */
    int32_t max_workgroups;  /* 0: the default grid bound */
    int32_t reserved;
    uint32_t palette[MN_RENDER_MAX_LEVELS];  /* r << 16 | g << 8 | b per level, by value */
} mn_render_style;           /* 192 bytes */
typedef struct mn_render_prim {
    double x0, y0, x1, y1;
    int32_t image_first, image_last;
    uint32_t color_z;
    uint16_t kind, half_width_px;
} mn_render_prim;            /* 48 bytes */
int mn_render_worlds(mn_handle *h, const int32_t *env_of_image_dev, int32_t env0, int32_t n_images, int32_t width, int32_t height,
                     const double view[4], const mn_render_style *style, uint32_t *pixels_dev, void *stream);
int mn_render_draw(uint32_t *pixels_dev, int32_t n_images, int32_t width, int32_t height, const double view[4],
                   const mn_render_prim *prims_dev, int64_t n_prims, void *stream);
/* The font of MN_RENDER_GLYPH into out [95][7] (host memory, 665 bytes): row byte j of code 32 + k at out[7 k + j].  MN_ERR_INVALID: out is NULL. */
int mn_render_font(uint8_t *out);

/* Minimum-time-to-goal fields (Zermelo navigation on a grid): for every cell of an nx x ny grid over a world the handle holds, the least travel time
 * to the goal of a vehicle of constant speed s through the water, carried by the current and kept out of the obstacles, and the first move of a path
 * that attains it.  A query like those above: it reads the float64 master tables only (cores, obstacles, goal, the placed counts) and the parameters,
 * computes in float64 whatever the handle's precision and writes NOTHING into the handle.  The rules are csrc/mn_time_field_body.h's, a
 * __host__ __device__ body on top of the query body: every operation is an IEEE float64 add, multiply, divide, square root or comparison
 * (contraction off), in the order written here, so host and device give the same words.
 *
 * Grid.  1 <= nx, ny and nx * ny <= MN_TIME_FIELD_MAX_CELLS (one workgroup's LDS holds the field).  hx = width / nx, hy = height / ny; cell (i, j),
 *   i = 0..nx-1, j = 0..ny-1, index c = j nx + i, has its centre at x = (i + 0.5) hx, y = (j + 0.5) hy.
 * Current.  c(i, j) = get_velocity at the centre (the arithmetic of mn_query_velocity).  A centre exactly on a core has a NaN current.
 * Free cells.  Cell (i, j) is free iff for EVERY placed obstacle sqrt(dx dx + dy dy) > (r + robot_r) + clearance, dx = ox - x, dy = oy - y.
 * Sources.  A free cell with sqrt(dx dx + dy dy) <= goal_dis, dx = x - gx, dy = y - gy (check_reach_goal); the goal is the world's own or
 *   goal_xy_dev[field].
 * Edges.  16 directions, in this order (the order breaks ties):
 *     k    0  1  2  3    4  5  6  7    8  9 10 11 12 13 14 15
 *     dx   1  0 -1  0    1 -1 -1  1    2  1 -1 -2 -2 -1  1  2
 *     dy   0  1  0 -1    1  1 -1 -1    1  2  2  1 -1 -2 -2 -1
 *   Edge u -> v = u + (dx, dy) exists iff u, v and the two cells the segment crosses are inside the grid and free: a diagonal (dx, dy) crosses
 *   u + (dx, 0) and u + (0, dy); a knight move (2 sx, sy) crosses u + (sx, 0) and u + (sx, sy); a knight move (sx, 2 sy) crosses u + (0, sy) and
 *   u + (sx, sy); an axis move crosses none.
 * Edge time.  s = speed if speed > 0, else the parameters' max_speed.  ex = dx hx, ey = dy hy (dx, dy converted to float64);
 *   L = sqrt(ex ex + ey ey); ux = ex / L, uy = ey / L; cx = (c_u.x + c_v.x) 0.5, cy = (c_u.y + c_v.y) 0.5; a = cx ux + cy uy;
 *   disc = (s s - (cx cx + cy cy)) + a a; g = a + sqrt(disc).  The edge is feasible iff disc >= 0.0 && g > 0.0 (a NaN is infeasible); w = L / g.
 *   An edge that does not exist or is infeasible has w = +inf.
 * Field.  T(u) = 0 for sources, +inf for blocked cells; otherwise T(u) = min over k of (w_k(u) + T(u + off_k)), the float64 sum as written, +inf
 *   where no path exists.  Every w exceeds an ulp of every finite T, so w + T > T strictly and the fixed point is unique: what Dijkstra's algorithm
 *   over the same w with the same float64 w + T settles.  Iteration order, sweep count and work distribution do not show in the result.
 *   dir(u) = the least k that attains the minimum; 255 for sources, blocked cells and cells with T = +inf.
 *
 * mn_time_field: field f is solved in world env_of_field_dev[f] ([n_fields] i32 on the device), or every field in world env0 if that is NULL.
 *   goal_xy_dev [n_fields][2] f64 or NULL (the world's own goal).  Outputs: T_dev [n_fields][ny][nx] f64; dir_dev [n_fields][ny][nx] u8 or NULL;
 *   status_dev [n_fields] i32; sweeps_dev [n_fields] i32 (the relaxation sweeps that ran) or NULL.  Status: MN_TIME_FIELD_OK; _NOT_CONVERGED: the
 *   max_sweeps-th sweep still lowered a cell -- T and dir are then unspecified upper bounds, call again with more; _NO_SOURCE: no free cell within
 *   goal_dis of the goal (T is +inf everywhere, dir 255); _BAD_ENV: the field's world index is outside [0, n_envs), or its goal is not finite: no
 *   table is read, T is NaN, dir 255, sweeps 0, and the other fields are unaffected (the queries' poison rule; the call returns MN_OK).
 *   workspace_dev: mn_time_field_workspace_bytes(nx, ny, n_fields) bytes, 8-byte aligned, contents arbitrary before and after ([n_fields][18][ny nx]
 *   f64: the 16 edge-time planes and the currents); one workspace per concurrently running call.
 * ONE launch on `stream` (one workgroup per field), no allocation, no host synchronisation; a pending mn_reset_done_async is joined on `stream`.
 * n_fields = 0 returns MN_OK without a launch.  MN_ERR_INVALID (message in mn_last_error), without a launch: a NULL handle; n_fields < 0 or >= 2^31;
 * nx or ny < 1 or nx * ny > MN_TIME_FIELD_MAX_CELLS; clearance < 0 or not finite; max_sweeps < 1; env0 outside [0, n_envs) without an index array;
 * and with n_fields > 0 a NULL T_dev, status_dev or workspace_dev.  mn_time_field_workspace_bytes returns MN_ERR_INVALID for a grid outside the
 * limit or n_fields < 0. */
#define MN_TIME_FIELD_MAX_CELLS 16384
#define MN_TIME_FIELD_NO_DIR 255
enum { MN_TIME_FIELD_OK = 0, MN_TIME_FIELD_NOT_CONVERGED = 1, MN_TIME_FIELD_NO_SOURCE = 2, MN_TIME_FIELD_BAD_ENV = 3 };
int64_t mn_time_field_workspace_bytes(int32_t nx, int32_t ny, int64_t n_fields);
int mn_time_field(mn_handle *h, const int32_t *env_of_field_dev, int32_t env0, const double *goal_xy_dev, int64_t n_fields, int32_t nx, int32_t ny,
                  double speed, double clearance, int32_t max_sweeps, double *T_dev, uint8_t *dir_dev, int32_t *status_dev, int32_t *sweeps_dev,
                  void *workspace_dev, void *stream);

/* Field pilot: a pilot with full knowledge of the map that drives the real 9-action robot by looking a few steps ahead with each action and scoring
 * the landing point with the world's minimum-time field T (the global dynamic-window approach).  The upper baseline beside the sonar-only planners,
 * and a per-pose expert action.  The rule is csrc/mn_pilot_body.h's, a __host__ __device__ body on top of the what-if step (mn_query_rollout's
 * arithmetic, csrc/mn_query_step_body.h): float64 whatever the handle's precision, every operation an IEEE float64 add, multiply, divide, floor or
 * comparison in the order written here (contraction off), so host and device give the same words.
 *
 * Inputs.  A world; a robot state [6] (the columns of mn_get_state; the velocity columns are not read) and its episode counter t; a field
 *   T [ny][nx] of that world as mn_time_field writes it (hx = width / nx, hy = height / ny); a horizon H, 1 <= H <= MN_PILOT_MAX_HORIZON.
 * Candidates.  For a = 0..8: copy the state; run the what-if step with action a and the counters t, t + 1, ... up to H times; stop behind the first
 *   step whose info is not MN_INFO_NORMAL.  n_a = the steps run, info_a = the last info, (x_a, y_a) = the end position.  This is mn_query_rollout
 *   with MN_QUERY_ACTIONS_CONSTANT, its rule for a state that leaves the finite numbers on the way included (that step counts, info_a =
 *   MN_QUERY_INFO_BAD_STATE).
 * Score.  step_time = (double)N * dt.  REACH_GOAL: score_a = n_a step_time.  COLLISION, OUT_OF_BOUNDARY (and BAD_STATE): score_a = +inf.
 *   NORMAL, TOO_LONG: score_a = n_a step_time + Tint(x_a, y_a), n_a converted to float64, the product first.
 * Tint(x, y).  +inf unless 0 <= x <= width and 0 <= y <= height.  Tc = T of the containing cell: i = (int)floor(x / hx), j = (int)floor(y / hy),
 *   each clamped to the grid (the far edge belongs to the last cell).  If nx == 1 or ny == 1: Tc.  Otherwise u = x / hx - 0.5, v = y / hy - 0.5;
 *   i0 = (int)floor(u) clamped to [0, nx - 2], j0 = (int)floor(v) clamped to [0, ny - 2]; fx = u - i0 clamped to [0, 1], fy = v - j0 likewise;
 *   T00 = T[j0][i0], T10 = T[j0][i0 + 1], T01 = T[j0 + 1][i0], T11 = T[j0 + 1][i0 + 1].  If all four are finite:
 *   (T00 (1 - fx) + T10 fx) (1 - fy) + (T01 (1 - fx) + T11 fx) fy, in exactly this order; otherwise Tc.  A NaN result counts as +inf.
 * Choice.  The action a with the least key (score_a, H - n_a, a) in lexicographic order: the first minimum wins, and if all nine scores are +inf
 *   the action that survives longest.
 * Poison (the queries' rule: the call returns MN_OK, the trouble stays with its own query).  A world index outside [0, n_envs): flag
 *   MN_QUERY_FLAG_BAD_ENV; a field index outside [0, n_fields): MN_PILOT_FLAG_BAD_FIELD; a state that is not finite or has |theta| >= 1e6:
 *   MN_QUERY_INFO_BAD_STATE; a field whose T[0] is NaN (a MN_TIME_FIELD_BAD_ENV field): MN_PILOT_FLAG_BAD_FIELD -- tested in this order, the first
 *   that holds names the flag.  Such a query gets action -1, NaN scores, 0 steps, its flag in every info and in flags_dev; every other query has
 *   flag 0.
 *
 * mn_pilot_act: a query.  Query q is a robot in state_dev[q] with counter episode_timesteps_dev[q] (NULL: 0) in world env_of_query_dev[q] (NULL:
 *   every query in env0), on field field_of_query_dev[q] (NULL: field 0) of T_dev [n_fields][ny][nx].  Outputs, each NULL or: actions_dev [Q] i32,
 *   scores_dev [Q][9] f64, steps_dev [Q][9] i32 (n_a), infos_dev [Q][9] u8 (info_a), flags_dev [Q] u8.  Nothing in the handle is written; ONE launch
 *   on `stream` (a row of 16 lanes per query), no allocation, no host synchronisation; a pending mn_reset_done_async is joined on `stream`.
 *   n_queries = 0 returns MN_OK without a launch.  MN_ERR_INVALID (message in mn_last_error), without a launch: a NULL handle; n_queries < 0; env0
 *   outside [0, n_envs) without an index array; a NULL state_dev or T_dev; n_fields < 1; a grid outside mn_time_field's; horizon outside
 *   [1, MN_PILOT_MAX_HORIZON]; every output NULL.
 *
 * mn_rollout_pilot: mn_rollout_policy's contract with the pilot as the policy -- every env runs its CURRENT episode for up to n_steps steps, a
 *   finished env idles (reward 0, done 1, its terminal info, action -1), no resets, an attached mn_set_trajectory_trace is honoured -- on
 *   MN_PRECISION_F64 handles only.  Env i follows field field_of_env_dev[i] ([n_envs] i32), or field i if that is NULL (then n_fields must equal
 *   n_envs).  Each step: the nine candidates from the env's own float64 state and counter, the choice, then the real step (mn_step's arithmetic)
 *   -- bit for bit the loop (mn_get_state, mn_pilot_act, mn_step).  A poisoned env (bad field index, BAD_ENV field, a state that is not finite)
 *   ends at once: reward 0, done 1, info MN_QUERY_INFO_BAD_STATE, action -1, and is not stepped.  ONE launch (a row of 16 lanes per env).
 *   MN_ERR_INVALID: a NULL handle, obs_dev or T_dev; n_steps < 1; a mixed-precision handle; the grid, horizon and n_fields errors above. */
#define MN_PILOT_MAX_HORIZON 16
enum { MN_PILOT_FLAG_BAD_FIELD = 32 };
int mn_pilot_act(mn_handle *h, const int32_t *env_of_query_dev, int32_t env0, const double *state_dev, const int32_t *episode_timesteps_dev,
                 const double *T_dev, const int32_t *field_of_query_dev, int64_t n_fields, int32_t nx, int32_t ny, int32_t horizon, int64_t n_queries,
                 int32_t *actions_dev, double *scores_dev, int32_t *steps_dev, uint8_t *infos_dev, uint8_t *flags_dev, void *stream);
int mn_rollout_pilot(mn_handle *h, int32_t n_steps, const double *T_dev, const int32_t *field_of_env_dev, int64_t n_fields, int32_t nx, int32_t ny,
                     int32_t horizon, float *obs_dev, float *obs_trace_dev, float *reward_trace_dev, uint8_t *done_trace_dev,
                     uint8_t *info_trace_dev, int32_t *action_trace_dev, void *stream);

/* Robot pose and counters (robot.py:40-44, marinenav_env.py:70-71).  state[count][6] =
 * x, y, theta, speed, velocity_x, velocity_y (float64).  NULL pointers are skipped. */
int mn_get_state(mn_handle *h, int32_t first_env, int32_t count, double *state, int32_t *episode_timesteps,
                 int64_t *total_timesteps);
int mn_set_state(mn_handle *h, int32_t first_env, int32_t count, const double *state,
                 const int32_t *episode_timesteps, const int64_t *total_timesteps);

/* Snapshot and restore of a whole handle, device to device: mark a point, go on, come back -- or carry the blob to the host and into another
 * process (VecMarineNavEnv.state_dict).  After mn_state_load the handle behaves exactly as the saved one would have: every later mn_step*,
 * mn_reset*, mn_rollout* and accessor gives the same bits.
 *   mn_state_bytes  the size of the handle's blob (a function of n_envs only), or MN_ERR_INVALID for a NULL handle.
 *   mn_state_save   first does what every state-reading entry point does (an owed reset of mn_reset_done_next_act is launched on `stream`, a
 *                   pending mn_reset_done_async joined), then packs the state in ONE launch on `stream` into blob_dev (16-byte aligned, at least
 *                   mn_state_bytes(h) bytes).  Nothing else of the handle is written; no allocation, no host synchronisation.
 *   mn_state_load   reads the blob's header (one small copy, waits for `stream`), validates it, then unpacks in ONE launch on `stream`.
 * The blob is self-describing: a header (magic word, format version, n_envs, precision, byte count, the handle's mn_params and schedule, and the
 * handle's host-side words: done-queue parity, reset tick, the decaying episode peak, the two reset-placement thresholds) followed by, compact
 * over n_envs (not the padded rows of the handle): every env's MT19937 row and position, both halves of the done-queue (counters and lists), pose
 * and velocity, the per-env episode constants (start, goal, init_theta, init_speed), episode / total timesteps, the world sizes, the float64
 * world tables and the compact tables of the mixed-precision step kernel (carried, not re-derived: bit-equal to what the reset kernel wrote).
 * The done-queue's lists are saved in a canonical form (per shard the live entries in ascending order, zeros behind them): the order in which the step
 * kernel's wavefronts appended them is timing, not state, so two handles with the same history give the same blob, byte for byte.
 * NOT state, and not carried: the last-step outputs kept only for parity reads (mn_get_obs64, mn_get_reward64, mn_get_trajectory) and whether
 * they are enabled, an attached trajectory trace, profiling windows, mn_debug_side_delay_us.  The caller's own buffers (observations, rewards,
 * done flags) are the caller's to keep.
 * MN_ERR_INVALID, with a message in mn_last_error and the handle untouched: a NULL or misaligned argument, `bytes` below mn_state_bytes(h), a wrong
 * magic word or version, a blob of another n_envs or precision, or of a handle with other params (step_lanes / rollout_lanes aside: results do not
 * depend on them) or another schedule -- the message names the first field that differs. */
int64_t mn_state_bytes(const mn_handle *h);
int mn_state_save(mn_handle *h, void *blob_dev, int64_t bytes, void *stream);
int mn_state_load(mn_handle *h, const void *blob_dev, int64_t bytes, void *stream);

/* Float64 copy of the last observation each env produced (the reference returns float64,
 * marinenav_env.py:326).  Only kept when precision == MN_PRECISION_F64; out[count][26]. */
/* Float64 copies of the last observation rows / rewards (what the reference's float64 step returns before the agent's .float()),
 * for parity checks and the n = 1 gym-shaped facade.  OFF by default since round 4 -- the training loop does not read them and they
 * were 14 MB of the step kernel's 39 MB of writes per 65 536-env launch: mn_enable_obs64(h, 1) (MN_PRECISION_F64 handles only) makes
 * every later mn_step / mn_step_append / mn_reset* / mn_rollout write them; (h, 0) stops again.  mn_get_obs64 / mn_get_reward64 return
 * MN_ERR_INVALID while disabled.  Enabling does not change any other output (bit-identity tests). */
int mn_enable_obs64(mn_handle *h, int32_t on);
int mn_get_obs64(mn_handle *h, int32_t first_env, int32_t count, double *out);
/* Float64 copy of the last reward (marinenav_env.py:220-255 computes it in float64); same rule. */
int mn_get_reward64(mn_handle *h, int32_t first_env, int32_t count, double *out);

/* robot.trajectory (marinenav_env.py:211-212: one [x, y] per kinematic SUB-step): after mn_enable_trajectory(h, max_N)
 * every mn_step also records the N sub-step positions of each env; mn_get_trajectory copies out[count][n_substeps][2]
 * of the LAST step.  MN_PRECISION_F64 handles only (the facade / evaluation path); off by default. */
int mn_enable_trajectory(mn_handle *h, int32_t max_substeps);
int mn_get_trajectory(mn_handle *h, int32_t first_env, int32_t count, int32_t n_substeps, double *out);
/* The same positions of WHOLE EPISODES: a device trace traj_trace_dev [n_steps][n][n_substeps][2] f64 for the next episode launch of `h` --
 * mn_rollout_policy, mn_rollout_iqn, mn_rollout_iqn_rows, mn_rollout_iqn_eval or mn_rollout_dqn --, which records into row [t][i] the N positions
 * mn_step would record for env i at step t (what mn_get_trajectory returns after that step of the per-step loop, bit for bit) while env i is alive; rows
 * of steps after an env has finished are not written.  A handle-level attachment, like mn_enable_trajectory, and independent of it: the launch that
 * takes it detaches it, whether it succeeds or not -- a call refused for any of its arguments included (only a NULL handle has nothing to detach) --
 * and a launch of more than n_steps steps, or after the robot's N has changed, is refused with MN_ERR_INVALID; mn_rollout records none and refuses to run while one is attached; traj_trace_dev = NULL detaches.  With nothing attached every
 * launch does exactly what it did before, and attaching changes no other output.  n_substeps must be the handle's robot N.  MN_PRECISION_F64 handles
 * only: a mixed-precision handle is refused with MN_ERR_INVALID and a message (mn_last_error).  The buffer must stay valid until the launch has run. */
int mn_set_trajectory_trace(mn_handle *h, double *traj_trace_dev, int32_t n_steps, int32_t n_substeps);

/* ---- Observation noise -------------------------------------------------------------------------
 * What the robot PERCEIVES of an observation row: [0:2] the DVL velocity, [2:4] the goal, [4:26] eleven sonar points, (0, 0) = no return.  The env
 * kernels keep computing the clean row; this rule turns a clean float32 row into the row a policy is fed.  It is a pure function of the clean row
 * and the key (seed, env, ep_t) -- env = the GLOBAL env index (row in the handle + first_env_index, as the seeds follow it), ep_t = the env's
 * episode_timesteps when the observation was made (0 for the reset observation, k for the one the episode's k-th step returned) -- so it does not
 * depend on the launch, the step index inside a launch, the lanes per env, or on whether a loop or an episode kernel applied it; an episode split
 * over two launches perceives what one launch perceives, and traces keep the CLEAN rows: anyone can re-derive what the policy saw.
 *
 * The rule (csrc/mn_obs_noise_body.h is this text as code; tests/obs_noise_twin.py restates it in numpy), uint64 arithmetic modulo 2^64:
 *   mix64         the splitmix64 finaliser of the other draws
 *   base    = mix64(seed + 0x9E3779B97F4A7C15 (env + 1))
 *   row_key = mix64(base ^ (0xC2B2AE3D27D4EB4F (ep_t + 1)))
 *   W(c, w) = mix64(row_key ^ (0x165667B19E3779F9 (2 c + w + 1)))      channel c = 0, 1 velocity | 2, 3 goal | 4 + b beam b;  w = 0 normal word, 1 miss word
 *   z(c)    = float32(s - 131070) * 0x1.bb67aep-16f,  s = the sum of the four 16-bit fields of W(c, 0): an exact integer, one float32 product;
 *             mean 0, variance 1 (the constant is float32(1 / sqrt((2^32 - 1) / 3))), support +-3.464.  No logf, cosf or erff anywhere.
 *   velocity, c = 0, 1:  row[c] = row[c] + vel_sigma  * z(c)            (product rounded, sum rounded; float32 throughout, no contraction)
 *   goal,     c = 2, 3:  row[c] = row[c] + goal_sigma * z(c)
 *   beam b, c = 4 + b, point (x, y) = row[4 + 2 b], row[5 + 2 b]:
 *       x == 0 and y == 0 (no return)                     -> left as it is, sign bits included, whatever the parameters
 *       else (W(c, 1) >> 40) < miss_thr                   -> (+0, +0): the beam reports none.  miss_thr = (uint32)(double(sonar_miss_p) * 2^24), computed
 *                                                            once on the host; p = 0: never (the word is not drawn), p = 1: always
 *       else f = 1 + sonar_rel_sigma * z(c);  x = x * f;  y = y * f      one draw per beam, both coordinates scaled
 * A channel whose parameter is zero is SKIPPED, not multiplied by zero (-0 + 0 is not -0): an all-zero description leaves every bit of the row.
 * sonar_rel_sigma * 3.464 >= 1 lets a point flip through the robot; the rule does not clamp.
 * MN_ERR_INVALID, nothing launched, nothing attached, the message (mn_last_error) naming the parameter: a negative or non-finite sigma, sonar_miss_p
 * outside [0, 1] or NaN.
 *
 *   mn_obs_perturb      rows obs_in_dev [n][26] -> obs_out_dev [n][26] (obs_out_dev == obs_in_dev is allowed; otherwise the two must not overlap) under
 *                       explicit keys: row r is env env_index0 + r at ep_t_dev[r].  One grid-stride launch, no LDS.  The noisy rows of a trace
 *                       [T][n][26] are T calls, each with the counters its step left.
 *   mn_set_obs_noise    attaches a copy of *spec to the handle (NULL detaches) with the handle's first_env_index, the way mn_set_trajectory_trace
 *                       attaches a trace -- but it STAYS attached until it is replaced or detached.  mn_step and every other stepping call keep
 *                       returning clean observations.  While one is attached, mn_rollout_iqn / mn_rollout_iqn_rows, mn_rollout_dqn and
 *                       mn_rollout_policy feed their policy the perceived row (the adaptive CVaR is taken from it too); obs_dev, every trace, obs64, the
 *                       pose, the counters and the act call counter are what they are without noise, given the actions.  An attached all-zero
 *                       description runs the noise-free kernels.  The forms WITHOUT a noisy instantiation -- mn_rollout_iqn_eval, mn_rollout_iqn_groups,
 *                       mn_rollout_dqn_groups, and mn_rollout_policy on a MIXED-precision handle -- return MN_ERR_INVALID and launch nothing while a
 *                       description that is not all-zero is attached (the loop form serves them).
 *                       mn_rollout (random or given actions) and mn_rollout_pilot read no observation and run unchanged.
 *   mn_env_perturb_obs  the loop form, obs -> perturb -> act: mn_obs_perturb of the handle's n rows with the attached description, the handle's own
 *                       episode_timesteps and first_env_index.  Nothing the handle holds is written.  With nothing attached: a copy. */
typedef struct mn_obs_noise {
    uint64_t seed;
    float vel_sigma;          /* m/s, additive, one draw per DVL component */
    float goal_sigma;         /* m, additive, one draw per goal component */
    float sonar_rel_sigma;    /* relative range error, one draw per beam */
    float sonar_miss_p;       /* probability that a beam with a return reports none */
} mn_obs_noise;
int mn_obs_perturb(const float *obs_in_dev, float *obs_out_dev, int64_t n, uint64_t env_index0, const int32_t *ep_t_dev, const mn_obs_noise *spec,
                   void *stream);
int mn_set_obs_noise(mn_handle *h, const mn_obs_noise *spec, uint64_t first_env_index);
int mn_env_perturb_obs(mn_handle *h, const float *obs_in_dev, float *obs_out_dev, void *stream);

/* Next double each env's RandomState would return, without consuming it (test hook pinning the
 * RNG stream position; cf. np.random.RandomState.random_sample). */
int mn_peek_next_double(mn_handle *h, int32_t first_env, int32_t count, double *out);

/* Number of envs the last mn_step flagged done (synchronises the stream). */
int mn_last_done_count(mn_handle *h, void *stream, int32_t *out);

/* Timing hook for benchmarks: records hipEvents on `stream` around the step kernel of the next max_launches mn_step / mn_step_append /
 * mn_rollout calls and around the reset kernel of the next max_launches mn_reset_done calls.  mn_profile_end returns the mean duration of
 * the recorded step launches and closes the window; mn_profile_reset_end (call it first) that of the recorded mn_reset_done launches. */
int mn_profile_begin(mn_handle *h, int32_t max_launches);
int mn_profile_reset_end(mn_handle *h, void *stream, double *mean_ms, int32_t *launches);
int mn_profile_end(mn_handle *h, void *stream, double *mean_ms, int32_t *launches);

/* ---- IQN inference ---------------------------------------------------------------------------
 * Context of one acting agent (the counterpart of holding an `IQNAgent`, thirdparty/IQN/agent.py:10-84): owns the
 * permuted copy of the network weights the act kernel stages into LDS, and the profiling events.  The copy is CACHED:
 * it is rebuilt by the first act call after mn_iqn_create and by the first act call after mn_iqn_weights_changed, which
 * the caller invokes whenever the weights behind the `weights` pointers were written (an optimizer step, a checkpoint
 * load, soft_update into this network).  Calls that share a context must be stream-ordered; different contexts are
 * independent (two agents may act concurrently on two streams of one device).  A context is bound to the HIP device
 * that was current at mn_iqn_create; act calls made while another device is current return MN_ERR_INVALID. */
typedef struct mn_iqn_ctx mn_iqn_ctx;
int mn_iqn_create(mn_iqn_ctx **out);
int mn_iqn_destroy(mn_iqn_ctx *c);
int mn_iqn_weights_changed(mn_iqn_ctx *c);
/* Which acting kernel serves the context's calls (with or without quantile output).
 *   2 (default): the split-f16 kernel -- every float32 operand is split into two f16 pieces (hi = RNE16(x), lo = RNE16(x - hi))
 *      and a product is accumulated as lo.hi + hi.lo + hi.hi on v_mfma_f32_16x16x32_f16 with power-of-two range scaling chosen
 *      from a guaranteed bound, so the result has the error class of float32 arithmetic (measured against a float64
 *      evaluation it is as close as the exact kernel and as eager PyTorch float32) at ~1/3 of the time;
 *   0: the exact-f32 v_mfma_f32_16x16x4_f32 kernel.
 * Same network in both; they differ by float32 rounding only.  Anything else is MN_ERR_INVALID (1 and 3 were the 32x32 re-layouts of the two kernels,
 * measured 2.6 % / 4 % slower on MI355X in rounds 2 / 4 and removed in round 6). */
int mn_iqn_set_variant(mn_iqn_ctx *c, int32_t variant);
/* Whether an act launch that returns nothing but actions evaluates only the rows that do not explore (on != 0: the default).  For an exploring row
 * (u <= eps, agent.py:199-203) the action depends on neither Q nor the observation, so the preparation launch of mn_iqn_act_rng -- which draws every row's
 * exploration uniform -- writes that action itself and lists the other rows, and the act kernel deals the list out evenly over its wavefronts: the launch
 * shrinks with the share of exploring rows (at eps ~ 1 to almost nothing, at eps = 0.05 by 1 row in 32 per wavefront).  Applies to mn_iqn_act_rng with variant 2,
 * per-row taus, actions_dev set, qvals_dev == quantiles_dev == NULL and eps > 0, with or without late rows; an exploring late row is never waited for.  Every
 * other call evaluates every row as before.  Actions, draws and the call counter are bit for bit those of `on` == 0; the list lives in the context
 * (int32 [n], allocated on the first launch of a size; that launch synchronises the device once). */
int mn_iqn_set_greedy_rows(mn_iqn_ctx *c, int32_t on);
/* A SHORT list of greedy rows runs in a kernel of its own (csrc/iqn_act_few.h): workgroups of two wavefronts, one per 16-tau column tile of a row, that read
 * the weight image straight from global memory instead of copying its 154 KB into LDS first.  The launch that would run the listed form without late rows
 * takes it while the list is EXPECTED to hold at most `rows` rows, (1 - eps) n <= rows (the host does not know the count; a longer list is still
 * evaluated correctly, a workgroup loops over its positions).  rows < 0: never; 0x7fffffff: always (tests, A / B measurements).  Actions, draws and the
 * call counter are bit for bit those of the listed form.
 * MN_IQN_FEW_ROWS_MAX_DEFAULT = 256 rows: at 65 536 envs the few-rows kernel wins 7.0 / 6.6 / 6.4 / 6.4 us per vector step at ~20 / 100 / 150 / 200 listed
 * rows, 2.1 us at 300 and 400 (more than those blocks' own spread, less than the 2.3 us sessions on this hardware have differed by), ties at 500 and loses
 * 18 us at 2 000 and 89 us at 8 000 (profiles/act_few_rows.txt).  256 is just above the last length that is clearly won, and the length at which a chip
 * of 256 CUs still gives every listed row a workgroup of its own. */
#ifndef MN_IQN_FEW_ROWS_MAX_DEFAULT
#define MN_IQN_FEW_ROWS_MAX_DEFAULT 256
#endif
int mn_iqn_set_few_rows_max(mn_iqn_ctx *c, int32_t rows);
/* Test hook: the context's act launches that ran as the few-rows kernel so far (host counter; nothing synchronises). */
int mn_iqn_few_rows_launches(mn_iqn_ctx *c, int64_t *out);
/* How an act launch's quantile fractions are drawn (round 4).
 *   0 (default): every observation row gets its own 32 taus -- what a batch of independent calls of the reference's batch-1
 *      IQNAgent.act (agent.py:186-205 -> model.py:149-153) would draw.  mn_iqn_act takes taus [n][32]; mn_iqn_act_rng writes
 *      draws[0 .. 32 n) = taus, draws[32 n .. 33 n) = exploration uniforms.
 *   1: ONE set of 32 taus (x the launch's cvar) for all n rows of the launch.  Every row still sees 32 i.i.d. U(0,1) cvar fractions per
 *      call (the reference's act is batch-1, so independence ACROSS environments is not a reference property), but layer 1 of the
 *      network -- relu(W1 cos(pi k tau) + b1), model.py:141-157,176-178 -- becomes a [32 x 208] constant of the launch that the
 *      preparation launch computes once (exact float32): 216 instead of 372 matrix instructions per row, no per-row cosines.
 *      mn_iqn_act then reads taus [32]; mn_iqn_act_rng writes draws[0 .. 32) = the taus, draws[32 .. 32 + n) = exploration uniforms.
 *      Only with variant 2, without per-row cvar (cvar_row_dev == NULL) and without a selected image slot: else MN_ERR_INVALID.
 *      Two kernel forms serve it: up to 65 535 rows (and for quantile output) one wavefront per row with the taus in the MFMA columns;
 *      from 65 536 rows (every CU of the chip gets a 256-row workgroup) the ENVIRONMENTS are the columns -- T[tau] = W2 diag(h1[tau]) is built once per launch, a wavefront splits the
 *      features of 32 rows once and streams T through LDS: ~260 instead of ~730 vector instructions per row.
 *   2: as 1, but always the wavefront-per-row form; 3: as 1, but always the environment-tiled form (A / B measurements, tests).
 * A row's result for GIVEN taus is the same function in both modes up to float32 rounding (tests). */
int mn_iqn_set_tau_mode(mn_iqn_ctx *c, int32_t mode);
/* Test hook: the rows the context's last act launch with listed rows (mn_iqn_set_greedy_rows) put through the network -- *count_out of them, the first
 * min(count, cap) row indices in list_host (host memory; any order).  Synchronises `stream`; count 0 before the first such launch. */
int mn_iqn_last_greedy_rows(mn_iqn_ctx *c, void *stream, int32_t *list_host, int32_t cap, int32_t *count_out);
/* Late rows of the NEXT act launch of this context (mn_reset_done_async): mask_dev [n] u8 != 0 marks the rows whose observation another
 * stream is still writing, flags_dev [n] / tick say when a row is final (flags_dev[e] == tick; the row itself written through at agent
 * scope before the word).  The launch takes those rows last and reads them past the caches; results equal those of a launch behind the
 * reset.  Returns MN_OK if the next launch of n rows will honour it (launch it next on this context), 1 if the context's current form
 * cannot (the exact-f32 variant, launch-shared taus, quantile capture, more than 64 rows per wavefront): the caller joins the reset
 * (mn_reset_join) instead.  NULL, NULL clears.  mn_iqn_late_timeouts: waits that ran out (0.5 s bound; mn_iqn_set_late_bound_ms, in (0, 60 000] ms,
 * for launches armed afterwards) since the context was made -- anything but 0 means an action was computed on an unfinished row, i.e. the reset
 * launch did not run beside the act kernel on this box: the caller goes back to mn_reset_done (synchronises `stream`).  mn_iqn_late_timeouts_peek:
 * the same count as far as the launches executed so far have reported it through a host-mapped word -- no synchronisation, for a look every few
 * vector steps. */
int mn_iqn_set_late_rows(mn_iqn_ctx *c, const uint8_t *mask_dev, const uint32_t *flags_dev, uint32_t tick, int32_t n);
int mn_iqn_late_timeouts(mn_iqn_ctx *c, void *stream, uint32_t *out);
int mn_iqn_late_timeouts_peek(mn_iqn_ctx *c, uint32_t *out);
int mn_iqn_set_late_bound_ms(mn_iqn_ctx *c, double ms);
/* Measurement aid (bench.py: `gpu_clock_probe`): runs a pure stream of the act kernel's matrix instruction (v_mfma_f32_16x16x32_f16, two
 * waves per SIMD on every CU) for about target_ms milliseconds on `stream` and returns out[0] = elapsed ms (HIP events), out[1] = the clock
 * in GHz the matrix pipe sustained (16 cycles per instruction), out[2] = the clock by the waves' own counters (s_memtime ticks per
 * s_memrealtime tick x 100 MHz), out[3] = sustained f16 TFLOP/s of the chip, out[4] = CUs.  Synchronises the stream.  The boxes of a pool
 * differ in the clock they hold under matrix load; this tells a slow box from a slow kernel. */
int mn_probe_mfma_clock(double target_ms, double *out, void *stream);
/* Grid of the act kernel.  0 (default): at most one PERSISTENT workgroup per CU, each looping over its share of the observations --
 * the weight image is staged into LDS once per CU, the fastest form when nothing else runs.  max_workgroups > 0: up to that many
 * workgroups (more than CUs = several rounds of shorter workgroups, e.g. 2048 for 65 536 observations = 4 per wavefront, ~3 % more
 * time in isolation): CUs are released every few tens of microseconds, so kernels of OTHER streams (the learner's gradient steps,
 * the env kernels of another batch half) are dispatched in between instead of waiting for the whole act launch.  Results do not
 * depend on it. */
int mn_iqn_set_grid(mn_iqn_ctx *c, int32_t max_workgroups);
/* Rebuilds the cached weight image of the selected acting kernel now, on `stream`, if it is stale (what the first act call after
 * mn_iqn_weights_changed would do).  For callers that issue act calls of ONE context on several streams: refresh on one stream,
 * make the others wait for it, and no act call has to write the image. */
int mn_iqn_refresh(mn_iqn_ctx *c, const float *const *weights, void *stream);

/* Fused IQNAgent.act (thirdparty/IQN/agent.py:186-205) for n observations: ObsEncoder.forward with
 * K = 32 quantile samples + mean over them (model.py:141-191), then argmax and the epsilon-greedy choice.
 *   obs_dev   [n][26] f32 : observations (row-major, as mn_step writes them)
 *   taus_dev  [n][32] f32 : quantile fractions, already multiplied by cvar (model.py:149-153)
 *   weights   [14]        : HOST array of DEVICE pointers, nn.Linear layout [out][in], in state-dict order:
 *                           velocity_encoder.weight [16][2], .bias [16], goal_encoder.weight [16][2], .bias [16],
 *                           sensor_encoder.weight [176][22], .bias [176], cos_embedding.weight [208][64], .bias [208],
 *                           hidden_layer.weight [64][208], .bias [64], hidden_layer_2.weight [64][64], .bias [64],
 *                           output_layer.weight [9][64], .bias [9].  Read only when the cached image is stale.
 *   qvals_dev [n][9] f32  : mean over taus of the quantile values (may be NULL)
 *   explore_u_dev [n] f32 : uniform [0,1) draws for exploration (may be NULL = greedy); env i takes the
 *                           greedy action iff u_i > eps (agent.py:200), else action floor(u_i / eps * 9)
 *   actions_dev [n] i32   : chosen actions (may be NULL if only Q-values are wanted)
 *   quantiles_dev [n][32][9] f32 : IQNAgent.act_eval's `quantiles` (agent.py:217-236; model.py:185 before the mean), or
 *                           NULL.  When given, the output layer runs per tau and Q is the mean of these values.
 * Exact float32 MFMA (v_mfma_f32_32x32x2_f32 / v_mfma_f32_16x16x4_f32).  num_taus must be 32. */
int mn_iqn_act(mn_iqn_ctx *c, const float *obs_dev, const float *taus_dev, const float *const *weights, float *qvals_dev,
               const float *explore_u_dev, float eps, int32_t *actions_dev, float *quantiles_dev, int32_t n,
               int32_t num_taus, void *stream);

/* Same act kernel, with the random numbers of the call drawn by the library (no separate generator kernels):
 * draws_dev [33 n] f32 (caller-owned scratch) receives tau[e][j] = U[0,1) * cvar (cvar_row_dev[e] if given, else the
 * scalar `cvar`; model.py:149-153) in its first 32 n entries -- act_eval's `taus` -- and the exploration uniforms of
 * agent.py:199 in the last n; the act kernel then consumes them.  Counter-based generator keyed by
 * rng_state_dev = u64[2] {seed, call counter} on the device; the counter is advanced by the call. */
int mn_iqn_act_rng(mn_iqn_ctx *c, const float *obs_dev, const float *const *weights, uint64_t *rng_state_dev,
                   float *draws_dev, const float *cvar_row_dev, float cvar, float eps, int32_t *actions_dev,
                   float *qvals_dev, float *quantiles_dev, int32_t n, int32_t num_taus, void *stream);
/* mn_iqn_act_rng for the observations of `env`: if the handle owes a reset (mn_reset_done_next_act: MN_RESET_OWED) the call's preparation launch also
 * runs it (mn_prep_reset.hip) -- for the acting form that has such a launch (variant 2, per-row taus); any other form settles the debt with a plain reset
 * launch on `stream` first.  With nothing owed, or env == NULL, exactly mn_iqn_act_rng.  Same actions, draws and call counter either way. */
int mn_iqn_act_rng_env(mn_iqn_ctx *c, mn_handle *env, const float *obs_dev, const float *const *weights, uint64_t *rng_state_dev,
                       float *draws_dev, const float *cvar_row_dev, float cvar, float eps, int32_t *actions_dev,
                       float *qvals_dev, float *quantiles_dev, int32_t n, int32_t num_taus, void *stream);
/* IQN EPISODES in ONE launch: mn_rollout_policy with the learned policy (IQNAgent.evaluation_vec, agent.py:319-398).  Every env of `h` runs its
 * CURRENT episode -- starting from the observation in obs_dev -- for up to n_steps steps; per step it acts exactly as one mn_iqn_act_rng call of
 * context `ctx` on the n current rows at eps = 0 would for its row (taus of call counter rng_state_dev[1] + t, x the scalar `cvar` or, with
 * `adaptive`, x IQNAgent.adjust_cvar_batch of the row; the split-f16 network; argmax, first maximum wins), then steps like mn_step.  An env that
 * finishes is NOT reset: it idles, its traces read reward 0 / done 1 / its terminal info code / action -1 from then on, obs_dev keeps its
 * terminal observation and its terminal pose and counters are stored.  Bit-identical to a loop of (mn_iqn_act_rng, mn_step) run while any env
 * is alive, the act call counter included: afterwards rng_state_dev[1] has grown by steps_run = the longest episode of the launch (at most
 * n_steps), also written to *steps_run_dev (device i32, may be NULL).  The context's weight image is rebuilt first if stale (mn_iqn_refresh).
 * Traces (device, any may be NULL) as mn_rollout_policy ([n_steps][n] ...), plus cvar_trace_dev [n_steps][n] f32 (the cvar each step's taus were
 * drawn with) and q_trace_dev [n_steps][n][9] f32 (Q(s, .) of each step); obs / cvar / Q entries of steps after an env finished are not written.
 * MN_ERR_INVALID for the exact-f32 variant (mn_iqn_set_variant 0), a launch-shared tau mode, n_steps < 1 or a NULL h / ctx / weights /
 * rng_state_dev / obs_dev.  One launch at a time per context (it keeps two device words for the counter update). */
int mn_rollout_iqn(mn_handle *h, mn_iqn_ctx *ctx, const float *const *weights, int32_t n_steps, uint64_t *rng_state_dev, float cvar,
                   int32_t adaptive, float *obs_dev, float *obs_trace_dev, float *reward_trace_dev, uint8_t *done_trace_dev,
                   uint8_t *info_trace_dev, int32_t *action_trace_dev, float *cvar_trace_dev, float *q_trace_dev, int32_t *steps_run_dev,
                   void *stream);
/* The same launch with PER-ENV cvar and adaptive flag (the experiment sweep: adaptive IQN and IQN at cvar 0.25 / 0.5 / 0.75 / 1.0 side by side in one
 * handle, taus keyed by the env index like one mn_iqn_act_rng call with cvar_row_dev on all rows): cvar_row_dev [n] f32 and adaptive_row_dev [n] u8
 * on the device, either may be NULL = the scalar `cvar` / `adaptive` for every env.  Env i acts with adjust_cvar of its row where its flag is set, with
 * cvar_row_dev[i] otherwise.  Refusals, traces, counter update and `one launch at a time per context` as mn_rollout_iqn, which is this call with two
 * NULLs.  No allocation after the context's first rollout, no host synchronisation, caller's stream. */
int mn_rollout_iqn_rows(mn_handle *h, mn_iqn_ctx *ctx, const float *const *weights, int32_t n_steps, uint64_t *rng_state_dev, float cvar,
                        int32_t adaptive, const float *cvar_row_dev, const uint8_t *adaptive_row_dev, float *obs_dev, float *obs_trace_dev,
                        float *reward_trace_dev, uint8_t *done_trace_dev, uint8_t *info_trace_dev, int32_t *action_trace_dev, float *cvar_trace_dev,
                        float *q_trace_dev, int32_t *steps_run_dev, void *stream);
/* mn_rollout_iqn_rows acting as IQNAgent.act_eval does, and recording what each action was chosen from (the experiment sweep's captured episodes,
 * run_experiments.py:26-69): per step each env acts exactly as one mn_iqn_act_rng call WITH quantiles_dev != NULL at eps = 0 would for its row -- the
 * output layer runs per tau on the matrix pipe, Q is the mean of those 32 values, the first maximum wins; mn_rollout_iqn_rows takes the tau mean in
 * front of the output layer, as the call without quantiles_dev does, and the two can differ in the last bit.  Two more traces (device, may be NULL):
 *   quantiles_trace_dev [n_steps][n][32][9] f32 : the quantile values Z(tau, a) of the step (act_eval's `quantiles` of the row)
 *   taus_trace_dev      [n_steps][n][32]    f32 : the taus they belong to (act_eval's `taus`: the call's draws x the row's cvar)
 * whose entries of steps after an env has finished are not written.  q_trace_dev holds the means.  Everything else -- the other traces, the
 * refusals, the counter update, steps_run_dev, `one launch at a time per context` -- as mn_rollout_iqn_rows.  A kernel of its own: its LDS holds the
 * full weight image incl. the output layer's matrix operands (4 KB more than the acting episode kernel's). */
int mn_rollout_iqn_eval(mn_handle *h, mn_iqn_ctx *ctx, const float *const *weights, int32_t n_steps, uint64_t *rng_state_dev, float cvar,
                        int32_t adaptive, const float *cvar_row_dev, const uint8_t *adaptive_row_dev, float *obs_dev, float *obs_trace_dev,
                        float *reward_trace_dev, uint8_t *done_trace_dev, uint8_t *info_trace_dev, int32_t *action_trace_dev, float *cvar_trace_dev,
                        float *q_trace_dev, float *quantiles_trace_dev, float *taus_trace_dev, int32_t *steps_run_dev, void *stream);

/* Size of the acting weight image in 32-bit words: what mn_iqn_export_image writes and one group of mn_rollout_iqn_groups reads. */
int32_t mn_iqn_image_floats(void);
/* Copies the context's acting weight image -- rebuilt first if stale, as mn_iqn_refresh does -- into image_out_dev[mn_iqn_image_floats()] (device,
 * 16-byte aligned), device to device on `stream`: a snapshot of the policy that mn_rollout_iqn_groups can act with later, whatever happens to the
 * weights meanwhile.  MN_ERR_INVALID for the forms mn_rollout_iqn refuses (the exact-f32 variant, a launch-shared tau mode) or a NULL argument. */
int mn_iqn_export_image(mn_iqn_ctx *c, const float *const *weights, uint32_t *image_out_dev, void *stream);
/* IQN episodes of MANY sets of weights in ONE launch: mn_rollout_iqn_rows with a weight image and a tau stream per GROUP of rows.  Row e of `h`
 * belongs to group e / rows_per_group and is row e % rows_per_group of it.  Group g acts with the image at images_dev + g * image_stride (32-bit
 * words; images of mn_iqn_export_image) and with rng_states_dev[g] = {seed, call counter}, its tau draws keyed by the row's index inside the group:
 * the group computes -- traces, final rows and poses, and its counter, which grows by steps_run_dev[g] = the longest episode of the group -- bit for
 * bit what mn_rollout_iqn_rows computes on a handle of rows_per_group rows holding those worlds.  cvar_row_dev / adaptive_row_dev are indexed by e
 * (NULL: cvar 1 / not adaptive).  Episode semantics and traces ([n_steps][n] ..., any may be NULL) as mn_rollout_iqn_rows.
 * group_words_dev [n_groups][2] u32 is the launch's scratch: zeroed ONCE by the caller, left zero by every launch; one launch at a time per
 * buffer.  steps_run_dev [n_groups] i32 may be NULL.  The launch has n workgroups, usually far more than the device runs at once; none waits for
 * another.  No allocation, no host synchronisation, caller's stream.
 * MN_ERR_INVALID, without launching, if n_groups * rows_per_group is not the handle's n_envs, if image_stride is below mn_iqn_image_floats() or no
 * multiple of 4, for a NULL h / images_dev / rng_states_dev / obs_dev / group_words_dev, or n_steps < 1.  It records no sub-step trajectories: an
 * attached trace (mn_set_trajectory_trace) is detached and the call refused. */
int mn_rollout_iqn_groups(mn_handle *h, const uint32_t *images_dev, int64_t image_stride, int32_t n_groups, int32_t rows_per_group, int32_t n_steps,
                          uint64_t *rng_states_dev, const float *cvar_row_dev, const uint8_t *adaptive_row_dev, float *obs_dev, float *obs_trace_dev,
                          float *reward_trace_dev, uint8_t *done_trace_dev, uint8_t *info_trace_dev, int32_t *action_trace_dev, float *cvar_trace_dev,
                          float *q_trace_dev, uint32_t *group_words_dev, int32_t *steps_run_dev, void *stream);

/* ---- replay ring ------------------------------------------------------------------------------
 * ReplayBuffer.add (thirdparty/IQN/replay_buffer.py:26-34) for n transitions in one launch: batch row i
 * goes to ring slot (ptr + i) mod capacity (FIFO eviction like deque(maxlen); if n > capacity only the
 * newest `capacity` rows are written, starting at ptr).  Batch: obs / next_obs [n][26] f32, actions [n]
 * i32, reward [n] f32, done [n] u8.  Ring (device, the layout ReplayBuffer.sample returns): states /
 * next_states [cap][26] f32, actions [cap] i64, rewards / dones [cap] f32.  The caller advances ptr. */
int mn_replay_append(const float *obs_dev, const int32_t *actions_dev, const float *reward_dev, const float *next_obs_dev,
                     const uint8_t *done_dev, float *ring_states, float *ring_next_states, int64_t *ring_actions,
                     float *ring_rewards, float *ring_dones, int64_t n, int64_t ptr, int64_t capacity, void *stream);

/* ---- n-step window ------------------------------------------------------------------------------
 * ReplayBuffer.add with n_step > 1 (thirdparty/IQN/replay_buffer.py:26-41) for k parallel streams in ONE launch: row i of every call
 * is the next transition of stream i.  Each stream keeps its last n = n_step transitions in a caller-owned window (device):
 *     hist_states [n][k][26] f32, hist_actions [n][k] i64, hist_rewards [n][k] f32,
 *     and in MN_NSTEP_EPISODE only: hist_next_states [n][k][26] f32, hist_dones [n][k] u8 (both may be NULL in MN_NSTEP_REFERENCE).
 * `count` is the number of calls the window has taken so far; the caller adds 1 after every call.  The call stores its transition
 * (obs, (i64) action, reward, and in episode mode next_obs and done ? 1 : 0) into window slot count % n.  If count + 1 >= n the
 * window is full and the call emits ONE transition per stream into ring slot (ptr + i - first) mod capacity, first = max(0, k -
 * capacity) (rows below `first` are stored in the window but not emitted: only the newest `capacity` rows of a call survive, as in
 * mn_replay_append); the caller then advances ptr by min(k, capacity).  Earlier calls emit nothing and leave the ring untouched.
 * Slots in AGE order: slot a = 0 .. n-1 is window slot (count + 1 + a) % n; slot n-1 is this call's.  s[a], act[a], r[a], ns[a], d[a]
 * are the slot's state, action, reward, next state and done; those of slot n-1 are this call's inputs.  gamma_pow.g[a] is the caller's
 * float32 table of gamma ** a (Python's double power rounded to float32 once), passed by value.
 *   MN_NSTEP_REFERENCE -- the reference's sliding window, which does not restart at episode ends:
 *     state = s[0], action = act[0]
 *     ret = 0.0f;  for a = 0 .. n-1:  ret = ret + g[a] * r[a]       float32; the product rounds, then the sum (no fused multiply-add);
 *                                                                  the first term is 0.0f + g[0] * r[0] (so -0.0f becomes +0.0f)
 *     next_state = ns[n-1] (this call's next_obs),  done = d[n-1] ? 1.0f : 0.0f
 *   MN_NSTEP_EPISODE -- the window is cut at its first episode end: j = the first a with d[a] set, or n-1 if none is set
 *     state = s[0], action = act[0]
 *     ret = 0.0f;  for a = 0 .. j:    ret = ret + g[a] * r[a]       as above
 *     next_state = ns[j],  done = (any d[a] set) ? 1.0f : 0.0f
 *   Every transition is still the head of exactly one emitted window; the step right behind an episode end heads a clean window,
 *   because the windows in front of it were cut at that end.  The learner's bootstrap discount stays gamma ** n: a cut window has done
 *   = 1, which switches the bootstrap off.
 * The slot a launch writes (count % n) is never the head it reads ((count + 1) % n), and nothing of the newest step is read back from
 * the window.  Two calls on one window must be ordered (one stream).  No allocation, no host synchronisation.
 * MN_ERR_INVALID, without a launch: a NULL among the batch, hist_states / hist_actions / hist_rewards or ring pointers; episode mode
 * without hist_next_states or hist_dones; an unknown mode; n_step outside 2..MN_NSTEP_MAX; count < 0; k <= 0; capacity <= 0; ptr
 * outside [0, capacity). */
#define MN_NSTEP_MAX 16
#define MN_NSTEP_REFERENCE 0
#define MN_NSTEP_EPISODE 1
typedef struct { float g[MN_NSTEP_MAX]; } mn_nstep_gamma;
int mn_replay_append_nstep(const float *obs_dev, const int32_t *actions_dev, const float *reward_dev, const float *next_obs_dev,
                           const uint8_t *done_dev, float *hist_states, int64_t *hist_actions, float *hist_rewards, float *hist_next_states,
                           uint8_t *hist_dones, int64_t count, int32_t n_step, mn_nstep_gamma gamma_pow, int32_t mode, float *ring_states,
                           float *ring_next_states, int64_t *ring_actions, float *ring_rewards, float *ring_dones, int64_t k, int64_t ptr,
                           int64_t capacity, void *stream);

/* ---- Prioritized replay --------------------------------------------------------------------------
 * Proportional prioritized experience replay (Schaul et al. 2016) next to the ring, opt-in.  Priorities are INTEGERS, so every sum is
 * exact and independent of the order in which it was formed; tests/per_twin.py restates all of this in numpy / Python ints.
 * The store (caller-owned, device, all zero at first except mmax):
 *     mass [capacity] u32        row i's mass m_i; MN_PER_MASS_ONE = 1 << 16 is priority 1.0; rows never written have mass 0; 16-byte aligned
 *     block_sums [ceil(capacity / 1024)] u64     bsum[b] = sum of m_i over rows [1024 b, 1024 (b + 1));  total = sum of bsum
 *     mmax [1] u32               the largest mass ever assigned; starts at MN_PER_MASS_ONE
 * capacity <= MN_PER_MAX_CAPACITY = 2^20 rows (<= 1 024 block sums: one scan in one workgroup), batch <= MN_PER_MAX_BATCH = 1 024.
 *
 * mn_per_append -- whenever the ring writes rows [ptr, ptr + n) mod capacity (1 <= n <= capacity; call it in stream order behind the
 *   write, before the caller advances ptr): every such row gets mass *mmax (read on the device) and its block's sum moves by the
 *   integer difference new - old (64-bit atomics, modulo 2^64).
 *
 * mn_per_sample -- `batch` = B slots from rows of positive mass, stratified; needs B <= size <= capacity (every written row has mass
 *   >= 1, so total >= B).  With {seed, ctr} = rng_state_dev (u64[2], the state mn_iqn_sample uses) and
 *   base = mix64(seed + 0x9E3779B97F4A7C15 (ctr + 1)):
 *     q = total / B                                   integer division; the top total - B q < B mass units are never drawn
 *     U_k = mix64(base ^ (0x8CB92BA72F3D8DD7 (k + 1))) >> 40          a 24-bit word; a key of its own, apart from the taus' 0xD1B5...
 *     target_k = k q + mulhi64(U_k << 40, q)          in [k q, (k + 1) q)
 *     idx[k] = the least row i whose inclusive prefix sum m_0 + ... + m_i exceeds target_k      (a zero-mass row is never chosen;
 *                                                      one mass that spans several strata is chosen by all of them: rows repeat)
 *     w_k = powf((float) size * (float) m_idx[k] / (float) total, -beta)       float32, left to right
 *     weights[k] = w_k / max_j w_j                    float32 division
 *   taus_out [2][B][8] f32 are the step's taus exactly as mn_iqn_sample draws them under the same base (target network's first);
 *   idx_out [B] i64, weights_out [B] f32: the layouts mn_iqn_train_grad_per takes.  The call counter advances by one per call.
 *
 * mn_per_update -- after the weighted step: slot k's priority delta_k = absdelta[k] (mn_iqn_train_grad_per) becomes
 *     m = clamp(floorf(powf(delta_k + eps, alpha) * 65536.0f + 0.5f), 1, 2^31 - 1)      float32, product and sum round separately;
 *                                                                                      a NaN gives 1
 *   written to row idx[k]; when several slots name one row the HIGHEST slot wins (one writer per row); block sums move by the integer
 *   difference; *mmax = max(*mmax, m) over the masses written.  A row index outside [0, capacity) is dropped.
 * One launch each, no allocation, no host synchronisation.  MN_ERR_INVALID, without a launch: a NULL pointer, capacity outside
 * 1..2^20, a mass array that is not 16-byte aligned (mn_per_sample), batch outside 1..1024, size outside [batch, capacity], ptr outside [0, capacity), n outside 1..capacity, beta < 0 or NaN. */
#define MN_PER_MASS_ONE 65536u
#define MN_PER_BLOCK 1024
#define MN_PER_MAX_CAPACITY 1048576
#define MN_PER_MAX_BATCH 1024
int mn_per_append(uint32_t *mass, uint64_t *block_sums, const uint32_t *mmax, int64_t ptr, int64_t n, int64_t capacity, void *stream);
int mn_per_sample(const uint32_t *mass, const uint64_t *block_sums, int64_t size, int64_t capacity, int32_t batch, float beta,
                  uint64_t *rng_state_dev, int64_t *idx_out, float *weights_out, float *taus_out, void *stream);
int mn_per_update(uint32_t *mass, uint64_t *block_sums, uint32_t *mmax, const int64_t *idx_dev, const float *absdelta_dev, int32_t batch,
                  float alpha, float eps, int64_t capacity, void *stream);

/* ---- Munchausen target ---------------------------------------------------------------------------
 * The TD target of Munchausen-IQN (Vieillard et al. 2020), opt-in: mn_iqn_train_grad_munch forms y[b, j] by the rule below; loss,
 * backward, reduction, clip and Adam are mn_iqn_train_grad's.  Per batch element b: reward r, done, the action taken a_b, three tau
 * sets tt[b, j], tm[b, j], tl[b, i] (i, j < 8), and with the TARGET weights
 *     Z'[j][a] = Z_target(s'_b, tt[b, j])[a]          the next state, as in mn_iqn_train_grad
 *     Z[j][a]  = Z_target(s_b,  tm[b, j])[a]          one more forward: the target network on the CURRENT state
 * Scalars: alpha >= 0, the entropy temperature te = entropy_tau > 0, the clip bound lo = clip_lo <= 0, gamma (the caller passes
 * gamma ** n_step).  All arithmetic is float32; sums run in index order from the first term; `/ te` is a float32 DIVISION by te (no
 * reciprocal is formed); the two divisions by E are divisions too.  For the next state:
 *     q'[a]   = 0.125f * (Z'[0][a] + Z'[1][a] + ... + Z'[7][a])
 *     d'[a]   = q'[a] - max_a q'
 *     e'[a]   = expf(d'[a] / te)
 *     E'      = e'[0] + e'[1] + ... + e'[8]
 *     tlp'[a] = d'[a] - te * logf(E')
 *     pi'[a]  = e'[a] / E'
 *     V[j]    = sum_a pi'[a] * (Z'[j][a] - tlp'[a])             from 0.0f; product and sum round separately
 * For the current state q, d, E, tlp from Z in the same way, and
 *     bonus   = alpha * fminf(fmaxf(tlp[a_b], lo), 0.0f)
 *     y[b, j] = fmaf(gamma * V[j], 1.0f - done, r + bonus)
 * then td[b, i, j] = y[b, j] - Z_local(s_b, tl[b, i])[a_b] and the quantile-Huber loss as in mn_iqn_train_grad.  The policy comes
 * from the MEAN over the 8 quantile samples, so for te -> 0 the target tends to Z'[j][argmax_a q'], not to mn_iqn_train_grad's
 * per-sample max_a Z'[j][a].  There is one instruction sequence per output: alpha == 0 and done == 1 take no other path (with every
 * row done and alpha == 0, y == r and the step is mn_iqn_train_grad's bit for bit).  expf and logf differ between device and host
 * by units in the last place, so this rule has no bit-exact host twin: tests hold it to float64 by eager float32's own error.
 * Every workgroup runs both target forwards of its own two batch elements (no workgroup waits for another). */

/* ---- Target rules ----------------------------------------------------------------------------------
 * Which action the TD target bootstraps from, opt-in: mn_iqn_train_grad_rule forms y[b, j] by the rule below; loss, backward,
 * reduction, clip and Adam are mn_iqn_train_grad's.  mn_iqn_train_grad itself takes max_a Z'[j][a] PER SAMPLE j (the reference's
 * operator: sample j and sample j + 1 of one element may bootstrap from different actions).  The two rules here choose ONE action
 * a* per next state, from the mean over the samples, and every sample takes that action's quantile:
 *     MN_TARGET_MEAN     the IQN paper's rule (Dabney et al. 2018): the TARGET network chooses and values
 *     MN_TARGET_DOUBLE   Double-IQN: the LOCAL network chooses, the target network values
 * Per batch element b: reward r, done, gamma (the caller passes gamma ** n_step), the tau sets tt[b, j], ts[b, j], tl[b, i]
 * (i, j < 8), and with the TARGET weights
 *     Z'[j][a] = Z_target(s'_b, tt[b, j])[a]           the next state, as in mn_iqn_train_grad
 * All arithmetic is float32.
 *     Zs[j][a] = Z'[j][a]                               MN_TARGET_MEAN
 *              = Z_local(s'_b, ts[b, j])[a]             MN_TARGET_DOUBLE: the LOCAL weights on the NEXT state, third tau set
 *     q[a]     = 0.125f * (Zs[0][a] + Zs[1][a] + ... + Zs[7][a])      summed in index order from the first term
 *     a*       = the FIRST index that attains max_a q[a]: the incumbent starts as a = 0 and, scanning a = 1..8, is replaced
 *                only where q[a] is strictly greater
 *     y[b, j]  = fmaf(gamma * Z'[j][a*], 1.0f - done, r)
 * then td[b, i, j] = y[b, j] - Z_local(s_b, tl[b, i])[a_b] and the quantile-Huber loss as in mn_iqn_train_grad.  There is one
 * instruction sequence per output: done == 1 takes no other path (with every row done, y == r and the step is
 * mn_iqn_train_grad's bit for bit).  Every workgroup runs the selecting pass and the target forward of its own two batch
 * elements (no workgroup waits for another). */
#define MN_TARGET_MEAN 1
#define MN_TARGET_DOUBLE 2

/* ---- training episode log ----------------------------------------------------------------------
 * The record the reference prints at every training episode end (thirdparty/IQN/agent.py:118-119, 152-168) for the n envs of a
 * vector step, in one launch that needs no env handle and no host look.  reward_dev [n] f32, done_dev / info_dev [n] u8 are a
 * step's outputs.  Per env i, in float64, every operation rounding on its own:
 *     ret += disc * (double)reward[i];   disc *= discount;   len += 1
 * on the running state ep_ret_dev / ep_disc_dev [n] f64 and ep_len_dev [n] i32, which the caller initialises to 0 / 1 / 0.  Where
 * done[i] is set the env writes one record -- rec_step = step_index, rec_env = i, rec_len = len, rec_info = info[i] (MN_INFO_*),
 * rec_ret = ret, rec_eps = eps -- and its state goes back to (0, 1, 0).  The return is the RUNNING PRODUCT form above, not the
 * reference's `discount ** ep_length` power.
 * Records are compacted through *count_dev (u32, caller-zeroed): a wavefront claims one run of slots for its finished lanes with
 * one atomic add.  A slot >= capacity is not written but counted: *count_dev - capacity records were dropped.  The order of the
 * records of one call is unspecified. */
int mn_episode_log(const float *reward_dev, const uint8_t *done_dev, const uint8_t *info_dev, int32_t n, double discount,
                   int64_t step_index, float eps, double *ep_ret_dev, double *ep_disc_dev, int32_t *ep_len_dev, int64_t *rec_step,
                   int32_t *rec_env, int32_t *rec_len, uint8_t *rec_info, double *rec_ret, float *rec_eps, int64_t capacity,
                   uint32_t *count_dev, void *stream);

/* ---- IQN gradient step ------------------------------------------------------------------------
 * One optimizer step of IQNAgent.train (thirdparty/IQN/agent.py:269-304) on `batch` transitions gathered from the
 * replay ring (layout above) at rows idx_dev[batch] (i64): target-network forward on next_states, local-network
 * forward on states, quantile-Huber TD loss (kappa = 1, 8 x 8 tau pairs; agent.py:279-295, 401-407), backward.
 * All pointers are device pointers, float32 unless noted, 16-byte aligned.
 *   taus_*_dev [batch][8]     : the uniform(0,1) tau draws of model.py:149 for the target / local forward
 *   params_local/_target      : FLAT parameter vectors, 35 785 floats in ObsEncoder.named_parameters() order
 *                               (model.py:120-136): velocity_encoder.{weight[16][2],bias[16]}, goal_encoder.{[16][2],[16]},
 *                               sensor_encoder.{[176][22],[176]}, cos_embedding.{[208][64],[208]},
 *                               hidden_layer.{[64][208],[64]}, hidden_layer_2.{[64][64],[64]}, output_layer.{[9][64],[9]}
 *   workspace                 : mn_iqn_train_workspace_floats(batch) floats (per-workgroup partial gradients, norm partials, the
 *                               TD-target hand-off granules with their epoch word, the Adam ticket).  Call
 *                               mn_iqn_train_workspace_init(workspace, batch, stream) ONCE before the first step and then pass the same
 *                               buffer and batch, untouched, to every call of one learner: the workspace carries state between calls
 *                               (hand-off epoch, tickets, the staged next batch).  A workspace that was never initialised is refused
 *                               on the device: the step returns a NaN loss and leaves gradient, moments and parameters untouched
 *   grad_out [35 785]         : d loss / d params_local (un-clipped); loss_out [1]: the loss
 * mn_iqn_train_grad computes loss and gradient (2 kernels, deterministic: no float atomics).  The forward / backward launch has
 * two workgroup roles -- batch / 2 TARGET workgroups (lower block indices) run the target network and hand their 16 TD targets
 * each to the LOCAL workgroup of the same two batch elements inside the launch -- so it wants batch <= 256 (one workgroup per CU);
 * larger batches, and mn_iqn_train_set_mode(1), let every local workgroup compute its own targets.  The caller may average
 * grad_out over ranks (RCCL all-reduce(SUM); pass grad_scale = 1 / world_size and grad_rewritten = 1) before mn_iqn_train_adam,
 * which applies clip_grad_norm_(max_norm) (agent.py:299) to grad_scale * grad and one torch.optim.Adam update (agent.py:300;
 * exp_avg / exp_avg_sq [35 785], step_dev: i32 step counter on the device, incremented by the call; grad is overwritten with the
 * clipped gradient).  grad_rewritten = 0 promises that grad_out is exactly what the preceding mn_iqn_train_grad* call on the same
 * workspace left there (the norm then comes from partial sums that call stored); grad_rewritten = 2 that mn_iqn_train_exchange formed
 * them for grad_scale * grad; with grad_rewritten = 1 or (grad_rewritten = 0 and grad_scale != 1) the
 * norm is recomputed from grad.
 * batch must be even and <= 1024, num_taus must be 8.  Exact float32 (v_mfma_f32_16x16x4_f32). */
/* The whole gradient step of a single learner -- IQNAgent.train (agent.py:269-304) incl. clip_grad_norm_ and optimizer.step() -- as TWO
 * launches: forward / backward, then a launch in which every block reduces the partial gradients of its own 256 parameters, exchanges the norm
 * partials with the other blocks as self-tagged granules and applies clip + Adam (round 4) -- or, with MN_TRAIN_ONE_LAUNCH in `flags`, as ONE launch (the FUSED
 * step; batch a multiple of 16 and every workgroup a CU of its own: batch <= 256 on an MI355X; else two launches): the target workgroups of the forward /
 * backward launch are also its reduction + Adam blocks.  XCD-grouped: the partial-gradient rows of the workgroups that share an XCD (block index mod 8: the
 * dispatcher deals workgroups out round-robin) are summed inside that XCD's L2 and only the eight group rows cross to the other XCDs, as self-tagged granules the
 * reduction blocks poll.  All forms are bit-identical.  rng_state_dev != NULL: the batch is drawn in the
 * launch (arguments as mn_iqn_train_grad_sampled; idx_dev / taus_*_dev ignored); NULL: the given batch (as mn_iqn_train_grad).  params_local is
 * updated in place, grad_out receives the clipped gradient.  Bit-identical to mn_iqn_train_grad* + mn_iqn_train_adam(grad_scale = 1): those stay
 * for callers that put something between the two (the shared learner's all-reduce / exchange). */
int mn_iqn_train_step(const float *ring_states, const float *ring_next_states, const int64_t *ring_actions, const float *ring_rewards,
                      const float *ring_dones, int64_t ring_size, uint64_t *rng_state_dev, const int64_t *idx_dev, const float *taus_target_dev,
                      const float *taus_local_dev, int64_t *idx_out, float *taus_out, float *params_local, const float *params_target,
                      float *workspace, float *grad_out, float *loss_out, float *exp_avg, float *exp_avg_sq, int32_t *step_dev, int32_t batch,
                      int32_t num_taus, float gamma, int32_t flags, double lr, double beta1, double beta2, double eps, double max_norm, void *stream);
int64_t mn_iqn_train_workspace_floats(int32_t batch);
/* Diagnostic: float index inside the workspace of a u32 counter -- local workgroups of one-launch steps that did not run on the XCD of the first
 * workgroup of their group (block index % 8) since mn_iqn_train_workspace_init (their partial-gradient rows go through memory instead of staying in the
 * XCD's L2: correct, slower; the dispatcher deals workgroups out to the XCDs round-robin, so 0 is expected). */
int64_t mn_iqn_train_workspace_misplaced_word(int32_t batch);
/* Float index inside the workspace of the u32 STATUS word: reduction + Adam blocks of which a bounded wait ran out since mn_iqn_train_workspace_init -- a hand-off
 * inside a fused launch, or (shared learner) a peer's granules.  Such a block leaves moments and parameters untouched and writes NaN into its piece of the
 * gradient.  0 in a healthy run; the caller reads the word where it synchronises anyway (evaluation points, the end of a run) and treats non-zero as an error. */
int64_t mn_iqn_train_workspace_status_word(int32_t batch);
int mn_iqn_train_workspace_init(float *workspace, int32_t batch, void *stream);
/* The fused forms wait, inside a launch, for other workgroups of the same launch, which is only safe while those are resident together: the launch plan is made
 * from the device's CU count and the kernels' occupancy (round 5), and a device that cannot hold them takes three launches (four for a shared learner:
 * reduction, gather, Adam) -- bit-identical.  mn_iqn_train_plan: launches one gradient step takes on the current device for this batch and these flags
 * (exchange != 0: mn_iqn_train_step_xchg); < 0: -error.  mn_iqn_train_set_cu_limit: plan as if the device had at most n_cu CUs (0: what it reports) -- tests, and
 * ranks that share one GPU (each plans for its share). */
int mn_iqn_train_plan(int32_t batch, int32_t flags, int32_t exchange);
int mn_iqn_train_set_cu_limit(int32_t n_cu);

/* ---- One-shot gradient exchange of a shared learner (BASELINE configs[4]; SURVEY 8e: one flat 143 KB bucket per gradient step, latency-
 * bound).  Alternative to an RCCL all-reduce between mn_iqn_train_grad* and mn_iqn_train_adam: every rank owns a MAILBOX in device memory;
 * once a workspace is attached, the gradient step's reduction kernel also publishes the reduced gradient there as self-tagged 8-byte
 * granules {step tag, value} (system-scope stores); mn_iqn_train_exchange launches ONE kernel that reads all ranks' mailboxes -- the peers'
 * through IPC-mapped pointers, i.e. directly over xGMI -- polling each granule until it carries the current step's tag, and leaves
 *     grad = sum over ranks, in rank order (bit-identical on every rank; equal to an all-reduce(SUM) for two ranks)
 * plus the norm partials of grad_scale * grad, so that the step continues with mn_iqn_train_adam(..., grad_scale, grad_rewritten = 2).
 * Four launches per step instead of five (no collective launch, no separate norm pass), no host synchronisation, graph-capturable -- the form a device too
 * small for the fused launches falls back to; mn_iqn_train_step_xchg (below) is the exchange INSIDE the gradient step's own launch(es).
 *   mn_xchg_create(rank, world <= 8)    this rank's context + mailbox on the current device
 *   mn_xchg_export(x, handle[64])       hipIpcMemHandle_t of the mailbox, to be sent to every peer (e.g. torch.distributed.all_gather_object)
 *   mn_xchg_import(x, peer, handle[64]) maps a peer's mailbox (once per peer)
 *   mn_xchg_attach(x, workspace, batch) the learner that steps on `workspace` publishes into x's mailbox from now on (x = NULL detaches)
 *   mn_iqn_train_exchange(x, grad, workspace, batch, grad_scale, stream)   after mn_iqn_train_grad* on the same stream
 *   mn_xchg_status(x, &timeouts)        gathers that did not get a peer's granules within the bound (0 in a healthy run; the poll is bounded so that a
 *                                       missing peer can never hang the device; the step that timed out updates nothing and raises the workspace's
 *                                       status word too).  mn_xchg_set_timeout_ms(x, ms): the bound; default 30 s with peers (one of them may be
 *                                       evaluating or writing a checkpoint meanwhile), 2 s alone
 *   mn_xchg_memory_kind(x)              how the mailbox was allocated: 2 = uncached device memory (hipDeviceMallocUncached), 1 = fine-grained, 0 = plain
 *                                       hipMalloc (coarse-grained: cross-device visibility inside a running kernel is then not promised by the memory model)
 * All ranks must call the step functions the same number of times (the tag is the workspace's step count).  RCCL stays the default
 * transport of iqn/fused_train.py; this path is opt-in (IQNAgent.exchange = "mailbox"). */
/* ---- DQN baseline, acting: the greedy policy of the reference's sb3 `ObsEncoderPolicy` for n observation rows in ONE
 * launch -- encoders (no activation) -> hidden_layer -> hidden_layer_2 -> output_layer (thirdparty/stable_baselines3/common/
 * torch_layers.py:96-135) -> q_net.0 -> q_net.2 -> q_net.4 (dqn/policies.py:48-58, net_arch [64, 64]) -> argmax (:69-73), exact float32 MFMA.
 *   weights[18]   device pointers, nn.Linear layout: {velocity, goal, sensor}_encoder, hidden_layer, hidden_layer_2, output_layer,
 *                 q_net.0, q_net.2, q_net.4, each as (weight, bias)
 *   image_dev     caller-owned scratch of mn_dqn_image_floats() floats: the permuted weight image; repack != 0 rebuilds it from
 *                 `weights` in front of the launch (first call, and after the weights changed)
 *   qvals_dev     [n][9] Q-values or NULL; actions_dev [n] greedy actions (first maximum) or NULL */
int64_t mn_dqn_image_floats(void);
int mn_dqn_act(const float *obs_dev, const float *const *weights, float *image_dev, int32_t repack, float *qvals_dev, int32_t *actions_dev,
               int32_t n, void *stream);
/* DQN EPISODES in ONE launch: mn_rollout_policy with the greedy DQN policy (train_dqn.evaluate, the DQN rows of run_experiments.py:213-282).  Every env
 * of `h` runs its CURRENT episode -- starting from the observation in obs_dev -- for up to n_steps steps; per step it acts exactly as mn_dqn_act would
 * for its row (same network code, same weight image, argmax with the first maximum), then steps like mn_step.  An env that finishes is NOT reset: it
 * idles, its traces read reward 0 / done 1 / its terminal info code / action -1 from then on, obs_dev keeps its terminal observation and its terminal
 * pose and counters are stored; an env still alive after n_steps stores its state, so a second call continues the episode.  Bit-identical to a loop of
 * (mn_dqn_act, mn_step).  weights[18], image_dev, repack as mn_dqn_act.  Traces (device, any may be NULL) as mn_rollout_policy ([n_steps][n] ...), plus
 * q_trace_dev [n_steps][n][9] f32 (Q(s, .) of each step); obs / Q entries of steps after an env finished are not written.  MN_ERR_INVALID for a NULL
 * h / weights / one of the 18 pointers / image_dev / obs_dev, or n_steps < 1.  No allocation, no host synchronisation, caller's stream. */
int mn_rollout_dqn(mn_handle *h, const float *const *weights, float *image_dev, int32_t repack, int32_t n_steps, float *obs_dev,
                   float *obs_trace_dev, float *reward_trace_dev, uint8_t *done_trace_dev, uint8_t *info_trace_dev, int32_t *action_trace_dev,
                   float *q_trace_dev, void *stream);
/* Packs weights[18] (as mn_dqn_act) into image_out_dev[mn_dqn_image_floats()] (device, 16-byte aligned) on `stream` -- the image mn_dqn_act and
 * mn_rollout_dqn build with repack != 0 --: a snapshot of the policy that mn_rollout_dqn_groups can act with later, whatever happens to the weights
 * meanwhile.  MN_ERR_INVALID for a NULL argument, a NULL entry among the 18 pointers or a misaligned destination. */
int mn_dqn_export_image(const float *const *weights, float *image_out_dev, void *stream);
/* DQN episodes of MANY sets of weights in ONE launch: mn_rollout_dqn with a weight image per GROUP of rows.  Row e of `h` belongs to group
 * e / rows_per_group and is row e % rows_per_group of it.  Group g acts with the image at images_dev + g * image_stride (floats; images of
 * mn_dqn_export_image, 16-byte aligned) and computes -- traces, final rows, poses and counters -- bit for bit what mn_rollout_dqn computes on a handle
 * of rows_per_group rows holding those worlds.  Episode semantics and traces ([n_steps][n] ..., indexed by the handle's row e, any may be NULL) as
 * mn_rollout_dqn.  The launch has n_groups * ceil(rows_per_group / 8) workgroups, possibly more than the device runs at once; none waits for
 * another, and nothing is counted on the device: the longest episode of a group is read from its columns of the done trace.  No allocation, no host
 * synchronisation, caller's stream.
 * MN_ERR_INVALID, without launching, if n_groups < 1, rows_per_group < 1 or n_groups * rows_per_group is not the handle's n_envs, if image_stride is
 * below mn_dqn_image_floats() or no multiple of 4 (or images_dev is not 16-byte aligned), for a NULL h / images_dev / obs_dev, or n_steps < 1.  It
 * records no sub-step trajectories: an attached trace (mn_set_trajectory_trace) is detached and the call refused. */
int mn_rollout_dqn_groups(mn_handle *h, const float *images_dev, int64_t image_stride, int32_t n_groups, int32_t rows_per_group, int32_t n_steps,
                          float *obs_dev, float *obs_trace_dev, float *reward_trace_dev, uint8_t *done_trace_dev, uint8_t *info_trace_dev,
                          int32_t *action_trace_dev, float *q_trace_dev, void *stream);
/* ---- Fused gradient step of the DQN baseline (csrc/dqn_train.hip): ONE launch = one optimizer step of DQNAgent.train (sb3 DQN.train, dqn/dqn.py:188-230):
 * target forward on next_states, max over the 9 actions, y = r + (1 - done) gamma max; local forward on states, gather Q[a], smooth_l1_loss (beta 1,
 * mean); backward through the 9 layers; clip_grad_norm_(max_norm); torch.optim.Adam (step counter t = *step_dev + 1, advanced by the launch).
 *   ring_*            the replay ring in mn_replay_append's layout: states / next_states [cap][26] f32, actions [cap] i64, rewards / dones [cap] f32
 *   rng_state_dev     u64[2] = {seed, call counter}: the batch is mn_iqn_sample's draw (batch DISTINCT rows of [0, ring_size), same keyed
 *                     permutation), the counter is advanced by exactly one; NULL: the rows are idx_dev [batch] i64
 *   idx_out           [batch] i64, receives the rows (NULL: not written)
 *   params_local      flat [27 650] f32 in DQNPolicy.q_net.named_parameters() order (features_extractor.{velocity,goal,sensor}_encoder,
 *                     hidden_layer, hidden_layer_2, output_layer, q_net.{0,2,4}; weight then bias, nn.Linear [out][in]), updated in place;
 *                     params_target the same layout (read only)
 *   workspace         mn_dqn_train_workspace_floats(batch) floats, 16-byte aligned, ZERO-initialised once by the caller (it holds the
 *                     workgroups' ticket, which every launch leaves at 0); one workspace per concurrently running step
 *   grad_out [27 650] the clipped gradient; loss_out [1] the loss; exp_avg / exp_avg_sq [27 650] Adam's moments
 * batch 1..256, exact float32, deterministic (no float atomics, fixed summation order, independent of workgroup placement).
 * mn_dqn_train_workspace_floats: < 0 for a batch outside 1..256. */
int64_t mn_dqn_train_workspace_floats(int32_t batch);
int mn_dqn_train_step(const float *ring_states, const float *ring_next_states, const int64_t *ring_actions, const float *ring_rewards,
                      const float *ring_dones, int64_t ring_size, uint64_t *rng_state_dev, const int64_t *idx_dev, int64_t *idx_out,
                      float *params_local, const float *params_target, float *workspace, float *grad_out, float *loss_out, float *exp_avg,
                      float *exp_avg_sq, int32_t *step_dev, int32_t batch, float gamma, double lr, double beta1, double beta2, double eps,
                      double max_norm, void *stream);
/* MANY gradient steps per call: n_steps consecutive mn_dqn_train_step, bit for bit.  After the call params_local, exp_avg, exp_avg_sq, *step_dev,
 * rng_state_dev[1] (advanced by n_steps), grad_out (the LAST step's clipped gradient), every losses_out[k] and every row of idx_out equal what n_steps
 * calls of mn_dqn_train_step leave from the same state: the single step is the specification, its summation orders included.  Two launches on the
 * caller's stream: the TD targets of all n_steps x batch samples, device-wide (the target network and the ring are constant while the steps run, and
 * the rows of step k depend only on {seed, call counter + k, ring_size}), then ONE workgroup that carries both 16-sample tiles through every step --
 * local forward, loss, backward, ordered sum, clip, Adam -- with no launch boundary, ticket or cross-workgroup wait between steps.
 *   idx_dev / idx_out  [n_steps][batch] i64 (idx_dev: the rows of every step when rng_state_dev is NULL)
 *   losses_out         [n_steps] f32
 *   workspace          mn_dqn_train_steps_workspace_floats(batch, n_steps) floats, 16-byte aligned, no initialisation needed; one per running call
 * The caller copies the target network BETWEEN calls (split a run of steps at the copies).  Other arguments as mn_dqn_train_step.
 * MN_ERR_INVALID, without launching: batch outside 1..32, n_steps outside 1..MN_DQN_MAX_STEPS, ring_size < batch in draw mode, rng_state_dev and
 * idx_dev both NULL, a NULL buffer, a misaligned workspace.  mn_dqn_train_steps_workspace_floats: < 0 for a batch or n_steps outside those ranges.
 * mn_dqn_train_steps_parts: the same call with its launches selectable, for measurements -- parts 1: the targets (and Adam scalars) only, 2: the chain only,
 * on the targets a parts-1 call left in the workspace, 3: both. */
#define MN_DQN_MAX_STEPS 1024
int64_t mn_dqn_train_steps_workspace_floats(int32_t batch, int32_t n_steps);
int mn_dqn_train_steps(const float *ring_states, const float *ring_next_states, const int64_t *ring_actions, const float *ring_rewards,
                       const float *ring_dones, int64_t ring_size, uint64_t *rng_state_dev, const int64_t *idx_dev, int64_t *idx_out,
                       float *params_local, const float *params_target, float *workspace, float *grad_out, float *losses_out, float *exp_avg,
                       float *exp_avg_sq, int32_t *step_dev, int32_t batch, int32_t n_steps, float gamma, double lr, double beta1, double beta2,
                       double eps, double max_norm, void *stream);
int mn_dqn_train_steps_parts(const float *ring_states, const float *ring_next_states, const int64_t *ring_actions, const float *ring_rewards,
                             const float *ring_dones, int64_t ring_size, uint64_t *rng_state_dev, const int64_t *idx_dev, int64_t *idx_out,
                             float *params_local, const float *params_target, float *workspace, float *grad_out, float *losses_out, float *exp_avg,
                             float *exp_avg_sq, int32_t *step_dev, int32_t batch, int32_t n_steps, float gamma, double lr, double beta1, double beta2,
                             double eps, double max_norm, int32_t parts, void *stream);
/* MANY LEARNERS per launch: G independent DQN learners with common hyper-parameters (the seeds of one config) take their gradient step in ONE launch, or
 * their n_steps steps in one multi-step call.  The learner is a grid dimension: workgroup (w, g) of the grouped step is workgroup w of learner g's
 * mn_dqn_train_step on g's own buffers and its own slice of the workspace, the grouped multi-step call runs learner g's TD-target tiles and, as workgroup g,
 * its whole chain.  The kernels inline the same bodies as the single calls, so EVERY learner is bit for bit what mn_dqn_train_step / mn_dqn_train_steps
 * leave from the same state -- parameters, moments, step and draw counters, gradient, every loss, every row.
 * mn_dqn_learner: the device pointers of ONE learner (arguments of the same names of mn_dqn_train_step; grad = grad_out, step = step_dev), caller-owned
 * and alive as long as the group is used.  rng_state may be NULL if the group is only ever called with rows (idx_dev).
 * mn_dqn_group_create validates on the host, uploads the pointer table once (one allocation, one synchronous copy) and returns the handle.
 * MN_ERR_INVALID: n_learners outside 1..MN_DQN_MAX_LEARNERS, a NULL among the required pointers, or two learners that alias -- a buffer one learner
 * writes (params_local, grad, exp_avg, exp_avg_sq over their 27 650 floats, step, a non-NULL rng_state) overlapping a buffer another learner writes or
 * the params_target another reads: such learners would race silently.  Learners may share a ring.
 * Per call, common to the group: ring_size (a lockstep run has the rings equally full), batch and the hyper-parameters.
 *   idx_dev     [G][n_steps][batch] i64, the rows of every learner and step (the draw states are left alone), or NULL: every learner draws from its own
 *               rng_state, which advances as in the single calls (MN_ERR_INVALID if a learner of the group has none)
 *   idx_out     [G][n_steps][batch] i64 or NULL;  losses_out [G][n_steps] f32   (n_steps = 1 for mn_dqn_group_train_step)
 *   workspace   [G][stride] f32, 16-byte aligned, ZERO before the first call (the tickets of the step stay zero behind every launch); stride =
 *               mn_dqn_train_workspace_floats(batch) (step) or mn_dqn_train_steps_workspace_floats(batch, n_steps) (multi-step call), rounded up to a
 *               multiple of 4 floats; one workspace per concurrently running call
 * Limits as the single calls': batch 1..256 (step), batch 1..32 and n_steps 1..MN_DQN_MAX_STEPS (multi-step call), batch <= ring_size < 2^31; outside them,
 * for a NULL group / workspace / losses_out or a misaligned workspace: MN_ERR_INVALID, without launching.  One launch (step) or two (multi-step call) on
 * the caller's stream, no allocation, no host synchronisation.  The target networks are copied by the caller BETWEEN calls. */
typedef struct mn_dqn_learner {      /* device pointers of ONE learner, caller-owned */
    const float *ring_states, *ring_next_states; const int64_t *ring_actions; const float *ring_rewards, *ring_dones;
    uint64_t *rng_state;             /* {seed, call counter}; may be NULL if the group is only ever called with rows */
    float *params_local; const float *params_target; float *grad, *exp_avg, *exp_avg_sq; int32_t *step;
} mn_dqn_learner;
typedef struct mn_dqn_group mn_dqn_group;
#define MN_DQN_MAX_LEARNERS 64
int mn_dqn_group_create(const mn_dqn_learner *learners_host, int32_t n_learners, mn_dqn_group **out);
int mn_dqn_group_destroy(mn_dqn_group *g);
int mn_dqn_group_train_step(mn_dqn_group *g, int64_t ring_size, const int64_t *idx_dev, int64_t *idx_out, float *workspace, float *losses_out,
                            int32_t batch, float gamma, double lr, double beta1, double beta2, double eps, double max_norm, void *stream);
int mn_dqn_group_train_steps(mn_dqn_group *g, int64_t ring_size, const int64_t *idx_dev, int64_t *idx_out, float *workspace, float *losses_out,
                             int32_t batch, int32_t n_steps, float gamma, double lr, double beta1, double beta2, double eps, double max_norm,
                             void *stream);

/* MANY IQN LEARNERS per launch: G independent IQN learners with common hyper-parameters (the seeds of one config) take their gradient step in THREE launches
 * on the caller's stream, the learner being the second grid dimension of each: forward / backward (batch / 2 x G workgroups, every workgroup computing the TD
 * targets of its own two batch elements), the fixed-order reduction (280 x G) and clip + Adam (140 x G).  These are the forms of the single step in which no
 * workgroup waits for another workgroup of its launch, so a grouped launch may be larger than the device; the fused one- and two-launch forms of
 * mn_iqn_train_step have no grouped counterpart.  The kernels inline the same bodies as the single calls: EVERY learner is bit for bit what mn_iqn_train_step
 * (any of its forms) leaves from the same state -- loss, parameters, clipped gradient, moments, step counter, generator state, the drawn rows and taus -- and
 * grouped and single calls may be interleaved on one learner in any order: the hand-off epoch, the tickets and the staging tag live in the learner's own
 * workspace.  A grouped step stages nothing (MN_TRAIN_STAGE_NEXT has no grouped form) and marks the workspace "nothing staged"; mn_iqn_train_set_mode and the
 * MN_TRAIN_* flags do not apply.
 * mn_iqn_learner: the device pointers of ONE learner -- the pointer arguments of mn_iqn_train_step of the same names (grad = grad_out, loss = loss_out, step =
 * step_dev); caller-owned, alive as long as the group is used.  workspace: that learner's own, mn_iqn_train_workspace_floats(batch) floats, initialised by
 * mn_iqn_train_workspace_init.  rng_state, idx_out and taus_out may be NULL in a group that is only ever called with given batches.
 * mn_iqn_group_create validates on the host, uploads the pointer table once (one allocation, one synchronous copy) and returns the handle.  MN_ERR_INVALID:
 * n_learners outside 1..MN_IQN_MAX_LEARNERS, batch odd, < 2 or > 1024, a NULL among the required pointers, or two learners that alias -- a buffer one learner
 * writes (params_local, grad, exp_avg, exp_avg_sq over their 35 785 floats, the workspace over its floats, loss, step, and where given rng_state [2] u64,
 * idx_out [batch] i64, taus_out [2][batch][8] f32) overlapping a buffer another learner writes or the params_target another reads.  Learners may share a ring.
 * mn_iqn_group_train_step: idx_dev [G][batch] i64, taus_target_dev / taus_local_dev [G][batch][8] f32 -- all three NULL: every learner draws its batch from
 * its own rng_state over the first ring_size rows and advances it exactly as mn_iqn_train_step does; all three given: the generator states are left alone.
 * MN_ERR_INVALID without launching: a NULL group, a mixed NULL / non-NULL triple, ring_size < batch or >= 2^31 when drawing, drawing in a group with a learner
 * without rng_state.  No allocation, no synchronisation.  The target networks are copied by the caller BETWEEN calls. */
typedef struct mn_iqn_learner {      /* device pointers of ONE learner, caller-owned */
    const float *ring_states, *ring_next_states; const int64_t *ring_actions; const float *ring_rewards, *ring_dones;
    uint64_t *rng_state;             /* {seed, call counter}; may be NULL if the group is only ever called with given batches */
    float *params_local; const float *params_target; float *workspace, *grad, *loss, *exp_avg, *exp_avg_sq; int32_t *step;
    int64_t *idx_out; float *taus_out;      /* the drawn rows [batch] and taus [2][batch][8] of the last drawn step, or NULL */
} mn_iqn_learner;
typedef struct mn_iqn_group mn_iqn_group;
#define MN_IQN_MAX_LEARNERS 64
int mn_iqn_group_create(const mn_iqn_learner *learners_host, int32_t n_learners, int32_t batch, mn_iqn_group **out);
int mn_iqn_group_destroy(mn_iqn_group *g);
int mn_iqn_group_train_step(mn_iqn_group *g, int64_t ring_size, const int64_t *idx_dev, const float *taus_target_dev, const float *taus_local_dev, float gamma,
                            double lr, double beta1, double beta2, double eps, double max_norm, void *stream);

/* MANY IQN ACTORS per launch: the act call and the replay append of G actors with one row count (the seeds of one config, stacked in ONE env handle of G n
 * rows: actor g owns rows [g n, (g + 1) n)) in one launch each on the caller's stream, the actor being the second grid dimension.  The kernels run the single
 * calls' own bodies: actor g gets, bit for bit, what mn_iqn_act_rng(ctx_g, obs + 26 g n, weights_g, rng_state_g, draws_g, NULL, cvar, eps, actions + g n,
 * NULL, NULL, n, 32, stream) leaves -- the actions, the [33 n] draws keyed by the row's index INSIDE the group, the call counter + 1, the context's
 * split-f16 image and constants rebuilt exactly when that context is stale (the stale contexts travel as a 64-bit mask argument), its stale flag cleared --
 * so single and grouped calls may be interleaved on one context.  With mn_iqn_set_greedy_rows on (the default) and eps > 0 only the rows that do not explore
 * run the network, each group listing its rows in its own context's buffer; with eps == 0 or the switch off every row runs.
 * mn_iqn_actor: the pointers of ONE actor, caller-owned, alive while the group is used; weights is read at create (the 14 device pointers are copied into the
 * group's device table).  The five ring pointers are mn_replay_append's and may ALL be NULL in EVERY actor of a group that only ever acts.
 * mn_iqn_actor_group_create validates on the host, makes sure every context's greedy-row buffer holds rows_per_group rows and uploads the table once (one
 * allocation, one synchronous copy); nothing allocates or synchronises afterwards.  MN_ERR_INVALID, before anything touches the device: n_actors outside
 * 1..MN_IQN_MAX_ACTORS, rows_per_group < 1, a NULL among the required pointers, rings given in part, a context on another device than the current one, a
 * context that is not variant 2 with per-row taus (tau mode 0), or two actors that share a context, overlap in draws or rng_state, or share a ring array.
 * mn_iqn_actor_group_act: obs_dev [G n][26], actions_dev [G n].  MN_ERR_INVALID without launching: a NULL argument, another current device, a context whose
 * variant or tau mode was changed, contexts that disagree on mn_iqn_set_greedy_rows, a context with late rows armed (mn_iqn_set_late_rows has no grouped
 * form), or a context whose greedy-row buffer a larger single call has replaced since create.  Workgroups per group: min(ceil(n / 8), max(1, CUs / G)) --
 * every workgroup with a row copies the 154-KB image into LDS, so a group gets its share of the CUs; mn_iqn_set_grid on the FIRST actor's context replaces
 * the share by its own cap (results do not depend on the count).
 * mn_iqn_actor_group_append: mn_replay_append per actor -- row i of group g goes to slot (ptr + i - first) mod capacity of ring g, first = max(0, n -
 * capacity), rows below first are not stored: the bytes mn_step_append writes.  ptr and capacity are common to the group; the caller advances ptr.
 * MN_ERR_INVALID: a group without rings, a NULL argument, capacity <= 0, ptr outside [0, capacity). */
typedef struct mn_iqn_actor {        /* device pointers / handles of ONE actor, caller-owned */
    mn_iqn_ctx *ctx;                 /* its act context: weight image, scale constants, greedy-row list, stale flag */
    const float *const *weights;     /* host array of 14 device pointers, as mn_iqn_act */
    uint64_t *rng_state;             /* {seed, call counter} */
    float *draws;                    /* [33 * rows_per_group] */
    float *ring_states, *ring_next_states; int64_t *ring_actions; float *ring_rewards, *ring_dones;
} mn_iqn_actor;
typedef struct mn_iqn_actor_group mn_iqn_actor_group;
#define MN_IQN_MAX_ACTORS 64
int mn_iqn_actor_group_create(const mn_iqn_actor *actors_host, int32_t n_actors, int32_t rows_per_group, mn_iqn_actor_group **out);
int mn_iqn_actor_group_destroy(mn_iqn_actor_group *g);
int mn_iqn_actor_group_act(mn_iqn_actor_group *g, const float *obs_dev, float cvar, float eps, int32_t *actions_dev, void *stream);
int mn_iqn_actor_group_append(mn_iqn_actor_group *g, const float *obs_dev, const int32_t *actions_dev, const float *reward_dev,
                              const float *next_obs_dev, const uint8_t *done_dev, int64_t ptr, int64_t capacity, void *stream);

/* ---- DQN collect on the device (csrc/dqn_collect.hip): the epsilon-greedy act of DQN training in ONE launch.  mn_dqn_act plus the exploration: row e
 * draws u_e = u01(e, k0, k1), (k0, k1) = draw_keys(seed, call_index) -- the counter-based generator of the IQN act kernels (csrc/iqn_act_common.h) -- and
 * acts greedily iff u_e > eps, else with min((int)(u_e / eps * 9.0f), 8) in float32; !(eps > 0): greedy everywhere.  seed and call_index are passed by
 * value: there is no generator state on the device and nothing to advance; the caller counts its calls.
 *   obs_dev, weights[18], image_dev, repack, n   as mn_dqn_act
 *   explore_u_dev   [n] the uniforms, or NULL
 *   qvals_dev       [n][9] Q-values of EVERY row, exploring ones included, or NULL.  A row's Q-values and greedy action are mn_dqn_act's bit for bit.
 *                   With NULL only rows that act greedily need the network: a wavefront whose 16 rows all explore skips it, and a workgroup whose
 *                   rows all explore does not load the weight image
 *   actions_dev     [n], required
 * MN_ERR_INVALID, without launching: a NULL obs_dev / weights / weight / image_dev / actions_dev, n <= 0.  No allocation, no host synchronisation. */
int mn_dqn_act_rng(const float *obs_dev, const float *const *weights, float *image_dev, int32_t repack, uint64_t seed, uint64_t call_index, float eps,
                   float *explore_u_dev, float *qvals_dev, int32_t *actions_dev, int32_t n, void *stream);

/* MANY DQN ACTORS per launch: mn_dqn_act_rng and mn_replay_append of G actors with one row count (the seeds of one config, stacked in ONE env handle of
 * G n rows: actor g owns rows [g n, (g + 1) n)), the actor being the second grid dimension.  Actor g gets, bit for bit, what mn_dqn_act_rng(obs + 26 g n,
 * weights_g, image_g, stale bit g, seed_g, call_index_host[g], eps, NULL, NULL, actions + g n, n, stream) and mn_replay_append into its ring leave: the
 * draw's index is the row INSIDE the group.  Nothing is hidden in the library, so grouped and single calls interleave freely.
 * mn_dqn_actor: caller-owned, alive while the group is used; the 18 weight pointers are copied into the group's device table at create.  The five ring
 * pointers are mn_replay_append's and may ALL be NULL in EVERY actor of a group that only ever acts.
 * mn_dqn_actor_group_create: one allocation, one synchronous copy; nothing allocates or synchronises afterwards.  MN_ERR_INVALID, before anything touches
 * the device: n_actors outside 1..MN_DQN_MAX_ACTORS, rows_per_group < 1, a NULL weights / weight / image, rings given in part, or two actors that share an
 * image or a ring array.
 * mn_dqn_actor_group_act: at most two launches.  The weight images of the actors whose bit of stale_mask is set are rebuilt first (one launch on grid
 * (pack blocks, G), skipped when the mask is 0); then the act launch.  call_index_host [G] is read during the call (copied into the argument block: no
 * device copy, no synchronisation).  Workgroups per group: min(ceil(tiles / 8), max(1, CUs / G)), tiles = ceil(n / 16);
 * mn_dqn_actor_group_set_grid(g, k) replaces the share max(1, CUs / G) by k (0: the default again); results do not depend on the count.  MN_ERR_INVALID
 * without launching: a NULL argument, a bit of stale_mask at or above G, another current device than at create.
 * mn_dqn_actor_group_append: mn_iqn_actor_group_append's semantics into this table's rings -- row i of group g goes to slot (ptr + i - first) mod capacity
 * of ring g, first = max(0, n - capacity); ptr and capacity are common to the group; the caller advances ptr.  MN_ERR_INVALID: a group without rings, a
 * NULL argument, capacity <= 0, ptr outside [0, capacity). */
typedef struct mn_dqn_actor {        /* device pointers of ONE actor, caller-owned */
    const float *const *weights;     /* host array of 18 device pointers, as mn_dqn_act */
    float *image;                    /* its weight image, mn_dqn_image_floats() floats */
    uint64_t seed;                   /* of its exploration draws */
    float *ring_states, *ring_next_states; int64_t *ring_actions; float *ring_rewards, *ring_dones;
} mn_dqn_actor;
typedef struct mn_dqn_actor_group mn_dqn_actor_group;
#define MN_DQN_MAX_ACTORS 64
int mn_dqn_actor_group_create(const mn_dqn_actor *actors_host, int32_t n_actors, int32_t rows_per_group, mn_dqn_actor_group **out);
int mn_dqn_actor_group_destroy(mn_dqn_actor_group *g);
int mn_dqn_actor_group_set_grid(mn_dqn_actor_group *g, int32_t workgroups_per_group);
int mn_dqn_actor_group_act(mn_dqn_actor_group *g, const float *obs_dev, float eps, uint64_t stale_mask, const uint64_t *call_index_host,
                           int32_t *actions_dev, void *stream);
int mn_dqn_actor_group_append(mn_dqn_actor_group *g, const float *obs_dev, const int32_t *actions_dev, const float *reward_dev,
                              const float *next_obs_dev, const uint8_t *done_dev, int64_t ptr, int64_t capacity, void *stream);

typedef struct mn_xchg mn_xchg;
int mn_xchg_create(int32_t rank, int32_t world, mn_xchg **out);
int mn_xchg_export(mn_xchg *x, void *handle_out);
int mn_xchg_import(mn_xchg *x, int32_t peer_rank, const void *handle);
int mn_xchg_attach(mn_xchg *x, float *workspace, int32_t batch, void *stream);
int mn_iqn_train_exchange(mn_xchg *x, float *grad, float *workspace, int32_t batch, float grad_scale, void *stream);
int mn_xchg_memory_kind(mn_xchg *x);
int mn_xchg_set_timeout_ms(mn_xchg *x, int64_t ms);
/* mn_iqn_train_step for a SHARED learner: the exchange happens INSIDE the reduction + clip + Adam role (every Adam block publishes its 64
 * reduced columns into this rank's mailbox, gathers the same columns of every rank in rank order and continues with grad_scale x the sum).  As many
 * launches per gradient step as a single learner's -- ONE with MN_TRAIN_ONE_LAUNCH (round 5), two without; bit-identical to the four-launch sequence
 * above, which is also what a device too small for the fused launches takes.  Arguments as mn_iqn_train_step. */
int mn_iqn_train_step_xchg(mn_xchg *x, const float *ring_states, const float *ring_next_states, const int64_t *ring_actions,
                           const float *ring_rewards, const float *ring_dones, int64_t ring_size, uint64_t *rng_state_dev, const int64_t *idx_dev,
                           const float *taus_target_dev, const float *taus_local_dev, int64_t *idx_out, float *taus_out, float *params_local,
                           const float *params_target, float *workspace, float *grad_out, float *loss_out, float *exp_avg, float *exp_avg_sq,
                           int32_t *step_dev, int32_t batch, int32_t num_taus, float gamma, int32_t flags, double lr, double beta1, double beta2,
                           double eps, double max_norm, float grad_scale, void *stream);
int mn_xchg_status(mn_xchg *x, int32_t *timeouts);
/* Text of the last failure of an mn_xchg_* call on this exchange ("" if none; valid until the next call on it). */
const char *mn_xchg_last_error(const mn_xchg *x);
int mn_xchg_destroy(mn_xchg *x);
/* ReplayBuffer.sample (replay_buffer.py:42-47, random.sample: `batch` DISTINCT uniform rows of [0, ring_size)) -> idx_out
 * [batch] i64, plus n_taus_total uniform [0,1) floats -> taus_out (the step's tau draws, model.py:149; may be 0).  Slot k reads
 * row perm(k) of a keyed pseudo-random permutation of [0, ring_size) (4-round Feistel network + cycle walking): distinct by
 * construction, O(1) per slot.  rng_state_dev: u64[2] = {seed, call counter} on the device; the counter is advanced by the call.
 * batch <= 1024, ring_size >= batch. */
int mn_iqn_sample(int64_t ring_size, int32_t batch, uint64_t *rng_state_dev, int64_t *idx_out, float *taus_out,
                  int32_t n_taus_total, void *stream);
int mn_iqn_train_grad(const float *ring_states, const float *ring_next_states, const int64_t *ring_actions,
                      const float *ring_rewards, const float *ring_dones, const int64_t *idx_dev,
                      const float *taus_target_dev, const float *taus_local_dev, const float *params_local,
                      const float *params_target, float *workspace, float *grad_out, float *loss_out, int32_t batch,
                      int32_t num_taus, float gamma, void *stream);
/* mn_iqn_train_grad for prioritized replay ("Prioritized replay" above): element b's loss terms are scaled by weights_dev[b] --
 * loss = 1 / (B N) sum_b w_b sum_ij rho_ij, in float32 the scale (w_b * (1.0f / (B N))) applied where mn_iqn_train_grad applies 1 / (B N),
 * so weights of 1.0f give its gradient and loss bit for bit -- and absdelta_out [batch] f32 receives
 *     delta_b = (1 / N^2) sum_ij |td_ij|      float32: the 8 |td| of a local-tau row i added in order j = 0..7 from 0.0f, the 8 row sums of
 *                                             an element added in order i = 0..7 from 0.0f, times 1 / 64.
 * Every workgroup runs the target forward of its own two batch elements (no workgroup waits for another), then the same reduction as
 * mn_iqn_train_grad; mn_iqn_train_adam follows unchanged. */
int mn_iqn_train_grad_per(const float *ring_states, const float *ring_next_states, const int64_t *ring_actions,
                          const float *ring_rewards, const float *ring_dones, const int64_t *idx_dev,
                          const float *taus_target_dev, const float *taus_local_dev, const float *params_local,
                          const float *params_target, float *workspace, float *grad_out, float *loss_out, int32_t batch,
                          int32_t num_taus, float gamma, const float *weights_dev, float *absdelta_out, void *stream);
/* mn_iqn_train_grad with the Munchausen target ("Munchausen target" above): taus_munch_dev [batch][8] is the third tau set (the
 * target network's pass over the current states; elements [2 B 8, 3 B 8) of an mn_iqn_sample call with n_taus_total = 3 B 8),
 * gamma is gamma ** n_step.  targets_out [batch][8] f32 receives y (NULL: not written; the gradient's bits do not depend on it).
 * mn_iqn_grad_reduce's sum and mn_iqn_train_adam follow unchanged.  MN_ERR_INVALID, with nothing launched: an odd batch or one
 * outside 2..1024, num_taus != 8, entropy_tau not finite or not above 0, clip_lo above 0 or NaN, alpha negative or not finite,
 * a NULL pointer other than targets_out. */
int mn_iqn_train_grad_munch(const float *ring_states, const float *ring_next_states, const int64_t *ring_actions,
                            const float *ring_rewards, const float *ring_dones, const int64_t *idx_dev,
                            const float *taus_target_dev, const float *taus_munch_dev, const float *taus_local_dev,
                            const float *params_local, const float *params_target, float *workspace, float *grad_out, float *loss_out,
                            int32_t batch, int32_t num_taus, float gamma, float alpha, float entropy_tau, float clip_lo,
                            float *targets_out, void *stream);
/* mn_iqn_train_grad with a greedy-on-mean target ("Target rules" above): rule is MN_TARGET_MEAN or MN_TARGET_DOUBLE.
 * taus_select_dev [batch][8] is the third tau set (the local network's selecting pass over the next states; elements
 * [2 B 8, 3 B 8) of an mn_iqn_sample call with n_taus_total = 3 B 8); it is read only under MN_TARGET_DOUBLE and may be NULL under
 * MN_TARGET_MEAN.  gamma is gamma ** n_step.  targets_out [batch][8] f32 receives y and select_out [batch] i32 receives a* (NULL:
 * not written; the gradient's bits do not depend on either).  mn_iqn_grad_reduce's sum and mn_iqn_train_adam follow unchanged.
 * MN_ERR_INVALID, with nothing launched: rule 0 (the per-sample max has mn_iqn_train_grad) or any other rule, an odd batch or one
 * outside 2..1024, num_taus != 8, a NULL pointer other than targets_out, select_out and -- under MN_TARGET_MEAN -- taus_select_dev. */
int mn_iqn_train_grad_rule(const float *ring_states, const float *ring_next_states, const int64_t *ring_actions,
                           const float *ring_rewards, const float *ring_dones, const int64_t *idx_dev,
                           const float *params_local, const float *params_target, float *workspace, float *grad_out, float *loss_out,
                           const float *taus_target_dev, const float *taus_select_dev, const float *taus_local_dev,
                           int32_t batch, int32_t num_taus, float gamma, int32_t rule, float *targets_out, int32_t *select_out,
                           void *stream);
/* The same gradient step with the batch drawn inside the launch: every workgroup of the forward / backward kernel evaluates
 * mn_iqn_sample's permutation for its own two slots (and its own taus) from {seed, call counter}, so there is no sampling launch.
 * Bit-identical to mn_iqn_sample followed by mn_iqn_train_grad from the same state; the call counter is advanced once (by the
 * reduction kernel).  idx_out [batch] i64 and taus_out [2][batch][8] receive the batch (NULL: not written).  Needs
 * batch <= ring_size < 2^31. */
/* flags: MN_TRAIN_STAGE_NEXT -- the reduction kernel of this step also draws the NEXT step's batch (call counter + 1) from the ring
 * as it is now and stages it (rows, transitions, taus) in the workspace; MN_TRAIN_USE_STAGED -- start from the batch a previous call
 * staged instead of drawing and gathering it (one memory round trip at the head of the launch instead of three dependent ones).
 * The staged batch is used only if it was drawn for this call counter and this ring_size (checked on the device; otherwise the
 * launch draws and gathers as usual), and its transitions are those the ring held when it was staged: pass MN_TRAIN_USE_STAGED only
 * if the ring was not written since the staging call (then the step is bit-identical to the unstaged one). */
#define MN_TRAIN_USE_STAGED 1
#define MN_TRAIN_STAGE_NEXT 2
#define MN_TRAIN_ONE_LAUNCH 4      /* mn_iqn_train_step[_xchg]: the fused step -- reduction + clip + Adam inside the forward / backward launch */
#define MN_TRAIN_TEST_MISPLACE(k) ((k) << 4)   /* test hook, k = 1..3, with MN_TRAIN_ONE_LAUNCH: treat some workgroups as if they had landed on another XCD */
int mn_iqn_train_grad_sampled(const float *ring_states, const float *ring_next_states, const int64_t *ring_actions,
                              const float *ring_rewards, const float *ring_dones, int64_t ring_size, uint64_t *rng_state_dev,
                              int64_t *idx_out, float *taus_out, const float *params_local, const float *params_target,
                              float *workspace, float *grad_out, float *loss_out, int32_t batch, int32_t num_taus, float gamma,
                              int32_t flags, void *stream);
int mn_iqn_train_adam(float *params, float *grad, float *exp_avg, float *exp_avg_sq, int32_t *step_dev, float *workspace,
                      int32_t batch, double lr, double beta1, double beta2, double eps, double max_norm, float grad_scale,
                      int32_t grad_rewritten, void *stream);
/* Process-wide switch of the forward / backward launch: 0 (default) = two workgroup roles with the in-launch TD-target hand-off,
 * 1 = every local workgroup runs the target forward itself (no inter-workgroup communication; what batches > 256 always use).
 * Same arithmetic either way: results are bit-identical. */
int mn_iqn_train_set_mode(int32_t mode);

/* Benchmark hook: HIP events on the launch stream around the next act launches of this context (weight / random-number
 * preparation launch included). */
int mn_iqn_profile_begin(mn_iqn_ctx *c, int32_t max_launches);
int mn_iqn_profile_end(mn_iqn_ctx *c, void *stream, double *mean_ms, int32_t *launches);

#ifdef __cplusplus
}
#endif
#endif /* MARINENAV_HIP_H */
