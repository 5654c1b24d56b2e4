// Internal device-side structures shared by the gfx950 kernels and the C-ABI host code.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "marinenav_hip.h"
#include "mn_obs_noise_body.h"

#define MN_WAVE 64
#define MN_PAD 256
#define MN_FIX_SCALE 16777216.0            // 2^24
#define MN_FIX_INV (1.0 / 16777216.0)
#define MN_TAB_ROWS (3 * MN_MAX_CORES + 3 * MN_MAX_OBS)

// Device-resident state.  Everything is struct-of-arrays with the env index fastest, padded to a
// multiple of 64 envs (one wavefront tile), so lane i of a wave touches element base+i of every
// array.  npad is a multiple of 256 so that any lanes-per-env setting fills whole workgroups.
struct MnArrays {
    int32_t n, npad;
    // robot pose (robot.py:40-44); kept in float64 in both precisions
    double *x, *y, *theta, *speed, *vx, *vy;
    // per-env episode constants
    double *start_x, *start_y, *goal_x, *goal_y, *init_theta, *init_speed;
    int32_t *ep_t;    // marinenav_env.py:70 episode_timesteps
    int64_t *tot_t;   // marinenav_env.py:71 total_timesteps
    int32_t *counts;  // placed cores | placed obstacles << 8
    // world tables, [k][npad], generation order (order matters for the sonar `break` quirk)
    double *cx, *cy, *cg;    // cg = +Gamma if clockwise else -Gamma
    double *ox, *oy, *orad;
    // compact copy of the tables read by the mixed-precision step kernel (half the bytes):
    // positions as int32 fixed point (2^-24 m: 6e-8 m resolution everywhere on the 50 m map, where a
    // float32 would have 3.8e-6), signed Gamma and radius as float32.  Written by the reset kernel.
    int32_t *qcx, *qcy, *qox, *qoy;
    float *qcg, *qor;
    // numpy RandomState streams: [n][624] key words + position in the block
    uint32_t *mt;
    int32_t *mt_pos;
    // float64 copy of the observations (parity precision only), [npad][26]
    double *obs64;
    double *rew64;  // float64 copy of the last reward (parity precision only), [npad]
    // per-sub-step positions of the last step, [npad][traj_n][2] (parity precision only, allocated by
    // mn_enable_trajectory): what marinenav_env.py:211-212 appends to robot.trajectory
    double *traj;
    int32_t traj_n;
    // done-queue filled by the step kernel, drained by the reset kernel.  SHARDED: env e pushes into shard (e >> 6) % MN_QSHARDS (wave-uniform for every lanes-per-env
    // mapping), every shard has its own counter on its own 128-byte line -- one counter for all (round 1-5) made a vector step with ~2 000 episode ends 11 us longer:
    // that many returning atomics on ONE address are served one after the other (profiles/r06_done_queue.txt)
    uint32_t *queue_count;  // [2][MN_QSHARDS * MN_QSTRIDE], alternating per step; shard s at word s * MN_QSTRIDE
    int32_t *queue;         // [MN_QSHARDS][qcap]
    int32_t qcap;           // entries per shard = ceil(npad / (64 * MN_QSHARDS)) * 64: every env of the shard can be in it
};
#define MN_QSHARDS 32
#define MN_QSTRIDE 32
#define MN_QWORDS (MN_QSHARDS * MN_QSTRIDE)

// Host-derived constants (computed once in double with the host libm so that the generated world
// tables are bit-identical to the numpy reference).
struct MnDev {
    double width, height, core_r, v_rel_max, p, v_lo, v_span, or_lo, or_span, clear_r, goal_dis;
    double timestep_penalty, collision_penalty, goal_reward;
    double min_start_goal_dis, init_theta, init_speed;
    double dt, robot_r, max_speed, k_drag, a[3], w[3];
    double sonar_range;
    double beam_rel[MN_NUM_BEAMS], beam_cos[MN_NUM_BEAMS], beam_sin[MN_NUM_BEAMS];
    double rot_c[3], rot_s[3];  // cos / sin of w[i]*dt: per-sub-step heading rotation
    double fan_sin, fan_cos;    // sin / cos of half the sonar opening angle (work-list wedge test)
    int32_t fan_filter;         // 1 if the fan is a convex wedge (half angle < 90 deg)
    double two_pi;          // 2*pi as python computes it
    double two_pi_r;        // (2*pi)*r              -> Gamma = two_pi_r * v_edge
    double two_pi_vrel;     // (2*pi)*v_rel_max      -> check_core same-direction boundary
    double inv_two_pi_vrel; // its reciprocal: squared-distance pre-test only (the exact rule divides, like the reference)
    double two_pi_r_r;      // ((2*pi)*r)*r          -> compute_speed inside the core
    double inv_two_pi_r2, inv_two_pi;   // 1 / two_pi_r_r, 1 / two_pi: the IEEE quotients the kernels used to form themselves, per step (wave-uniform, ~26 instructions each)
    double binom_q;         // exp(1*log(1-0.5))     -> binomial(1,.5) == (U > binom_q)
    double sg_lo_x, sg_span_x, sg_lo_y, sg_span_y;  // start/goal uniform: 2 + (w-2-2)*U
    double c_span_x, c_span_y;                      // core centre: 0 + w*U
    double o_lo, o_span_x, o_span_y;                // obstacle centre: 5 + (w-5-5)*U
    double timestep_scale;
    int32_t num_cores, num_obs, reset_start_and_goal, random_reset_state, set_boundary, max_episode_steps, N;
    int32_t n_stages;
    int32_t debug_skip;  // read ONLY by -DMN_ABLATION builds (mn_set_debug_skip): 1 = sub-steps, 2 = sonar scan, 4 = sincos, 8 = obstacle rotation, 16 = beam stores
    int64_t sched_t[MN_MAX_STAGES];
    int32_t sched_nc[MN_MAX_STAGES], sched_no[MN_MAX_STAGES];
    double sched_md[MN_MAX_STAGES];
};

// Replay ring the step kernel appends the transition (obs_t, a_t, r_t, obs_t+1, done_t) to (mn_step_append): the
// layout ReplayBuffer.sample hands to the learner (thirdparty/IQN/replay_buffer.py:49-57).  Env e goes to slot
// (ptr + e - first) mod cap for e >= first = max(0, n - cap) (deque(maxlen) keeps only the newest cap rows).
struct MnRing {
    const float *prev_obs;   // [n][26] observations the actions were chosen from (obs_t)
    float *states, *next_states;   // [cap][26]
    int64_t *actions;        // [cap]
    float *rewards, *dones;  // [cap]
    int64_t ptr, cap;
};

// Snapshot of a handle (mn_state_save / mn_state_load; kernels in mn_state.hip, host side in mn_capi.hip).  The blob is one device buffer:
//   [0, MN_STATE_HEADER_BYTES)   MnStateHeader, zero-filled behind it
//   mt          [n][624] u32     every env's MT19937 row
//   queue_count [2][MN_QWORDS]   both halves of the done-queue's shard counters ...
//   queue       [MN_QSHARDS][qcap] i32   ... and the shard lists (qcap is a function of n)
//                                        CANONICAL in the blob: per shard the live entries ([0, count) of the half the last step filled) in ascending order, zeros
//                                        behind them -- the order the step kernel's waves appended in is wave timing, not state; the blob is a function of the history
//   f64 rows    [MN_STATE_F64_ROWS][n]   x y theta speed vx vy | start_x start_y goal_x goal_y init_theta init_speed | cx cy cg [8] | ox oy orad [10] | tot_t (i64)
//   i32 rows    [MN_STATE_I32_ROWS][n]   ep_t counts mt_pos | qcx qcy qcg [8] | qox qoy qor [10]   (qcg / qor are f32, moved as words)
// Rows are compact over n (the handle pads them to npad); every section starts 8-byte aligned, the MT rows 16-byte aligned; there are no gaps.
#define MN_STATE_MAGIC 0x54534e4du      // "MNST"
#define MN_STATE_VERSION 1
#define MN_STATE_HEADER_BYTES 1024
#define MN_STATE_F64_ROWS (12 + 3 * MN_MAX_CORES + 3 * MN_MAX_OBS + 1)
#define MN_STATE_I32_ROWS (3 + 3 * MN_MAX_CORES + 3 * MN_MAX_OBS)
#define MN_STATE_MT_WORDS 624
struct MnStateHeader {
    uint32_t magic, version;
    int32_t n, precision;
    int64_t bytes;                       // of the whole blob
    int32_t header_bytes, qcap;
    mn_params params;
    // the schedule (mn_set_schedule); its position is a function of each env's tot_t, which the rows carry
    int32_t n_stages, pad0;
    double timestep_scale;
    int64_t sched_t[MN_MAX_STAGES];
    int32_t sched_nc[MN_MAX_STAGES], sched_no[MN_MAX_STAGES];
    double sched_md[MN_MAX_STAGES];
    // the host-side words of mn_handle that later calls depend on (enumerated in mn_capi.hip: state_header)
    int32_t step_parity, last_parity;
    uint32_t tick;
    int32_t under_act_max, owed_max_rows;
    uint32_t has_peak;                   // the handle had its asynchronous-reset pieces (async_ready): peak / seen are its words, else 0 / 0xffffffff
    uint32_t peak, seen;                 // the decaying episode peak: device word and host-mapped copy, read by the save launch in stream order
};
static_assert(sizeof(MnStateHeader) <= MN_STATE_HEADER_BYTES, "MnStateHeader outgrew its slot");
static inline int64_t mn_state_layout_bytes(int64_t n, int64_t qcap) {
    return MN_STATE_HEADER_BYTES + n * MN_STATE_MT_WORDS * 4 + 2 * MN_QWORDS * 4 + MN_QSHARDS * qcap * 4 + MN_STATE_F64_ROWS * n * 8 + MN_STATE_I32_ROWS * n * 4;
}
// one launch: save = handle -> blob (hdr is written in front, with the two peak words read on the device), else blob -> handle (`ready`, if there is one, is
// zeroed: no stale word may equal a tick the restored counter will hand out again; *peak_dev = hdr.peak)
void mn_launch_state(bool save, const MnArrays &A, const MnStateHeader &hdr, void *blob, uint32_t *peak_dev, uint32_t *seen_dev, uint32_t *ready, hipStream_t s);

// kernels (defined in mn_step.hip / mn_reset.hip)
void mn_launch_step(const MnArrays &A, const MnDev &P, int precision, int lanes, const int32_t *actions, float *obs,
                    float *reward, uint8_t *done, uint8_t *info, int parity, const MnRing *ring, hipStream_t s);
void mn_launch_rollout(const MnArrays &A, const MnDev &P, int precision, int lanes, int n_steps, const int32_t *actions_in,
                       uint64_t seed, uint64_t step0, uint64_t env0, float *obs_out, float *obs_trace, float *reward_trace,
                       uint8_t *done_trace, uint8_t *info_trace, int32_t *action_trace, hipStream_t s);
// observation noise on a vector of rows (mn_obs_noise.hip): the arguments of mn_obs_perturb, validated
void mn_launch_obs_perturb(const float *obs_in, float *obs_out, int64_t n, uint64_t env_index0, const int32_t *ep_t, const MnObsNoiseDev &S, hipStream_t s);
void mn_launch_random_actions(uint64_t seed, uint64_t step, uint64_t env0, int n, int32_t *out, hipStream_t s);
// episodes under a device-side policy (MN_POLICY_APF / MN_POLICY_BA, mn_planners.h), and one policy step for a vector of observations
void mn_launch_rollout_policy(const MnArrays &A, const MnDev &P, int precision, int n_steps, int policy, float *obs_io, float *obs_trace,
                              float *reward_trace, uint8_t *done_trace, uint8_t *info_trace, int32_t *action_trace, double *traj_trace, hipStream_t s,
                              const MnObsNoiseDev *noise = nullptr, uint64_t noise_env0 = 0);
void mn_launch_planner_act(const float *obs, int n, int policy, const double *a, const double *w, int32_t *actions, hipStream_t s);
// IQN evaluation episodes in one launch (mn_rollout_iqn.hip); `image` / `words` from mn_iqn_rollout_image (iqn_act.hip)
// cvar_row / adaptive_row: per-env cvar / adaptive flags ([n] device arrays; NULL = the scalar)
// noise (here and in the policy / DQN launches): NULL = the policy reads the clean row (the kernels as they were); else the NOISE instantiation, which feeds
// it mn_obs_noise_channel of the row under the key (noise->seed, noise_env0 + env, the env's episode_timesteps)
// traj_trace (here and in the policy / DQN launches): [n_steps][n][P.N][2] sub-step positions (mn_set_trajectory_trace), or NULL
void mn_launch_rollout_iqn_rows(const MnArrays &A, const MnDev &P, int precision, int n_steps, const uint32_t *image, uint64_t *rng_state, float cvar,
                                int adaptive, const float *cvar_row, const uint8_t *adaptive_row, float *obs_io, float *obs_trace, float *reward_trace,
                                uint8_t *done_trace, uint8_t *info_trace, int32_t *action_trace, float *cvar_trace, float *q_trace, double *traj_trace,
                                uint32_t *words, int32_t *steps_run, hipStream_t s, const MnObsNoiseDev *noise = nullptr, uint64_t noise_env0 = 0);
// the same episodes acting as act_eval does, with the quantile / tau traces (mn_rollout_iqn_eval.hip)
void mn_launch_rollout_iqn_eval(const MnArrays &A, const MnDev &P, int precision, int n_steps, const uint32_t *image, uint64_t *rng_state, float cvar,
                                int adaptive, const float *cvar_row, const uint8_t *adaptive_row, float *obs_io, float *obs_trace, float *reward_trace,
                                uint8_t *done_trace, uint8_t *info_trace, int32_t *action_trace, float *cvar_trace, float *q_trace, double *traj_trace,
                                float *quantiles_trace, float *taus_trace, uint32_t *words, int32_t *steps_run, hipStream_t s);
// the acting episodes with a weight image and a tau stream per group of rows (mn_rollout_iqn_groups.hip); image_stride in 32-bit words
void mn_launch_rollout_iqn_groups(const MnArrays &A, const MnDev &P, int precision, int n_steps, const uint32_t *images, int64_t image_stride,
                                  int rows_per_group, uint64_t *rng_states, const float *cvar_row, const uint8_t *adaptive_row, float *obs_io,
                                  float *obs_trace, float *reward_trace, uint8_t *done_trace, uint8_t *info_trace, int32_t *action_trace, float *cvar_trace,
                                  float *q_trace, uint32_t *group_words, int32_t *steps_run, hipStream_t s);
int mn_iqn_rollout_image(mn_iqn_ctx *c, const float *const *weights, hipStream_t s, const uint32_t **image, uint32_t **words);
// DQN evaluation episodes in one launch (mn_rollout_dqn.hip); `image` = the weight image mn_launch_dqn_pack (dqn_act.hip) builds from weights[18]
void mn_launch_dqn_pack(const float *const *weights, float *image_dev, hipStream_t s);
void mn_launch_rollout_dqn(const MnArrays &A, const MnDev &P, int precision, int n_steps, const float *image, float *obs_io, float *obs_trace,
                           float *reward_trace, uint8_t *done_trace, uint8_t *info_trace, int32_t *action_trace, float *q_trace, double *traj_trace, hipStream_t s,
                           const MnObsNoiseDev *noise = nullptr, uint64_t noise_env0 = 0);
// the same episodes with a weight image per group of rows (mn_rollout_dqn_groups.hip); image_stride in floats
void mn_launch_rollout_dqn_groups(const MnArrays &A, const MnDev &P, int precision, int n_steps, const float *images, int64_t image_stride, int n_groups,
                                  int rows_per_group, float *obs_io, float *obs_trace, float *reward_trace, uint8_t *done_trace, uint8_t *info_trace,
                                  int32_t *action_trace, float *q_trace, hipStream_t s);
// mode 0: full reset (RNG); mode 1: pose-only (keeps the loaded world, no RNG)
// (mn_launch_reset: `sharded` = count_dev / list_dev are the handle's done-queue of one step -- MN_QSHARDS counters and lists; otherwise one counter, one list)
void mn_launch_reset_under_act(const MnArrays &A, const MnDev &P, int precision, const uint32_t *count_dev, const int32_t *list_dev, float *obs,
                               uint32_t *ready, uint32_t tick, uint32_t *peak_dev, uint32_t *peak_host, hipStream_t s);
void mn_launch_reset(const MnArrays &A, const MnDev &P, int precision, const uint32_t *count_dev, uint32_t count_host,
                     const int32_t *list_dev, int mode, float *obs, hipStream_t s, uint32_t *peak_dev = nullptr, uint32_t *peak_host = nullptr, bool sharded = false);
// The resets of the last step and the preparation of the next act call in one launch (mn_prep_reset.hip; mn_iqn_act_rng_env).  MnOwedReset: the handle's
// side -- what mn_launch_reset would be given, `blocks` reset wavefronts (mn_prep_reset_blocks); MnPrepLaunch: the act context's side -- what the
// preparation launch of mn_iqn_act_rng would be given (`pack`: the weight image is stale; rows_words NULL: every row goes through the network).
#define MN_PREP_RESET_MIN_BLOCKS 256
#define MN_PREP_RESET_MAX_BLOCKS 8192
struct MnOwedReset {
    const MnArrays *A;
    const MnArrays *A_mem;            // the handle's DEVICE copy of *A (mn_reset_env's TAIL_MEM)
    const MnDev *P;
    int precision;
    const uint32_t *count_dev;
    const int32_t *list;
    float *obs;
    uint32_t *peak_dev, *peak_host;
    int blocks;
    hipEvent_t ev_begin, ev_end;      // the handle's profiling pair for this reset (mn_profile_begin .. mn_profile_reset_end), or NULL: recorded around the launch
};
struct MnPrepLaunch {
    const float *const *weights;      // the 14 pointers of the C ABI
    const float *consts;
    uint32_t *packed;
    bool pack;
    const uint64_t *rng_state;
    float *draws;
    int n;
    const float *cvar_row;
    float cvar, eps;
    int32_t *actions;
    int32_t *rows_list;
    uint32_t *rows_words;
    int max_draw_blocks;              // of 64 threads
};
int mn_prep_reset_blocks(uint32_t seen, int n);
void mn_launch_prep_reset(const MnOwedReset &o, const MnPrepLaunch &p, hipStream_t s);
// the handle's owed reset (mn_capi.hip; mn_reset_done_next_act), for the act launch that takes it: mn_owed_reset_take fills *out and clears the debt (1), or
// returns 0 when nothing is owed -- or the handle lives on another device, which the settling call then reports; mn_owed_reset_settle launches it on `s`
bool mn_owed_reset_take(mn_handle *h, hipStream_t s, MnOwedReset *out);
int mn_owed_reset_settle(mn_handle *h, hipStream_t s);
void mn_launch_seed(const MnArrays &A, const uint32_t *seeds_dev, hipStream_t s);
void mn_launch_mask_to_queue(const MnArrays &A, const uint8_t *mask, uint32_t *count, int32_t *list, hipStream_t s);
void mn_launch_peek(const MnArrays &A, int first, int count, double *out_dev, hipStream_t s);
void mn_launch_sleep(uint32_t us, hipStream_t s);
// queries (mn_query.hip): read-only on A; env_of = NULL: every query in world env0
void mn_launch_query_velocity(const MnArrays &A, const MnDev &P, const int32_t *env_of, int env0, const double *xy, int64_t nq, double *v, hipStream_t s);
void mn_launch_query_observation(const MnArrays &A, const MnDev &P, const int32_t *env_of, int env0, const double *state, int from_current, int64_t nq,
                                 float *obs, double *obs64, uint8_t *flags, hipStream_t s);
// what-if steps / open-loop rollouts (mn_query_step.hip): read-only on A; the arguments of mn_query_rollout
void mn_launch_query_rollout(const MnArrays &A, const MnDev &P, const int32_t *env_of, int env0, const double *state, const int32_t *ep_t, int action_mode,
                             const int32_t *actions, int n_steps, const int32_t *n_steps_of, int64_t nq, double *state_out, float *obs, double *obs64,
                             double *reward, uint8_t *done, uint8_t *info, int32_t *steps, double *reward_tr, uint8_t *done_tr, uint8_t *info_tr,
                             int32_t *action_tr, double *state_tr, double *traj_tr, hipStream_t s);
// minimum-time-to-goal fields (mn_time_field.hip): read-only on A; the arguments of mn_time_field, validated.  MN_OK or MN_ERR_HIP
int64_t mn_time_field_planes_bytes(int nx, int ny, int64_t n_fields);
int mn_launch_time_field(const MnArrays &A, const MnDev &P, const int32_t *env_of, int env0, const double *goal_xy, int64_t n_fields, int nx, int ny,
                         double speed, double clearance, int max_sweeps, double *T, uint8_t *dir, int32_t *status, int32_t *sweeps, void *workspace,
                         hipStream_t s);
// the field pilot (mn_pilot.hip): mn_pilot_act is read-only on A, mn_rollout_pilot steps the envs; the arguments of the entry points, validated
void mn_launch_pilot_act(const MnArrays &A, const MnDev &P, const int32_t *env_of, int env0, const double *state, const int32_t *ep_t, const double *T,
                         const int32_t *field_of, int64_t n_fields, int nx, int ny, int horizon, int64_t nq, int32_t *actions, double *scores,
                         int32_t *steps, uint8_t *infos, uint8_t *flags, hipStream_t s);
void mn_launch_rollout_pilot(const MnArrays &A, const MnDev &P, int n_steps, const double *T, const int32_t *field_of, int64_t n_fields, int nx, int ny,
                             int horizon, float *obs_io, float *obs_trace, float *reward_trace, uint8_t *done_trace, uint8_t *info_trace,
                             int32_t *action_trace, double *traj_trace, hipStream_t s);
// pictures (mn_render.hip): read-only on A; env_of = NULL: every image shows world env0.  The arguments of mn_render_worlds / mn_render_draw, validated
void mn_launch_render_worlds(const MnArrays &A, const MnDev &P, const int32_t *env_of, int env0, int n_images, int width, int height, const double view[4],
                             const mn_render_style &style, uint32_t *pixels, hipStream_t s);
void mn_launch_render_draw(uint32_t *pixels, int n_images, int width, int height, const double view[4], const mn_render_prim *prims, int64_t n_prims,
                           hipStream_t s);
