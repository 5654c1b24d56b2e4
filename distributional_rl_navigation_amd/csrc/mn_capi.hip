// mn_capi.hip -- C-ABI host side of libmarinenav_hip.so (see include/marinenav_hip.h).
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "mn_internal.h"
#include "mn_render_font.h"

struct mn_handle {
    MnArrays A;
    MnDev P;
    mn_params params;
    std::vector<void *> allocs;
    std::string err;
    int step_parity = 0;  // queue counter the NEXT step will fill
    int last_parity = 0;  // queue counter the LAST step filled
    uint32_t *seeds_dev = nullptr;
    uint32_t *mask_count = nullptr;
    int32_t *list_scratch = nullptr;
    double *peek_scratch = nullptr;
    double *obs64_buf = nullptr, *rew64_buf = nullptr;      // mn_enable_obs64: A.obs64 / A.rew64 point here while enabled
    MnArrays *A_mem = nullptr;                              // device copy of A (sync_arrays): the preparation launch's reset blocks read their store pointers from it
    double *traj_trace = nullptr;                           // mn_set_trajectory_trace: the caller's [traj_trace_steps][n][N][2] buffer, until the next episode launch takes it
    int32_t traj_trace_steps = 0, traj_trace_sub = 0;
    // mn_set_obs_noise: the attached description in the kernels' form and the handle's first_env_index; stays until replaced or detached
    bool noise_on = false;                                  // attached AND not all-zero: the episode launches take their NOISE instantiation
    bool noise_attached = false;
    MnObsNoiseDev noise = {};
    uint64_t noise_env0 = 0;
    int device = -1;      // HIP device the handle's memory lives on (the caller's current device at mn_create)
    // profiling
    std::vector<hipEvent_t> ev;
    int prof_max = 0, prof_n = 0;
    std::vector<hipEvent_t> ev_reset;      // ... and around mn_reset_done (mn_profile_reset_end)
    int prof_reset_n = 0;
    // mn_reset_done_async: the reset launch on the handle's own stream, under the caller's next act kernel
    hipStream_t side = nullptr;
    hipEvent_t ev_stepped = nullptr, ev_reset_end = nullptr;
    uint32_t *ready = nullptr;             // [n] "first observation is final" words (value = tick of the reset that wrote it)
    uint32_t tick = 0;
    bool reset_pending = false;            // a reset launched by mn_reset_done_async has not been joined by the caller's stream yet
    // decaying peak of the episodes the queue-driven reset launches start (mn_reset.hip: mn_note_count): device word + host-mapped copy (read without synchronising)
    volatile uint32_t *seen_host = nullptr;
    uint32_t *seen_dev = nullptr, *peak_dev = nullptr;
    int32_t under_act_max = MN_RESET_UNDER_ACT_MAX_DEFAULT;      // mn_reset_done_async: above this peak the reset runs in front of the act kernel
    bool async_ready = false;              // side stream, events, `ready`, the peak words: all there
    int32_t side_delay_us = 0;             // mn_debug_side_delay_us (tests): a sleeping kernel in front of every reset launch on the side stream
    // mn_reset_done_next_act: the last step's finished envs await their reset -- the next act call's preparation launch runs it (mn_iqn_act_rng_env), or
    // whichever entry point touches the handle's state first settles it (settle_owed)
    bool reset_owed = false;
    float *owed_obs = nullptr;
    hipStream_t owed_stream = nullptr;     // the stream the step ran on
    int32_t owed_max_rows = MN_RESET_OWED_MAX_ROWS_DEFAULT;      // mn_set_reset_owed_max_rows
};

#define MT_WORDS 624      // one env's MT19937 row (mn_reset_body.h: MT_N)
static thread_local std::string g_create_err;

#define MN_HIP(h, call)                                                                                     \
    do {                                                                                                    \
        hipError_t _e = (call);                                                                             \
        if (_e != hipSuccess) {                                                                             \
            char _b[512];                                                                                   \
            snprintf(_b, sizeof(_b), "%s failed: %s (%s:%d)", #call, hipGetErrorString(_e), __FILE__, __LINE__); \
            if (h) (h)->err = _b; else g_create_err = _b;                                                   \
            return MN_ERR_HIP;                                                                              \
        }                                                                                                   \
    } while (0)

static int fail(mn_handle *h, int code, const char *msg) {
    if (h) h->err = msg; else g_create_err = msg;
    return code;
}

// mn_reset_done's launch: the queue-driven reset of the last step's finished envs on `s`, inside the profiling window's event pairs
static void launch_reset_done(mn_handle *h, float *obs_dev, hipStream_t s) {
    const bool prof = h->prof_reset_n < h->prof_max;
    if (prof) (void)hipEventRecord(h->ev_reset[2 * h->prof_reset_n], s);
    mn_launch_reset(h->A, h->P, h->params.precision, h->A.queue_count + h->last_parity * MN_QWORDS, 0, h->A.queue, 0, obs_dev, s, h->peak_dev, h->seen_dev, true);
    if (prof) { (void)hipEventRecord(h->ev_reset[2 * h->prof_reset_n + 1], s); h->prof_reset_n++; }
}
// An owed reset (mn_reset_done_next_act) as a plain reset launch on `s`.  The ONE place a debt is paid outside the act call that was meant to take it:
// join_reset and on_device call it, and through them every entry point that reads or writes the handle's state.
static void settle_owed(mn_handle *h, hipStream_t s) {
    if (!h->reset_owed) return;
    if (s != h->owed_stream) (void)hipStreamSynchronize(h->owed_stream);      // (another stream than the step's: nothing orders the two)
    launch_reset_done(h, h->owed_obs, s);
    h->reset_owed = false;
}

// Every entry point that touches device memory runs on the device the handle was created on: a caller that has
// switched devices since (one process driving several GPUs) gets an error instead of a fault on a foreign pointer.
static int on_device(mn_handle *h) {
    if (!h) return MN_ERR_INVALID;
    int cur = -1;
    if (hipGetDevice(&cur) != hipSuccess) return fail(h, MN_ERR_HIP, "hipGetDevice failed");
    if (cur != h->device) {
        char b[160];
        snprintf(b, sizeof(b), "handle lives on HIP device %d but the calling thread's current device is %d", h->device, cur);
        return fail(h, MN_ERR_INVALID, b);
    }
    // an asynchronous reset (mn_reset_done_async) that the caller's stream has not joined: whatever this entry point is about to do with the
    // handle's state must come after it.  The per-step entry points join on their stream (join_reset) before they get here; the others wait on the host.
    if (h->reset_pending) {
        if (hipEventSynchronize(h->ev_reset_end) != hipSuccess) return fail(h, MN_ERR_HIP, "waiting for the asynchronous reset failed");
        h->reset_pending = false;
    }
    // ... and an owed one (mn_reset_done_next_act) that no act call has taken: launched now, on the stream its step ran on, and waited for
    if (h->reset_owed) {
        const hipStream_t s = h->owed_stream;
        settle_owed(h, s);
        if (hipStreamSynchronize(s) != hipSuccess) return fail(h, MN_ERR_HIP, "waiting for the owed reset failed");
    }
    return MN_OK;
}
// stream-side join: everything enqueued on `s` from here on runs after the asynchronous reset, and after an owed one, which is launched here
static void join_reset(mn_handle *h, hipStream_t s) {
    if (!h) return;
    if (h->reset_owed) {
        int cur = -1;
        if (hipGetDevice(&cur) == hipSuccess && cur == h->device) settle_owed(h, s);      // (a foreign device: on_device reports it, nothing was launched)
    }
    if (h->reset_pending) {
        if (hipStreamWaitEvent(s, h->ev_reset_end, 0) == hipSuccess) h->reset_pending = false;
    }
}
#define MN_ON_DEVICE(h) do { int _rc = on_device(h); if (_rc) return _rc; } while (0)

extern "C" int mn_default_params(mn_params *p) {
    if (!p) return MN_ERR_INVALID;
    memset(p, 0, sizeof(*p));
    p->width = 50; p->height = 50; p->core_r = 0.5; p->v_rel_max = 1.0; p->p = 0.8;
    p->v_range[0] = 5; p->v_range[1] = 10; p->obs_r_range[0] = 1; p->obs_r_range[1] = 3;
    p->clear_r = 10.0; p->goal_dis = 2.0; p->timestep_penalty = -1.0; p->collision_penalty = -50.0;
    p->goal_reward = 100.0; p->discount = 0.99; p->min_start_goal_dis = 25.0;
    p->init_theta = M_PI / 4; p->init_speed = 0.0;
    p->dt = 0.1; p->robot_r = 0.8; p->max_speed = 2.0;
    p->a[0] = -0.4; p->a[1] = 0.0; p->a[2] = 0.4;
    p->w[0] = -M_PI / 6; p->w[1] = 0.0; p->w[2] = M_PI / 6;
    p->sonar_range = 10.0; p->sonar_angle = 2 * M_PI / 3;
    p->num_cores = 8; p->num_obs = 5; p->reset_start_and_goal = 1; p->random_reset_state = 1;
    p->set_boundary = 0; p->max_episode_steps = 1000; p->N = 10; p->num_beams = MN_NUM_BEAMS;
    p->precision = MN_PRECISION_MIXED;
    return MN_OK;
}

// Host-side constants, evaluated in the reference's (python) expression order.
static int derive(mn_handle *h, const mn_params &p) {
    const int32_t keep_skip = h->P.debug_skip;   // only ever non-zero in -DMN_ABLATION builds (mn_set_debug_skip)
    if (p.num_beams != MN_NUM_BEAMS) return fail(h, MN_ERR_INVALID, "num_beams must be 11");
    if (p.num_cores < 0 || p.num_cores > MN_MAX_CORES) return fail(h, MN_ERR_INVALID, "num_cores out of [0, 8]");
    if (p.num_obs < 0 || p.num_obs > MN_MAX_OBS) return fail(h, MN_ERR_INVALID, "num_obs out of [0, 10]");
    if (p.N < 1 || p.N > 1000) return fail(h, MN_ERR_INVALID, "robot N out of range");
    if (p.precision != MN_PRECISION_F64 && p.precision != MN_PRECISION_MIXED) return fail(h, MN_ERR_INVALID, "bad precision");
    if (p.step_lanes != 0 && p.step_lanes != 1 && p.step_lanes != 2 && p.step_lanes != 4 && p.step_lanes != 8) return fail(h, MN_ERR_INVALID, "step_lanes must be 0 (default), 1, 2, 4 or 8");
    if (p.rollout_lanes != 0 && p.rollout_lanes != 2 && p.rollout_lanes != 4 && p.rollout_lanes != 8 && p.rollout_lanes != 16) return fail(h, MN_ERR_INVALID, "rollout_lanes must be 0 (default), 2, 4, 8 or 16");
    MnDev &d = h->P;
    const int32_t keep_n = d.n_stages;
    d.width = p.width; d.height = p.height; d.core_r = p.core_r; d.v_rel_max = p.v_rel_max; d.p = p.p;
    d.v_lo = p.v_range[0]; d.v_span = p.v_range[1] - p.v_range[0];
    d.or_lo = p.obs_r_range[0]; d.or_span = p.obs_r_range[1] - p.obs_r_range[0];
    d.clear_r = p.clear_r; d.goal_dis = p.goal_dis;
    d.timestep_penalty = p.timestep_penalty; d.collision_penalty = p.collision_penalty; d.goal_reward = p.goal_reward;
    d.min_start_goal_dis = p.min_start_goal_dis; d.init_theta = p.init_theta; d.init_speed = p.init_speed;
    d.dt = p.dt; d.robot_r = p.robot_r; d.max_speed = p.max_speed;
    double amax = p.a[0];
    for (int i = 0; i < 3; ++i) {
        d.a[i] = p.a[i]; d.w[i] = p.w[i]; if (p.a[i] > amax) amax = p.a[i];
        d.rot_c[i] = cos(p.w[i] * p.dt); d.rot_s[i] = sin(p.w[i] * p.dt);
    }
    d.k_drag = amax / p.max_speed;  // robot.py:52
    d.sonar_range = p.sonar_range;
    const double phi = p.sonar_angle / (p.num_beams - 1);  // robot.py:14-21
    const double a0 = -p.sonar_angle / 2;
    for (int i = 0; i < MN_NUM_BEAMS; ++i) {
        d.beam_rel[i] = a0 + i * phi;
        d.beam_cos[i] = cos(d.beam_rel[i]);
        d.beam_sin[i] = sin(d.beam_rel[i]);
    }
    d.fan_sin = sin(p.sonar_angle / 2); d.fan_cos = cos(p.sonar_angle / 2);
    d.fan_filter = (p.sonar_angle / 2 < 0.49 * M_PI) ? 1 : 0;
    d.two_pi = 2 * M_PI;
    d.two_pi_r = 2 * M_PI * p.core_r;
    d.two_pi_vrel = 2 * M_PI * p.v_rel_max;
    d.inv_two_pi_vrel = 1.0 / d.two_pi_vrel;
    d.two_pi_r_r = 2 * M_PI * p.core_r * p.core_r;
    d.inv_two_pi_r2 = 1.0 / d.two_pi_r_r;      // plain float64 divisions: the correctly rounded quotients a kernel's `1.0 / P.two_pi_r_r` gives
    d.inv_two_pi = 1.0 / d.two_pi;
    d.binom_q = exp(1.0 * log(1.0 - 0.5));
    d.sg_lo_x = 2.0; d.sg_span_x = (p.width - 2.0) - 2.0; d.sg_lo_y = 2.0; d.sg_span_y = (p.height - 2.0) - 2.0;
    d.c_span_x = p.width - 0.0; d.c_span_y = p.height - 0.0;
    d.o_lo = 5.0; d.o_span_x = (p.width - 5.0) - 5.0; d.o_span_y = (p.height - 5.0) - 5.0;
    d.num_cores = p.num_cores; d.num_obs = p.num_obs; d.reset_start_and_goal = p.reset_start_and_goal;
    d.random_reset_state = p.random_reset_state; d.set_boundary = p.set_boundary;
    d.max_episode_steps = p.max_episode_steps; d.N = p.N;
    d.n_stages = keep_n;
    d.debug_skip = keep_skip;
    h->params = p;
    return MN_OK;
}

template <typename T>
static int dev_alloc(mn_handle *h, T **out, size_t count, bool zero = true) {
    void *p = nullptr;
    hipError_t e = hipMalloc(&p, count * sizeof(T));
    if (e != hipSuccess) { h->err = std::string("hipMalloc failed: ") + hipGetErrorString(e); return MN_ERR_ALLOC; }
    if (zero) { e = hipMemset(p, 0, count * sizeof(T)); if (e != hipSuccess) { h->err = hipGetErrorString(e); return MN_ERR_HIP; } }
    h->allocs.push_back(p);
    *out = (T *)p;
    return MN_OK;
}

// h->A as the device sees it (MnOwedReset::A_mem; mn_reset_env's TAIL_MEM): rewritten wherever a pointer of A changes.  The callers have synchronised the device.
static int sync_arrays(mn_handle *h) {
    if (!h->A_mem) {
        const int rc = dev_alloc(h, &h->A_mem, 1, false);
        if (rc) return rc;
    }
    MN_HIP(h, hipMemcpy(h->A_mem, &h->A, sizeof(MnArrays), hipMemcpyHostToDevice));
    return MN_OK;
}

extern "C" int mn_destroy(mn_handle *h) {
    if (!h) return MN_ERR_INVALID;
    int cur = -1;
    const bool moved = hipGetDevice(&cur) == hipSuccess && h->device >= 0 && cur != h->device;
    if (moved) (void)hipSetDevice(h->device);   // free on the owning device, then restore the caller's
    if (h->reset_owed) { const hipStream_t s = h->owed_stream; settle_owed(h, s); (void)hipStreamSynchronize(s); }      // the caller's obs buffer gets its rows
    for (hipEvent_t e : h->ev) (void)hipEventDestroy(e);
    for (hipEvent_t e : h->ev_reset) (void)hipEventDestroy(e);
    if (h->side) { (void)hipStreamSynchronize(h->side); (void)hipStreamDestroy(h->side); }
    if (h->ev_stepped) (void)hipEventDestroy(h->ev_stepped);
    if (h->ev_reset_end) (void)hipEventDestroy(h->ev_reset_end);
    if (h->seen_host) (void)hipHostFree((void *)h->seen_host);
    for (void *p : h->allocs) (void)hipFree(p);
    if (moved) (void)hipSetDevice(cur);
    delete h;
    return MN_OK;
}

extern "C" int mn_create(int32_t n_envs, const mn_params *p, mn_handle **out) {
    if (!out || !p || n_envs <= 0) return fail(nullptr, MN_ERR_INVALID, "mn_create: bad arguments");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(nullptr, MN_ERR_NO_DEVICE, "no HIP device visible");
    mn_handle *h = new mn_handle();
    if (hipGetDevice(&h->device) != hipSuccess) { delete h; return fail(nullptr, MN_ERR_HIP, "hipGetDevice failed"); }
    memset(&h->A, 0, sizeof(h->A));
    memset(&h->P, 0, sizeof(h->P));
    h->P.timestep_scale = 1.0;
    h->params.precision = p->precision;
    int rc = derive(h, *p);
    if (rc) { g_create_err = h->err; delete h; return rc; }
    MnArrays &A = h->A;
    A.n = n_envs;
    A.npad = (n_envs + MN_PAD - 1) / MN_PAD * MN_PAD;
    const size_t np = (size_t)A.npad;
#define ALLOC(field, count)                                    \
    if ((rc = dev_alloc(h, &A.field, (count))) != MN_OK) {      \
        g_create_err = h->err;                                 \
        mn_destroy(h);                                         \
        return rc;                                             \
    }
    ALLOC(x, np) ALLOC(y, np) ALLOC(theta, np) ALLOC(speed, np) ALLOC(vx, np) ALLOC(vy, np)
    ALLOC(start_x, np) ALLOC(start_y, np) ALLOC(goal_x, np) ALLOC(goal_y, np) ALLOC(init_theta, np) ALLOC(init_speed, np)
    ALLOC(ep_t, np) ALLOC(tot_t, np) ALLOC(counts, np)
    ALLOC(cx, np * MN_MAX_CORES) ALLOC(cy, np * MN_MAX_CORES) ALLOC(cg, np * MN_MAX_CORES)
    ALLOC(ox, np * MN_MAX_OBS) ALLOC(oy, np * MN_MAX_OBS) ALLOC(orad, np * MN_MAX_OBS)
    ALLOC(qcx, np * MN_MAX_CORES) ALLOC(qcy, np * MN_MAX_CORES) ALLOC(qcg, np * MN_MAX_CORES)
    ALLOC(qox, np * MN_MAX_OBS) ALLOC(qoy, np * MN_MAX_OBS) ALLOC(qor, np * MN_MAX_OBS)
    ALLOC(mt, np * 624) ALLOC(mt_pos, np)
    A.qcap = (int32_t)(((np >> 6) + MN_QSHARDS - 1) / MN_QSHARDS * 64);
    ALLOC(queue_count, 2 * MN_QWORDS) ALLOC(queue, (size_t)MN_QSHARDS * A.qcap)
    // (obs64 / rew64 -- float64 copies of the last observation rows / rewards -- are allocated and written only after mn_enable_obs64)
#undef ALLOC
    if ((rc = dev_alloc(h, &h->seeds_dev, np)) || (rc = dev_alloc(h, &h->mask_count, 1)) ||
        (rc = dev_alloc(h, &h->list_scratch, np)) || (rc = dev_alloc(h, &h->peek_scratch, np))) {
        g_create_err = h->err; mn_destroy(h); return rc;
    }
    // default start / goal (marinenav_env.py:49,53) and default seeds 0..n-1
    {
        std::vector<double> v(np);
        for (size_t i = 0; i < np; ++i) v[i] = 5.0;
        (void)hipMemcpy(A.start_x, v.data(), np * 8, hipMemcpyHostToDevice);
        (void)hipMemcpy(A.start_y, v.data(), np * 8, hipMemcpyHostToDevice);
        for (size_t i = 0; i < np; ++i) v[i] = 45.0;
        (void)hipMemcpy(A.goal_x, v.data(), np * 8, hipMemcpyHostToDevice);
        (void)hipMemcpy(A.goal_y, v.data(), np * 8, hipMemcpyHostToDevice);
        std::vector<uint32_t> s(np);
        for (size_t i = 0; i < np; ++i) s[i] = (uint32_t)i;
        rc = mn_seed(h, s.data(), nullptr);
        if (rc) { g_create_err = h->err; mn_destroy(h); return rc; }
        hipError_t e = hipDeviceSynchronize();
        if (e != hipSuccess) { g_create_err = hipGetErrorString(e); mn_destroy(h); return MN_ERR_HIP; }
    }
    if ((rc = sync_arrays(h)) != MN_OK) { g_create_err = h->err; mn_destroy(h); return rc; }
    *out = h;
    return MN_OK;
}

extern "C" const char *mn_last_error(const mn_handle *h) { return h ? h->err.c_str() : g_create_err.c_str(); }
extern "C" int32_t mn_num_envs(const mn_handle *h) { return h ? h->A.n : 0; }

extern "C" int mn_set_params(mn_handle *h, const mn_params *p) {
    if (!h || !p) return MN_ERR_INVALID;
    if (p->precision != h->params.precision) return fail(h, MN_ERR_INVALID, "precision is fixed at mn_create");
    if (h->reset_owed) MN_ON_DEVICE(h);      // an owed reset runs with the parameters of its step
    return derive(h, *p);
}

extern "C" int mn_get_params(const mn_handle *h, mn_params *p) {
    if (!h || !p) return MN_ERR_INVALID;
    *p = h->params;
    return MN_OK;
}

extern "C" int mn_seed(mn_handle *h, const uint32_t *seeds_host, void *stream) {
    if (!h || !seeds_host) return MN_ERR_INVALID;
    MN_ON_DEVICE(h);
    hipStream_t s = (hipStream_t)stream;
    MN_HIP(h, hipMemcpyAsync(h->seeds_dev, seeds_host, (size_t)h->A.n * 4, hipMemcpyHostToDevice, s));
    mn_launch_seed(h->A, h->seeds_dev, s);
    MN_HIP(h, hipGetLastError());
    MN_HIP(h, hipStreamSynchronize(s));  // seeds_host may be freed by the caller
    return MN_OK;
}

extern "C" int mn_set_schedule(mn_handle *h, int32_t n, const int64_t *ts, const int32_t *nc, const int32_t *no,
                               const double *md, double timestep_scale) {
    if (!h || n < 0 || n > MN_MAX_STAGES) return fail(h, MN_ERR_INVALID, "schedule: 0..8 stages");
    if (n > 0 && (!ts || !nc || !no || !md)) return MN_ERR_INVALID;
    if (h->reset_owed) MN_ON_DEVICE(h);      // an owed reset runs with the schedule of its step
    for (int i = 0; i < n; ++i) {
        if (nc[i] < 0 || nc[i] > MN_MAX_CORES || no[i] < 0 || no[i] > MN_MAX_OBS) return fail(h, MN_ERR_INVALID, "schedule world size exceeds capacity (8 cores, 10 obstacles)");
        h->P.sched_t[i] = ts[i]; h->P.sched_nc[i] = nc[i]; h->P.sched_no[i] = no[i]; h->P.sched_md[i] = md[i];
    }
    h->P.n_stages = n;
    h->P.timestep_scale = timestep_scale > 0 ? timestep_scale : 1.0;
    return MN_OK;
}

static int range_ok(mn_handle *h, int first, int count) {
    if (!h || first < 0 || count < 0 || first + count > h->A.n) return fail(h, MN_ERR_INVALID, "env range out of bounds");
    return on_device(h);
}

extern "C" int mn_set_start_goal(mn_handle *h, int32_t env_idx, const double start[2], const double goal[2]) {
    if (!h || !start || !goal || env_idx >= h->A.n) return MN_ERR_INVALID;
    MN_ON_DEVICE(h);
    const int first = env_idx < 0 ? 0 : env_idx, count = env_idx < 0 ? h->A.n : 1;
    std::vector<double> v(count);
    double *dst[4] = {h->A.start_x, h->A.start_y, h->A.goal_x, h->A.goal_y};
    const double val[4] = {start[0], start[1], goal[0], goal[1]};
    for (int k = 0; k < 4; ++k) {
        for (int i = 0; i < count; ++i) v[i] = val[k];
        MN_HIP(h, hipMemcpy(dst[k] + first, v.data(), (size_t)count * 8, hipMemcpyHostToDevice));
    }
    return MN_OK;
}

extern "C" int mn_reset(mn_handle *h, const uint8_t *mask_dev, float *obs_dev, void *stream) {
    if (!h || !obs_dev) return MN_ERR_INVALID;
    MN_ON_DEVICE(h);
    hipStream_t s = (hipStream_t)stream;
    if (!mask_dev) {
        mn_launch_reset(h->A, h->P, h->params.precision, nullptr, (uint32_t)h->A.n, nullptr, 0, obs_dev, s);
    } else {
        MN_HIP(h, hipMemsetAsync(h->mask_count, 0, 4, s));
        mn_launch_mask_to_queue(h->A, mask_dev, h->mask_count, h->list_scratch, s);
        mn_launch_reset(h->A, h->P, h->params.precision, h->mask_count, 0, h->list_scratch, 0, obs_dev, s);
    }
    MN_HIP(h, hipGetLastError());
    return MN_OK;
}

static int step_common(mn_handle *h, const int32_t *actions_dev, float *obs_dev, float *reward_dev, uint8_t *done_dev,
                       uint8_t *info_dev, const MnRing *ring, void *stream) {
    if (!h || !actions_dev || !obs_dev || !reward_dev || !done_dev || !info_dev) return MN_ERR_INVALID;
    hipStream_t s = (hipStream_t)stream;
    join_reset(h, s);
    MN_ON_DEVICE(h);
    const int parity = h->step_parity;
    const bool prof = h->prof_n < h->prof_max;
    if (prof) (void)hipEventRecord(h->ev[2 * h->prof_n], s);
    mn_launch_step(h->A, h->P, h->params.precision, h->params.step_lanes, actions_dev, obs_dev, reward_dev, done_dev, info_dev, parity, ring, s);
    if (prof) { (void)hipEventRecord(h->ev[2 * h->prof_n + 1], s); h->prof_n++; }
    MN_HIP(h, hipGetLastError());
    h->last_parity = parity;
    h->step_parity = parity ^ 1;
    return MN_OK;
}

extern "C" int mn_step(mn_handle *h, const int32_t *actions_dev, float *obs_dev, float *reward_dev, uint8_t *done_dev,
                       uint8_t *info_dev, void *stream) {
    return step_common(h, actions_dev, obs_dev, reward_dev, done_dev, info_dev, nullptr, stream);
}

extern "C" int mn_step_append(mn_handle *h, const int32_t *actions_dev, const float *prev_obs_dev, float *obs_dev,
                              float *reward_dev, uint8_t *done_dev, uint8_t *info_dev, float *ring_states,
                              float *ring_next_states, int64_t *ring_actions, float *ring_rewards, float *ring_dones,
                              int64_t ptr, int64_t capacity, void *stream) {
    if (!h || !prev_obs_dev || !ring_states || !ring_next_states || !ring_actions || !ring_rewards || !ring_dones)
        return MN_ERR_INVALID;
    if (prev_obs_dev == obs_dev) return fail(h, MN_ERR_INVALID, "mn_step_append: obs_t and obs_t+1 must be different buffers");
    if (capacity <= 0 || ptr < 0 || ptr >= capacity) return fail(h, MN_ERR_INVALID, "mn_step_append: ptr out of [0, capacity)");
    const MnRing R = {prev_obs_dev, ring_states, ring_next_states, ring_actions, ring_rewards, ring_dones, ptr, capacity};
    return step_common(h, actions_dev, obs_dev, reward_dev, done_dev, info_dev, &R, stream);
}

// What the episode entry points share around their one launch: the device guard, whatever has to be enqueued in front of the launch (`prepare`: the
// weight image of a learned policy; its error code is the entry point's), the profiling event pair, the launch error and the parity reset -- the
// episode kernels zero both done-queue counters: a following mn_reset_done has nothing to do, the next mn_step starts clean.
template <class Prepare, class Launch>
static int launch_episodes(mn_handle *h, hipStream_t s, Prepare prepare, Launch launch) {
    MN_ON_DEVICE(h);
    const int rc = prepare();
    if (rc) return rc;
    const bool prof = h->prof_n < h->prof_max;
    if (prof) (void)hipEventRecord(h->ev[2 * h->prof_n], s);
    launch();
    if (prof) { (void)hipEventRecord(h->ev[2 * h->prof_n + 1], s); h->prof_n++; }
    MN_HIP(h, hipGetLastError());
    h->step_parity = 0;
    h->last_parity = 0;
    return MN_OK;
}
template <class Launch>
static int launch_episodes(mn_handle *h, hipStream_t s, Launch launch) {
    return launch_episodes(h, s, [] { return MN_OK; }, launch);
}

// The sub-step trajectory trace an episode entry point launches with: the attachment of mn_set_trajectory_trace, detached here whatever the outcome
// (*out = NULL: none).  One that is too short for the launch, or whose sub-step count is no longer the handle's N, is refused.
static int take_traj_trace(mn_handle *h, int32_t n_steps, double **out) {
    double *t = h->traj_trace;
    const int32_t steps = h->traj_trace_steps, sub = h->traj_trace_sub;
    h->traj_trace = nullptr;
    h->traj_trace_steps = 0;
    *out = nullptr;
    if (!t) return MN_OK;
    if (h->params.precision != MN_PRECISION_F64) return fail(h, MN_ERR_INVALID, "sub-step trajectories are recorded only with MN_PRECISION_F64");
    if (n_steps > steps) return fail(h, MN_ERR_INVALID, "the attached trajectory trace has fewer steps than the launch");
    if (sub != h->P.N) return fail(h, MN_ERR_INVALID, "the attached trajectory trace was sized for another robot N");
    *out = t;
    return MN_OK;
}

extern "C" int mn_set_trajectory_trace(mn_handle *h, double *traj_trace_dev, int32_t n_steps, int32_t n_substeps) {
    if (!h) return MN_ERR_INVALID;
    if (!traj_trace_dev) { h->traj_trace = nullptr; h->traj_trace_steps = 0; return MN_OK; }      // detach
    if (h->params.precision != MN_PRECISION_F64) return fail(h, MN_ERR_INVALID, "sub-step trajectories are recorded only with MN_PRECISION_F64");
    if (n_steps < 1) return fail(h, MN_ERR_INVALID, "mn_set_trajectory_trace: n_steps < 1");
    if (n_substeps != h->P.N) return fail(h, MN_ERR_INVALID, "mn_set_trajectory_trace: n_substeps must be the handle's robot N");
    h->traj_trace = traj_trace_dev;
    h->traj_trace_steps = n_steps;
    h->traj_trace_sub = n_substeps;
    return MN_OK;
}

// ---- observation noise (mn_obs_noise_body.h, mn_obs_noise.hip) ----
static int noise_spec(mn_handle *h, const mn_obs_noise *spec, MnObsNoiseDev *out) {
    const char *bad = mn_obs_noise_dev_of(*spec, out);
    if (!bad) return MN_OK;
    char b[160];
    snprintf(b, sizeof(b), "observation noise: %s must be %s", bad, !strcmp(bad, "sonar_miss_p") ? "in [0, 1]" : "finite and not negative");
    return fail(h, MN_ERR_INVALID, b);
}
// the episode forms without a NOISE instantiation refuse a handle that perceives noise; they do not ignore the description
static int refuse_noise(mn_handle *h, const char *who) {
    if (!h->noise_on) return MN_OK;
    char b[200];
    snprintf(b, sizeof(b), "%s has no observation-noise form: detach the description (mn_set_obs_noise(h, NULL, 0)) or run the per-step loop (mn_env_perturb_obs)", who);
    return fail(h, MN_ERR_INVALID, b);
}

extern "C" int mn_obs_perturb(const float *obs_in_dev, float *obs_out_dev, int64_t n, uint64_t env_index0, const int32_t *ep_t_dev, const mn_obs_noise *spec,
                              void *stream) {
    if (!obs_in_dev || !obs_out_dev || !ep_t_dev || !spec || n < 1 || n > (int64_t)1 << 40) return fail(nullptr, MN_ERR_INVALID, "mn_obs_perturb: a NULL argument or n < 1");
    if ((uintptr_t)obs_in_dev % 4 != 0 || (uintptr_t)obs_out_dev % 4 != 0 || (uintptr_t)ep_t_dev % 4 != 0)
        return fail(nullptr, MN_ERR_INVALID, "mn_obs_perturb: a misaligned argument");
    MnObsNoiseDev d;
    const int rc = noise_spec(nullptr, spec, &d);
    if (rc) return rc;
    mn_launch_obs_perturb(obs_in_dev, obs_out_dev, n, env_index0, ep_t_dev, d, (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? MN_OK : MN_ERR_HIP;
}

extern "C" int mn_set_obs_noise(mn_handle *h, const mn_obs_noise *spec, uint64_t first_env_index) {
    if (!h) return MN_ERR_INVALID;
    if (!spec) { h->noise_on = h->noise_attached = false; return MN_OK; }      // detach
    MnObsNoiseDev d;
    const int rc = noise_spec(h, spec, &d);      // (a refused description leaves the attachment as it was)
    if (rc) return rc;
    h->noise = d;
    h->noise_env0 = first_env_index;
    h->noise_attached = true;
    h->noise_on = !mn_obs_noise_is_off(d);
    return MN_OK;
}

extern "C" int mn_env_perturb_obs(mn_handle *h, const float *obs_in_dev, float *obs_out_dev, void *stream) {
    if (!h) return MN_ERR_INVALID;
    if (!obs_in_dev || !obs_out_dev || (uintptr_t)obs_in_dev % 4 != 0 || (uintptr_t)obs_out_dev % 4 != 0)
        return fail(h, MN_ERR_INVALID, "mn_env_perturb_obs: a NULL or misaligned argument");
    hipStream_t s = (hipStream_t)stream;
    join_reset(h, s);      // the counters a pending or owed reset writes are final before they are read
    MN_ON_DEVICE(h);
    const MnObsNoiseDev off = {};
    mn_launch_obs_perturb(obs_in_dev, obs_out_dev, h->A.n, h->noise_env0, h->A.ep_t, h->noise_attached ? h->noise : off, s);
    MN_HIP(h, hipGetLastError());
    return MN_OK;
}

extern "C" int mn_rollout(mn_handle *h, int32_t n_steps, const int32_t *actions_dev, uint64_t action_seed,
                          uint64_t first_step_index, uint64_t first_env_index, float *obs_dev, float *obs_trace_dev,
                          float *reward_trace_dev, uint8_t *done_trace_dev, uint8_t *info_trace_dev,
                          int32_t *action_trace_dev, void *stream) {
    if (!h || !obs_dev || n_steps < 1) return MN_ERR_INVALID;
    if (h->traj_trace) return fail(h, MN_ERR_INVALID, "mn_rollout records no trajectory trace: detach it (mn_set_trajectory_trace(h, NULL, 0, 0))");
    hipStream_t s = (hipStream_t)stream;
    return launch_episodes(h, s, [&] {
        mn_launch_rollout(h->A, h->P, h->params.precision, h->params.rollout_lanes, n_steps, actions_dev, action_seed, first_step_index,
                          first_env_index, obs_dev, obs_trace_dev, reward_trace_dev, done_trace_dev, info_trace_dev, action_trace_dev, s);
    });
}

extern "C" int mn_rollout_policy(mn_handle *h, int32_t n_steps, int32_t policy, float *obs_dev, float *obs_trace_dev, float *reward_trace_dev,
                                 uint8_t *done_trace_dev, uint8_t *info_trace_dev, int32_t *action_trace_dev, void *stream) {
    if (!h) return MN_ERR_INVALID;
    double *traj = nullptr;
    const int trc = take_traj_trace(h, n_steps, &traj);      // first: the attachment is consumed even by a call refused below
    if (!obs_dev || n_steps < 1 || (policy != MN_POLICY_APF && policy != MN_POLICY_BA)) return MN_ERR_INVALID;
    if (trc) return trc;
    if (h->noise_on && h->params.precision != MN_PRECISION_F64) {
        const int nrc = refuse_noise(h, "mn_rollout_policy on a mixed-precision handle");
        if (nrc) return nrc;
    }
    hipStream_t s = (hipStream_t)stream;
    return launch_episodes(h, s, [&] {
        mn_launch_rollout_policy(h->A, h->P, h->params.precision, n_steps, policy, obs_dev, obs_trace_dev, reward_trace_dev, done_trace_dev,
                                 info_trace_dev, action_trace_dev, traj, s, h->noise_on ? &h->noise : nullptr, h->noise_env0);
    });
}

// mn_rollout_iqn_rows and mn_rollout_iqn_eval: one routine, the acting kernel or -- `eval` -- act_eval's with its two traces
static int rollout_iqn(mn_handle *h, mn_iqn_ctx *ctx, const float *const *weights, int32_t n_steps, uint64_t *rng_state_dev, float cvar, int32_t adaptive,
                       const float *cvar_row_dev, const uint8_t *adaptive_row_dev, float *obs_dev, float *obs_trace_dev, float *reward_trace_dev,
                       uint8_t *done_trace_dev, uint8_t *info_trace_dev, int32_t *action_trace_dev, float *cvar_trace_dev, float *q_trace_dev, bool eval,
                       float *quantiles_trace_dev, float *taus_trace_dev, int32_t *steps_run_dev, void *stream) {
    if (!h) return MN_ERR_INVALID;
    double *traj = nullptr;
    const int trc = take_traj_trace(h, n_steps, &traj);      // first: the attachment is consumed even by a call refused below
    if (!ctx || !weights || !rng_state_dev || !obs_dev || n_steps < 1) return MN_ERR_INVALID;      // (the 14 pointers of `weights`: mn_iqn_rollout_image)
    if ((long)h->A.n * 32 >= (1L << 32)) return MN_ERR_INVALID;      // 32-bit draw index, as mn_iqn_act_rng
    if (trc) return trc;
    if (eval) { const int nrc = refuse_noise(h, "mn_rollout_iqn_eval"); if (nrc) return nrc; }
    hipStream_t s = (hipStream_t)stream;
    const uint32_t *image = nullptr;
    uint32_t *words = nullptr;
    return launch_episodes(h, s, [&] { return mn_iqn_rollout_image(ctx, weights, s, &image, &words); }, [&] {
        if (eval)
            mn_launch_rollout_iqn_eval(h->A, h->P, h->params.precision, n_steps, image, rng_state_dev, cvar, adaptive ? 1 : 0, cvar_row_dev, adaptive_row_dev, obs_dev,
                                       obs_trace_dev, reward_trace_dev, done_trace_dev, info_trace_dev, action_trace_dev, cvar_trace_dev, q_trace_dev, traj,
                                       quantiles_trace_dev, taus_trace_dev, words, steps_run_dev, s);
        else
            mn_launch_rollout_iqn_rows(h->A, h->P, h->params.precision, n_steps, image, rng_state_dev, cvar, adaptive ? 1 : 0, cvar_row_dev, adaptive_row_dev, obs_dev,
                                       obs_trace_dev, reward_trace_dev, done_trace_dev, info_trace_dev, action_trace_dev, cvar_trace_dev, q_trace_dev, traj, words,
                                       steps_run_dev, s, h->noise_on ? &h->noise : nullptr, h->noise_env0);
    });
}

extern "C" int mn_rollout_iqn_rows(mn_handle *h, mn_iqn_ctx *ctx, const float *const *weights, int32_t n_steps, uint64_t *rng_state_dev, float cvar,
                                   int32_t adaptive, const float *cvar_row_dev, const uint8_t *adaptive_row_dev, float *obs_dev, float *obs_trace_dev,
                                   float *reward_trace_dev, uint8_t *done_trace_dev, uint8_t *info_trace_dev, int32_t *action_trace_dev, float *cvar_trace_dev,
                                   float *q_trace_dev, int32_t *steps_run_dev, void *stream) {
    return rollout_iqn(h, ctx, weights, n_steps, rng_state_dev, cvar, adaptive, cvar_row_dev, adaptive_row_dev, obs_dev, obs_trace_dev, reward_trace_dev,
                       done_trace_dev, info_trace_dev, action_trace_dev, cvar_trace_dev, q_trace_dev, false, nullptr, nullptr, steps_run_dev, stream);
}

extern "C" int mn_rollout_iqn_eval(mn_handle *h, mn_iqn_ctx *ctx, const float *const *weights, int32_t n_steps, uint64_t *rng_state_dev, float cvar,
                                   int32_t adaptive, const float *cvar_row_dev, const uint8_t *adaptive_row_dev, float *obs_dev, float *obs_trace_dev,
                                   float *reward_trace_dev, uint8_t *done_trace_dev, uint8_t *info_trace_dev, int32_t *action_trace_dev, float *cvar_trace_dev,
                                   float *q_trace_dev, float *quantiles_trace_dev, float *taus_trace_dev, int32_t *steps_run_dev, void *stream) {
    return rollout_iqn(h, ctx, weights, n_steps, rng_state_dev, cvar, adaptive, cvar_row_dev, adaptive_row_dev, obs_dev, obs_trace_dev, reward_trace_dev,
                       done_trace_dev, info_trace_dev, action_trace_dev, cvar_trace_dev, q_trace_dev, true, quantiles_trace_dev, taus_trace_dev, steps_run_dev,
                       stream);
}

extern "C" int mn_rollout_iqn(mn_handle *h, mn_iqn_ctx *ctx, const float *const *weights, int32_t n_steps, uint64_t *rng_state_dev, float cvar,
                              int32_t adaptive, float *obs_dev, float *obs_trace_dev, float *reward_trace_dev, uint8_t *done_trace_dev,
                              uint8_t *info_trace_dev, int32_t *action_trace_dev, float *cvar_trace_dev, float *q_trace_dev, int32_t *steps_run_dev,
                              void *stream) {
    return mn_rollout_iqn_rows(h, ctx, weights, n_steps, rng_state_dev, cvar, adaptive, nullptr, nullptr, obs_dev, obs_trace_dev, reward_trace_dev,
                               done_trace_dev, info_trace_dev, action_trace_dev, cvar_trace_dev, q_trace_dev, steps_run_dev, stream);
}

extern "C" int mn_rollout_iqn_groups(mn_handle *h, const uint32_t *images_dev, int64_t image_stride, int32_t n_groups, int32_t rows_per_group,
                                     int32_t n_steps, uint64_t *rng_states_dev, const float *cvar_row_dev, const uint8_t *adaptive_row_dev, float *obs_dev,
                                     float *obs_trace_dev, float *reward_trace_dev, uint8_t *done_trace_dev, uint8_t *info_trace_dev, int32_t *action_trace_dev,
                                     float *cvar_trace_dev, float *q_trace_dev, uint32_t *group_words_dev, int32_t *steps_run_dev, void *stream) {
    if (!h) return MN_ERR_INVALID;
    if (h->traj_trace) {      // as mn_rollout: the attachment is consumed, the call refused
        h->traj_trace = nullptr;
        h->traj_trace_steps = 0;
        return fail(h, MN_ERR_INVALID, "mn_rollout_iqn_groups records no trajectory trace");
    }
    if (!images_dev || !rng_states_dev || !obs_dev || !group_words_dev || n_steps < 1) return MN_ERR_INVALID;
    if (n_groups < 1 || rows_per_group < 1 || (int64_t)n_groups * rows_per_group != (int64_t)h->A.n)
        return fail(h, MN_ERR_INVALID, "mn_rollout_iqn_groups: n_groups * rows_per_group must be the handle's n_envs");
    if (image_stride < mn_iqn_image_floats() || image_stride % 4 != 0)
        return fail(h, MN_ERR_INVALID, "mn_rollout_iqn_groups: image_stride below mn_iqn_image_floats() or no multiple of 4");
    { const int nrc = refuse_noise(h, "mn_rollout_iqn_groups"); if (nrc) return nrc; }
    hipStream_t s = (hipStream_t)stream;
    return launch_episodes(h, s, [&] {
        mn_launch_rollout_iqn_groups(h->A, h->P, h->params.precision, n_steps, images_dev, image_stride, rows_per_group, rng_states_dev, cvar_row_dev,
                                     adaptive_row_dev, obs_dev, obs_trace_dev, reward_trace_dev, done_trace_dev, info_trace_dev, action_trace_dev,
                                     cvar_trace_dev, q_trace_dev, group_words_dev, steps_run_dev, s);
    });
}

extern "C" int mn_rollout_dqn(mn_handle *h, const float *const *weights, float *image_dev, int32_t repack, int32_t n_steps, float *obs_dev,
                              float *obs_trace_dev, float *reward_trace_dev, uint8_t *done_trace_dev, uint8_t *info_trace_dev, int32_t *action_trace_dev,
                              float *q_trace_dev, void *stream) {
    if (!h) return MN_ERR_INVALID;
    double *traj = nullptr;
    const int trc = take_traj_trace(h, n_steps, &traj);      // first: the attachment is consumed even by a call refused below
    if (!weights || !image_dev || !obs_dev || n_steps < 1) return MN_ERR_INVALID;
    for (int i = 0; i < 18; ++i) if (!weights[i]) return MN_ERR_INVALID;
    if (trc) return trc;
    hipStream_t s = (hipStream_t)stream;
    return launch_episodes(h, s, [&] { if (repack) mn_launch_dqn_pack(weights, image_dev, s); return MN_OK; }, [&] {
        mn_launch_rollout_dqn(h->A, h->P, h->params.precision, n_steps, image_dev, obs_dev, obs_trace_dev, reward_trace_dev, done_trace_dev, info_trace_dev,
                              action_trace_dev, q_trace_dev, traj, s, h->noise_on ? &h->noise : nullptr, h->noise_env0);
    });
}

extern "C" int mn_dqn_export_image(const float *const *weights, float *image_out_dev, void *stream) {
    if (!weights || !image_out_dev || (uintptr_t)image_out_dev % 16 != 0) return MN_ERR_INVALID;
    for (int i = 0; i < 18; ++i) if (!weights[i]) return MN_ERR_INVALID;
    mn_launch_dqn_pack(weights, image_out_dev, (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? MN_OK : MN_ERR_HIP;
}

extern "C" int mn_rollout_dqn_groups(mn_handle *h, const float *images_dev, int64_t image_stride, int32_t n_groups, int32_t rows_per_group, int32_t n_steps,
                                     float *obs_dev, float *obs_trace_dev, float *reward_trace_dev, uint8_t *done_trace_dev, uint8_t *info_trace_dev,
                                     int32_t *action_trace_dev, float *q_trace_dev, void *stream) {
    if (!h) return MN_ERR_INVALID;
    if (h->traj_trace) {      // as mn_rollout_iqn_groups: the attachment is consumed, the call refused
        h->traj_trace = nullptr;
        h->traj_trace_steps = 0;
        return fail(h, MN_ERR_INVALID, "mn_rollout_dqn_groups records no trajectory trace");
    }
    if (!images_dev || !obs_dev || n_steps < 1) return MN_ERR_INVALID;
    if (n_groups < 1 || rows_per_group < 1 || (int64_t)n_groups * rows_per_group != (int64_t)h->A.n)
        return fail(h, MN_ERR_INVALID, "mn_rollout_dqn_groups: n_groups * rows_per_group must be the handle's n_envs");
    if (image_stride < mn_dqn_image_floats() || image_stride % 4 != 0 || (uintptr_t)images_dev % 16 != 0)
        return fail(h, MN_ERR_INVALID, "mn_rollout_dqn_groups: image_stride below mn_dqn_image_floats() or no multiple of 4, or images_dev not 16-byte aligned");
    { const int nrc = refuse_noise(h, "mn_rollout_dqn_groups"); if (nrc) return nrc; }
    hipStream_t s = (hipStream_t)stream;
    return launch_episodes(h, s, [&] {
        mn_launch_rollout_dqn_groups(h->A, h->P, h->params.precision, n_steps, images_dev, image_stride, n_groups, rows_per_group, obs_dev, obs_trace_dev,
                                     reward_trace_dev, done_trace_dev, info_trace_dev, action_trace_dev, q_trace_dev, s);
    });
}

extern "C" int mn_planner_act(const float *obs_dev, int32_t n, int32_t policy, const double *a, const double *w, int32_t *actions_dev, void *stream) {
    if (!obs_dev || !actions_dev || !a || !w || n <= 0 || (policy != MN_POLICY_APF && policy != MN_POLICY_BA)) return MN_ERR_INVALID;
    if ((uintptr_t)obs_dev % 8 != 0 || (uintptr_t)actions_dev % 4 != 0) return MN_ERR_INVALID;      // the kernel loads the rows as float2
    mn_launch_planner_act(obs_dev, n, policy, a, w, actions_dev, (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? MN_OK : MN_ERR_HIP;
}

extern "C" int mn_random_actions(uint64_t action_seed, uint64_t step_index, uint64_t first_env_index, int32_t n,
                                 int32_t *actions_dev, void *stream) {
    if (!actions_dev || n <= 0) return MN_ERR_INVALID;
    mn_launch_random_actions(action_seed, step_index, first_env_index, n, actions_dev, (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? MN_OK : MN_ERR_HIP;
}

extern "C" int32_t mn_build_info(void) {
#ifdef MN_ABLATION
    return MN_BUILD_ABLATION;
#else
    return 0;
#endif
}

#ifdef MN_ABLATION
// Developer builds only (libmarinenav_hip_ablation.so): removes parts of the step kernel to attribute its time.
extern "C" int mn_set_debug_skip(mn_handle *h, int32_t mask) {
    if (!h) return MN_ERR_INVALID;
    h->P.debug_skip = mask;
    return MN_OK;
}
#endif

// mn_reset_done on the handle's own stream, so that it runs UNDER whatever the caller enqueues next on `stream` -- in the training loop the act
// kernel of the next vector step, which is told which rows are still being written (mn_iqn_set_late_rows: the step's done flags, `*ready_out`,
// `*tick_out`) and takes them last.  The caller's stream is joined again by mn_reset_join, or by the next per-step entry point of this handle.
// Beside the act kernel's workgroups a CU has room for ONE reset wavefront (LDS), which runs ~4 x slower there: that hides a few hundred resets
// (a latency chain that leaves the chip idle when it runs alone) but not thousands.  So the launch goes under the act kernel only while the last
// reset launch the host has seen started at most `under_act_max` episodes (mn_set_reset_under_act_max; the count arrives through a host-mapped word,
// no synchronisation); otherwise this IS mn_reset_done and *ready_out is NULL.
// The rule of mn_reset_done_next_act (include/marinenav_hip.h)
extern "C" int32_t mn_reset_placement(float eps, int32_t n_rows, int64_t peak, int32_t under_act_max, int32_t owed_max_rows, int32_t fallback) {
    if (under_act_max == 0x7fffffff) return MN_RESET_UNDER_ACT;      // forced: the preflight tests the under-act arrangement itself
    const bool front = fallback != 0 || under_act_max < 0 || peak < 0 || peak > (int64_t)under_act_max;
    if (owed_max_rows < 0) return front ? MN_RESET_IN_FRONT : MN_RESET_UNDER_ACT;
    if (front) return MN_RESET_OWED;
    if (!(eps >= 0.f) || n_rows <= 0) return MN_RESET_UNDER_ACT;      // nothing known about the act launch
    const double rows = (1.0 - (eps < 1.f ? (double)eps : 1.0)) * (double)n_rows;      // the rows that do not explore: the ones the launch evaluates
    return rows <= (double)owed_max_rows ? MN_RESET_OWED : MN_RESET_UNDER_ACT;
}

// The pieces of an asynchronous reset (mn_reset_done_async, mn_reset_done_next_act; mn_state_load for a blob that carries the peak words): created on first use
static int ensure_async(mn_handle *h) {
    if (h->async_ready) return MN_OK;
    // a stream of ANOTHER priority gets a hardware queue of its own: created with the default priority it can end up sharing the queue of the caller's
    // stream (HIP deals streams out over a few queues; with an RCCL communicator in the process it did), and then the reset launch simply runs in front of
    // the act kernel again, behind two cross-stream events (measured: 0.380 instead of 0.360 ms per vector step)
    // (every piece is created if it is not there yet -- a call that failed half way is completed by the next one -- and `async_ready` is set last)
    int prio_lo = 0, prio_hi = 0;
    MN_HIP(h, hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi));
    if (!h->side) MN_HIP(h, hipStreamCreateWithPriority(&h->side, hipStreamNonBlocking, prio_hi));
    if (!h->ev_stepped) MN_HIP(h, hipEventCreateWithFlags(&h->ev_stepped, hipEventDisableTiming));
    if (!h->ev_reset_end) MN_HIP(h, hipEventCreateWithFlags(&h->ev_reset_end, hipEventDisableTiming));
    if (!h->ready) { int rc = dev_alloc(h, &h->ready, (size_t)h->A.npad); if (rc) return rc; }
    if (!h->seen_host) {
        void *hp = nullptr;
        MN_HIP(h, hipHostMalloc(&hp, sizeof(uint32_t), hipHostMallocMapped));
        *(volatile uint32_t *)hp = 0xffffffffu;      // nothing seen yet: the first launches run in front
        h->seen_host = (volatile uint32_t *)hp;
    }
    if (!h->seen_dev) MN_HIP(h, hipHostGetDevicePointer((void **)&h->seen_dev, (void *)h->seen_host, 0));
    if (!h->peak_dev) { int rc = dev_alloc(h, &h->peak_dev, 1); if (rc) return rc; }
    h->async_ready = true;
    return MN_OK;
}

static int reset_done_placed(mn_handle *h, float *obs_dev, void *stream, bool next_act, float eps, int32_t n_rows, int32_t fallback,
                             const uint32_t **ready_out, uint32_t *tick_out, int32_t *placement_out) {
    if (!h || !obs_dev || !ready_out || !tick_out) return MN_ERR_INVALID;
    hipStream_t s = (hipStream_t)stream;
    join_reset(h, s);
    MN_ON_DEVICE(h);
    { const int arc = ensure_async(h); if (arc) return arc; }
    *ready_out = nullptr;
    *tick_out = 0;
    // the estimate: the launches' own decaying peak of their episode counts, as of the last launch whose word has arrived (the host may run several
    // launches ahead of the device) -- a burst of episode ends keeps the resets in front for ~20 vector steps
    const uint32_t seen = *h->seen_host;
    // (mn_reset_done_async knows nothing of the next act call and whoever calls it makes that call through mn_iqn_act_rng: never owed)
    const int32_t place = mn_reset_placement(eps, n_rows, seen == 0xffffffffu ? -1 : (int64_t)seen, h->under_act_max, next_act ? h->owed_max_rows : -1, fallback);
    if (placement_out) *placement_out = place;
    if (place == MN_RESET_OWED) {
        h->reset_owed = true;
        h->owed_obs = obs_dev;
        h->owed_stream = s;
        return MN_OK;
    }
    if (place == MN_RESET_IN_FRONT) {
        launch_reset_done(h, obs_dev, s);
        MN_HIP(h, hipGetLastError());
        return MN_OK;
    }
    MN_HIP(h, hipEventRecord(h->ev_stepped, s));
    MN_HIP(h, hipStreamWaitEvent(h->side, h->ev_stepped, 0));
    h->tick += 1;
    const bool prof = h->prof_reset_n < h->prof_max;
    if (prof) (void)hipEventRecord(h->ev_reset[2 * h->prof_reset_n], h->side);
    if (h->side_delay_us > 0) mn_launch_sleep((uint32_t)h->side_delay_us, h->side);
    mn_launch_reset_under_act(h->A, h->P, h->params.precision, h->A.queue_count + h->last_parity * MN_QWORDS, h->A.queue, obs_dev, h->ready, h->tick, h->peak_dev, h->seen_dev, h->side);
    if (prof) { (void)hipEventRecord(h->ev_reset[2 * h->prof_reset_n + 1], h->side); h->prof_reset_n++; }
    MN_HIP(h, hipGetLastError());
    MN_HIP(h, hipEventRecord(h->ev_reset_end, h->side));
    h->reset_pending = true;
    *ready_out = h->ready;
    *tick_out = h->tick;
    return MN_OK;
}

extern "C" int mn_reset_done_async(mn_handle *h, float *obs_dev, void *stream, const uint32_t **ready_out, uint32_t *tick_out) {
    return reset_done_placed(h, obs_dev, stream, false, -1.f, 0, 0, ready_out, tick_out, nullptr);
}

extern "C" int mn_reset_done_next_act(mn_handle *h, float *obs_dev, void *stream, float eps, int32_t n_rows, int32_t fallback, const uint32_t **ready_out,
                                      uint32_t *tick_out, int32_t *placement_out) {
    if (!placement_out) return MN_ERR_INVALID;
    return reset_done_placed(h, obs_dev, stream, true, eps, n_rows, fallback, ready_out, tick_out, placement_out);
}

// owed_max_rows: mn_reset_done_next_act owes the reset to the next act call while that call evaluates at most this many rows ((1 - eps) n_rows), and wherever
// it would otherwise run in front of the act kernel (-1: never owed; 0x7fffffff: wherever the forced under-act mode does not rule)
extern "C" int mn_set_reset_owed_max_rows(mn_handle *h, int32_t owed_max_rows) {
    if (!h) return MN_ERR_INVALID;
    h->owed_max_rows = owed_max_rows;
    return MN_OK;
}

extern "C" int32_t mn_reset_is_owed(const mn_handle *h) { return h && h->reset_owed ? 1 : 0; }

// The act launch's side of an owed reset (mn_internal.h): iqn_act.hip's launch routine takes the debt into its preparation launch, or settles it
bool mn_owed_reset_take(mn_handle *h, hipStream_t s, MnOwedReset *out) {
    if (!h || !h->reset_owed) return false;
    int cur = -1;
    if (hipGetDevice(&cur) != hipSuccess || cur != h->device) return false;
    if (s != h->owed_stream) (void)hipStreamSynchronize(h->owed_stream);
    // (inside a profiling window the launch that runs the reset is timed as the handle's reset launch of this step, as mn_reset_done's is)
    const bool prof = h->prof_reset_n < h->prof_max;
    *out = MnOwedReset{&h->A, h->A_mem, &h->P, h->params.precision, h->A.queue_count + h->last_parity * MN_QWORDS, h->A.queue, h->owed_obs, h->peak_dev, h->seen_dev,
                       mn_prep_reset_blocks(*h->seen_host, h->A.n), prof ? h->ev_reset[2 * h->prof_reset_n] : nullptr,
                       prof ? h->ev_reset[2 * h->prof_reset_n + 1] : nullptr};
    if (prof) h->prof_reset_n++;
    h->reset_owed = false;
    return true;
}
int mn_owed_reset_settle(mn_handle *h, hipStream_t s) {
    if (!h) return MN_OK;
    join_reset(h, s);
    return h->reset_owed ? fail(h, MN_ERR_INVALID, "the handle's owed reset lives on another HIP device") : MN_OK;
}

// under_act_max: mn_reset_done_async launches under the next act kernel while the decaying peak of the episodes started per reset launch (as of the last
// launch seen) is at most this (default 1200; 0x7fffffff: always, -1: never).  *last_seen: that peak (-1: none seen yet).
extern "C" int mn_set_reset_under_act_max(mn_handle *h, int32_t under_act_max, int64_t *last_seen) {
    if (!h) return MN_ERR_INVALID;
    h->under_act_max = under_act_max;
    if (last_seen) *last_seen = (h->seen_host && *h->seen_host != 0xffffffffu) ? (int64_t)*h->seen_host : -1;
    return MN_OK;
}

// Test hook: every reset launch mn_reset_done_async puts on the handle's own stream is preceded there by a kernel that sleeps `us` microseconds -- a reset
// launch that does NOT run beside the act kernel (shared hardware queue, no room on the CUs), without needing such a box.  0 switches it off.
extern "C" int mn_debug_side_delay_us(mn_handle *h, int32_t us) {
    if (!h || us < 0 || us > 10000000) return MN_ERR_INVALID;
    h->side_delay_us = us;
    return MN_OK;
}

extern "C" int mn_reset_join(mn_handle *h, void *stream) {
    if (!h) return MN_ERR_INVALID;
    join_reset(h, (hipStream_t)stream);
    return h->reset_pending ? fail(h, MN_ERR_HIP, "hipStreamWaitEvent failed") : MN_OK;
}

extern "C" int mn_reset_done(mn_handle *h, float *obs_dev, void *stream) {
    if (!h || !obs_dev) return MN_ERR_INVALID;
    join_reset(h, (hipStream_t)stream);
    MN_ON_DEVICE(h);
    launch_reset_done(h, obs_dev, (hipStream_t)stream);
    MN_HIP(h, hipGetLastError());
    return MN_OK;
}

extern "C" int mn_last_done_count(mn_handle *h, void *stream, int32_t *out) {
    if (!h || !out) return MN_ERR_INVALID;
    MN_ON_DEVICE(h);
    MN_HIP(h, hipStreamSynchronize((hipStream_t)stream));
    uint32_t w[MN_QWORDS], v = 0;      // the shard counters of the last step's done-queue
    MN_HIP(h, hipMemcpy(w, h->A.queue_count + h->last_parity * MN_QWORDS, sizeof(w), hipMemcpyDeviceToHost));
    for (int sh = 0; sh < MN_QSHARDS; ++sh) v += w[sh * MN_QSTRIDE];
    *out = (int32_t)v;
    return MN_OK;
}

// [count][K] host rows <-> [K][npad] device table
static int table_to_dev(mn_handle *h, double *dev, int first, int count, int K, const std::vector<double> &host_kc) {
    MN_HIP(h, hipMemcpy2D(dev + first, (size_t)h->A.npad * 8, host_kc.data(), (size_t)count * 8, (size_t)count * 8, K, hipMemcpyHostToDevice));
    return MN_OK;
}
static int table_from_dev(mn_handle *h, const double *dev, int first, int count, int K, std::vector<double> &host_kc) {
    host_kc.resize((size_t)K * count);
    MN_HIP(h, hipMemcpy2D(host_kc.data(), (size_t)count * 8, dev + first, (size_t)h->A.npad * 8, (size_t)count * 8, K, hipMemcpyDeviceToHost));
    return MN_OK;
}

extern "C" int mn_load_worlds(mn_handle *h, int32_t first, int32_t count, const int32_t *n_cores, const double *cores_xy,
                              const int32_t *clockwise, const double *gamma, const int32_t *n_obs, const double *obs_xy,
                              const double *obs_r, const double *start, const double *goal, const double *init_theta,
                              const double *init_speed, float *obs_dev, void *stream) {
    int rc = range_ok(h, first, count);
    if (rc) return rc;
    if (count == 0) return MN_OK;
    if (!n_cores || !cores_xy || !clockwise || !gamma || !n_obs || !obs_xy || !obs_r || !start || !goal || !init_theta || !init_speed)
        return MN_ERR_INVALID;
    hipStream_t s = (hipStream_t)stream;
    MN_HIP(h, hipStreamSynchronize(s));
    const int C = MN_MAX_CORES, O = MN_MAX_OBS;
    std::vector<double> cx((size_t)C * count), cy((size_t)C * count), cg((size_t)C * count);
    std::vector<double> ox((size_t)O * count), oy((size_t)O * count), orr((size_t)O * count);
    std::vector<double> sx(count), sy(count), gx(count), gy(count);
    std::vector<int32_t> cnt(count), zeros(count, 0), list(count);
    for (int i = 0; i < count; ++i) {
        if (n_cores[i] < 0 || n_cores[i] > C || n_obs[i] < 0 || n_obs[i] > O) return fail(h, MN_ERR_INVALID, "world exceeds capacity (8 cores, 10 obstacles)");
        for (int k = 0; k < C; ++k) {
            const bool v = k < n_cores[i];
            cx[(size_t)k * count + i] = v ? cores_xy[((size_t)i * C + k) * 2] : 0.0;
            cy[(size_t)k * count + i] = v ? cores_xy[((size_t)i * C + k) * 2 + 1] : 0.0;
            cg[(size_t)k * count + i] = v ? (clockwise[(size_t)i * C + k] ? gamma[(size_t)i * C + k] : -gamma[(size_t)i * C + k]) : 0.0;
        }
        for (int k = 0; k < O; ++k) {
            const bool v = k < n_obs[i];
            ox[(size_t)k * count + i] = v ? obs_xy[((size_t)i * O + k) * 2] : 0.0;
            oy[(size_t)k * count + i] = v ? obs_xy[((size_t)i * O + k) * 2 + 1] : 0.0;
            orr[(size_t)k * count + i] = v ? obs_r[(size_t)i * O + k] : 0.0;
        }
        sx[i] = start[2 * i]; sy[i] = start[2 * i + 1]; gx[i] = goal[2 * i]; gy[i] = goal[2 * i + 1];
        cnt[i] = n_cores[i] | (n_obs[i] << 8);
        list[i] = first + i;
    }
    if ((rc = table_to_dev(h, h->A.cx, first, count, C, cx)) || (rc = table_to_dev(h, h->A.cy, first, count, C, cy)) ||
        (rc = table_to_dev(h, h->A.cg, first, count, C, cg)) || (rc = table_to_dev(h, h->A.ox, first, count, O, ox)) ||
        (rc = table_to_dev(h, h->A.oy, first, count, O, oy)) || (rc = table_to_dev(h, h->A.orad, first, count, O, orr)))
        return rc;
    const size_t b8 = (size_t)count * 8;
    MN_HIP(h, hipMemcpy(h->A.start_x + first, sx.data(), b8, hipMemcpyHostToDevice));
    MN_HIP(h, hipMemcpy(h->A.start_y + first, sy.data(), b8, hipMemcpyHostToDevice));
    MN_HIP(h, hipMemcpy(h->A.goal_x + first, gx.data(), b8, hipMemcpyHostToDevice));
    MN_HIP(h, hipMemcpy(h->A.goal_y + first, gy.data(), b8, hipMemcpyHostToDevice));
    MN_HIP(h, hipMemcpy(h->A.init_theta + first, init_theta, b8, hipMemcpyHostToDevice));
    MN_HIP(h, hipMemcpy(h->A.init_speed + first, init_speed, b8, hipMemcpyHostToDevice));
    MN_HIP(h, hipMemcpy(h->A.counts + first, cnt.data(), (size_t)count * 4, hipMemcpyHostToDevice));
    MN_HIP(h, hipMemcpy(h->list_scratch, list.data(), (size_t)count * 4, hipMemcpyHostToDevice));
    mn_launch_reset(h->A, h->P, h->params.precision, nullptr, (uint32_t)count, h->list_scratch, 1, obs_dev, s);
    MN_HIP(h, hipGetLastError());
    MN_HIP(h, hipStreamSynchronize(s));
    return MN_OK;
}

extern "C" int mn_get_worlds(mn_handle *h, int32_t first, int32_t count, int32_t *n_cores, double *cores_xy, int32_t *clockwise,
                             double *gamma, int32_t *n_obs, double *obs_xy, double *obs_r, double *start, double *goal,
                             double *init_theta, double *init_speed) {
    int rc = range_ok(h, first, count);
    if (rc) return rc;
    if (count == 0) return MN_OK;
    MN_HIP(h, hipDeviceSynchronize());
    const int C = MN_MAX_CORES, O = MN_MAX_OBS;
    std::vector<double> cx, cy, cg, ox, oy, orr, sx(count), sy(count), gx(count), gy(count);
    std::vector<int32_t> cnt(count);
    if ((rc = table_from_dev(h, h->A.cx, first, count, C, cx)) || (rc = table_from_dev(h, h->A.cy, first, count, C, cy)) ||
        (rc = table_from_dev(h, h->A.cg, first, count, C, cg)) || (rc = table_from_dev(h, h->A.ox, first, count, O, ox)) ||
        (rc = table_from_dev(h, h->A.oy, first, count, O, oy)) || (rc = table_from_dev(h, h->A.orad, first, count, O, orr)))
        return rc;
    const size_t b8 = (size_t)count * 8;
    MN_HIP(h, hipMemcpy(sx.data(), h->A.start_x + first, b8, hipMemcpyDeviceToHost));
    MN_HIP(h, hipMemcpy(sy.data(), h->A.start_y + first, b8, hipMemcpyDeviceToHost));
    MN_HIP(h, hipMemcpy(gx.data(), h->A.goal_x + first, b8, hipMemcpyDeviceToHost));
    MN_HIP(h, hipMemcpy(gy.data(), h->A.goal_y + first, b8, hipMemcpyDeviceToHost));
    if (init_theta) MN_HIP(h, hipMemcpy(init_theta, h->A.init_theta + first, b8, hipMemcpyDeviceToHost));
    if (init_speed) MN_HIP(h, hipMemcpy(init_speed, h->A.init_speed + first, b8, hipMemcpyDeviceToHost));
    MN_HIP(h, hipMemcpy(cnt.data(), h->A.counts + first, (size_t)count * 4, hipMemcpyDeviceToHost));
    for (int i = 0; i < count; ++i) {
        const int nc = cnt[i] & 0xff, no = (cnt[i] >> 8) & 0xff;
        if (n_cores) n_cores[i] = nc;
        if (n_obs) n_obs[i] = no;
        for (int k = 0; k < C; ++k) {
            const double g = cg[(size_t)k * count + i];
            if (cores_xy) { cores_xy[((size_t)i * C + k) * 2] = cx[(size_t)k * count + i]; cores_xy[((size_t)i * C + k) * 2 + 1] = cy[(size_t)k * count + i]; }
            if (clockwise) clockwise[(size_t)i * C + k] = g > 0.0 ? 1 : 0;
            if (gamma) gamma[(size_t)i * C + k] = fabs(g);
        }
        for (int k = 0; k < O; ++k) {
            if (obs_xy) { obs_xy[((size_t)i * O + k) * 2] = ox[(size_t)k * count + i]; obs_xy[((size_t)i * O + k) * 2 + 1] = oy[(size_t)k * count + i]; }
            if (obs_r) obs_r[(size_t)i * O + k] = orr[(size_t)k * count + i];
        }
        if (start) { start[2 * i] = sx[i]; start[2 * i + 1] = sy[i]; }
        if (goal) { goal[2 * i] = gx[i]; goal[2 * i + 1] = gy[i]; }
    }
    return MN_OK;
}

// ---- queries: nothing in the handle is written (mn_query.hip) -------------------------------------------------------------------
static int query_common(mn_handle *h, const int32_t *env_of_query_dev, int32_t env0, const void *in_dev, int64_t n_queries, hipStream_t s) {
    if (!h) return fail(nullptr, MN_ERR_INVALID, "query: NULL handle");
    if (n_queries < 0) return fail(h, MN_ERR_INVALID, "query: n_queries is negative");
    if (!env_of_query_dev && (env0 < 0 || env0 >= h->A.n)) {
        char b[128];
        snprintf(b, sizeof(b), "query: env0 = %d is outside [0, %d) and no env_of_query array is given", env0, h->A.n);
        return fail(h, MN_ERR_INVALID, b);
    }
    if (n_queries > 0 && !in_dev) return fail(h, MN_ERR_INVALID, "query: NULL input array");
    join_reset(h, s);
    return on_device(h);
}

extern "C" int mn_query_velocity(mn_handle *h, const int32_t *env_of_query_dev, int32_t env0, const double *xy_dev, int64_t n_queries, double *v_dev,
                                 void *stream) {
    hipStream_t s = (hipStream_t)stream;
    const int rc = query_common(h, env_of_query_dev, env0, xy_dev, n_queries, s);
    if (rc) return rc;
    if (n_queries == 0) return MN_OK;
    if (!v_dev) return fail(h, MN_ERR_INVALID, "mn_query_velocity: v_dev is NULL");
    mn_launch_query_velocity(h->A, h->P, env_of_query_dev, env0, xy_dev, n_queries, v_dev, s);
    MN_HIP(h, hipGetLastError());
    return MN_OK;
}

extern "C" int mn_query_observation(mn_handle *h, const int32_t *env_of_query_dev, int32_t env0, const double *state_dev, int32_t velocity_mode,
                                    int64_t n_queries, float *obs_dev, double *obs64_dev, uint8_t *flags_dev, void *stream) {
    hipStream_t s = (hipStream_t)stream;
    if (h && velocity_mode != MN_QUERY_VELOCITY_GIVEN && velocity_mode != MN_QUERY_VELOCITY_FROM_CURRENT)
        return fail(h, MN_ERR_INVALID, "mn_query_observation: velocity_mode is neither MN_QUERY_VELOCITY_GIVEN nor MN_QUERY_VELOCITY_FROM_CURRENT");
    const int rc = query_common(h, env_of_query_dev, env0, state_dev, n_queries, s);
    if (rc) return rc;
    if (n_queries == 0) return MN_OK;
    if (!obs_dev && !obs64_dev && !flags_dev) return fail(h, MN_ERR_INVALID, "mn_query_observation: every output is NULL");
    if ((uintptr_t)obs_dev & 7) return fail(h, MN_ERR_INVALID, "mn_query_observation: obs_dev must be 8-byte aligned (rows leave as float pairs)");
    mn_launch_query_observation(h->A, h->P, env_of_query_dev, env0, state_dev, velocity_mode == MN_QUERY_VELOCITY_FROM_CURRENT, n_queries, obs_dev,
                                obs64_dev, flags_dev, s);
    MN_HIP(h, hipGetLastError());
    return MN_OK;
}

extern "C" int mn_query_rollout(mn_handle *h, const int32_t *env_of_query_dev, int32_t env0, const double *state_dev, const int32_t *episode_timesteps_dev,
                                int32_t action_mode, const int32_t *actions_dev, int32_t n_steps, const int32_t *n_steps_of_query_dev, int64_t n_queries,
                                double *state_out_dev, float *obs_dev, double *obs64_dev, double *reward_dev, uint8_t *done_dev, uint8_t *info_dev,
                                int32_t *steps_dev, double *reward_trace_dev, uint8_t *done_trace_dev, uint8_t *info_trace_dev, int32_t *action_trace_dev,
                                double *state_trace_dev, double *traj_trace_dev, void *stream) {
    hipStream_t s = (hipStream_t)stream;
    if (h && action_mode != MN_QUERY_ACTIONS_SHARED && action_mode != MN_QUERY_ACTIONS_CONSTANT && action_mode != MN_QUERY_ACTIONS_PER_QUERY)
        return fail(h, MN_ERR_INVALID, "mn_query_rollout: action_mode is none of MN_QUERY_ACTIONS_SHARED, _CONSTANT, _PER_QUERY");
    if (h && (n_steps < 0 || n_steps > MN_QUERY_MAX_STEPS)) {
        char b[128];
        snprintf(b, sizeof(b), "mn_query_rollout: n_steps = %d is outside [0, %d]", n_steps, MN_QUERY_MAX_STEPS);
        return fail(h, MN_ERR_INVALID, b);
    }
    const int rc = query_common(h, env_of_query_dev, env0, state_dev, n_queries, s);
    if (rc) return rc;
    if (n_queries == 0) return MN_OK;
    if (n_steps > 0 && !actions_dev) return fail(h, MN_ERR_INVALID, "mn_query_rollout: actions_dev is NULL");
    if (!state_out_dev && !obs_dev && !obs64_dev && !reward_dev && !done_dev && !info_dev && !steps_dev && !reward_trace_dev && !done_trace_dev &&
        !info_trace_dev && !action_trace_dev && !state_trace_dev && !traj_trace_dev)
        return fail(h, MN_ERR_INVALID, "mn_query_rollout: every output is NULL");
    if ((uintptr_t)obs_dev & 7) return fail(h, MN_ERR_INVALID, "mn_query_rollout: obs_dev must be 8-byte aligned (rows leave as float pairs)");
    mn_launch_query_rollout(h->A, h->P, env_of_query_dev, env0, state_dev, episode_timesteps_dev, action_mode, actions_dev, n_steps, n_steps_of_query_dev,
                            n_queries, state_out_dev, obs_dev, obs64_dev, reward_dev, done_dev, info_dev, steps_dev, reward_trace_dev, done_trace_dev,
                            info_trace_dev, action_trace_dev, state_trace_dev, traj_trace_dev, s);
    MN_HIP(h, hipGetLastError());
    return MN_OK;
}

// ---- minimum-time-to-goal fields: nothing in the handle is written (mn_time_field.hip) ------------------------------------------------------------
static bool time_field_grid_ok(int32_t nx, int32_t ny) { return nx >= 1 && ny >= 1 && (int64_t)nx * ny <= MN_TIME_FIELD_MAX_CELLS; }

extern "C" int64_t mn_time_field_workspace_bytes(int32_t nx, int32_t ny, int64_t n_fields) {
    if (!time_field_grid_ok(nx, ny) || n_fields < 0) return (int64_t)MN_ERR_INVALID;
    return mn_time_field_planes_bytes(nx, ny, n_fields);
}

extern "C" int mn_time_field(mn_handle *h, const int32_t *env_of_field_dev, int32_t env0, const double *goal_xy_dev, int64_t n_fields, int32_t nx,
                             int32_t ny, double speed, double clearance, int32_t max_sweeps, double *T_dev, uint8_t *dir_dev, int32_t *status_dev,
                             int32_t *sweeps_dev, void *workspace_dev, void *stream) {
    hipStream_t s = (hipStream_t)stream;
    if (!h) return fail(nullptr, MN_ERR_INVALID, "mn_time_field: NULL handle");
    if (n_fields < 0 || n_fields >= ((int64_t)1 << 31)) return fail(h, MN_ERR_INVALID, "mn_time_field: n_fields is negative or not below 2^31");
    if (!time_field_grid_ok(nx, ny)) {
        char b[160];
        snprintf(b, sizeof(b), "mn_time_field: a grid of %d x %d cells is outside 1 <= nx, ny and nx * ny <= %d", nx, ny, MN_TIME_FIELD_MAX_CELLS);
        return fail(h, MN_ERR_INVALID, b);
    }
    if (!(clearance >= 0.0) || !(clearance - clearance == 0.0)) return fail(h, MN_ERR_INVALID, "mn_time_field: clearance is negative or not finite");
    if (max_sweeps < 1) return fail(h, MN_ERR_INVALID, "mn_time_field: max_sweeps < 1");
    if (!env_of_field_dev && (env0 < 0 || env0 >= h->A.n)) {
        char b[128];
        snprintf(b, sizeof(b), "mn_time_field: env0 = %d is outside [0, %d) and no env_of_field array is given", env0, h->A.n);
        return fail(h, MN_ERR_INVALID, b);
    }
    if (n_fields > 0 && (!T_dev || !status_dev || !workspace_dev)) return fail(h, MN_ERR_INVALID, "mn_time_field: T_dev, status_dev or workspace_dev is NULL");
    join_reset(h, s);
    MN_ON_DEVICE(h);
    if (n_fields == 0) return MN_OK;
    if (mn_launch_time_field(h->A, h->P, env_of_field_dev, env0, goal_xy_dev, n_fields, nx, ny, speed, clearance, max_sweeps, T_dev, dir_dev, status_dev,
                             sweeps_dev, workspace_dev, s) != MN_OK)
        return fail(h, MN_ERR_HIP, "mn_time_field: raising the kernel's dynamic LDS limit failed");
    MN_HIP(h, hipGetLastError());
    return MN_OK;
}

// ---- the field pilot (mn_pilot.hip): mn_pilot_act is a query, mn_rollout_pilot an episode entry point --------------------------------------------
static int pilot_args_ok(mn_handle *h, const char *who, const double *T_dev, int64_t n_fields, int32_t nx, int32_t ny, int32_t horizon) {
    char b[192];
    if (!T_dev) { snprintf(b, sizeof(b), "%s: T_dev is NULL", who); return fail(h, MN_ERR_INVALID, b); }
    if (n_fields < 1 || n_fields >= ((int64_t)1 << 31)) { snprintf(b, sizeof(b), "%s: n_fields is below 1 or not below 2^31", who); return fail(h, MN_ERR_INVALID, b); }
    if (!time_field_grid_ok(nx, ny)) {
        snprintf(b, sizeof(b), "%s: a grid of %d x %d cells is outside 1 <= nx, ny and nx * ny <= %d", who, nx, ny, MN_TIME_FIELD_MAX_CELLS);
        return fail(h, MN_ERR_INVALID, b);
    }
    if (horizon < 1 || horizon > MN_PILOT_MAX_HORIZON) {
        snprintf(b, sizeof(b), "%s: horizon = %d is outside [1, %d]", who, horizon, MN_PILOT_MAX_HORIZON);
        return fail(h, MN_ERR_INVALID, b);
    }
    return MN_OK;
}

extern "C" int mn_pilot_act(mn_handle *h, const int32_t *env_of_query_dev, int32_t env0, const double *state_dev, const int32_t *episode_timesteps_dev,
                            const double *T_dev, const int32_t *field_of_query_dev, int64_t n_fields, int32_t nx, int32_t ny, int32_t horizon,
                            int64_t n_queries, int32_t *actions_dev, double *scores_dev, int32_t *steps_dev, uint8_t *infos_dev, uint8_t *flags_dev,
                            void *stream) {
    hipStream_t s = (hipStream_t)stream;
    if (h) {
        const int arc = pilot_args_ok(h, "mn_pilot_act", T_dev, n_fields, nx, ny, horizon);
        if (arc) return arc;
    }
    const int rc = query_common(h, env_of_query_dev, env0, state_dev, n_queries, s);
    if (rc) return rc;
    if (n_queries == 0) return MN_OK;
    if (!actions_dev && !scores_dev && !steps_dev && !infos_dev && !flags_dev) return fail(h, MN_ERR_INVALID, "mn_pilot_act: every output is NULL");
    mn_launch_pilot_act(h->A, h->P, env_of_query_dev, env0, state_dev, episode_timesteps_dev, T_dev, field_of_query_dev, n_fields, nx, ny, horizon,
                        n_queries, actions_dev, scores_dev, steps_dev, infos_dev, flags_dev, s);
    MN_HIP(h, hipGetLastError());
    return MN_OK;
}

extern "C" int mn_rollout_pilot(mn_handle *h, int32_t n_steps, const double *T_dev, const int32_t *field_of_env_dev, int64_t n_fields, int32_t nx,
                                int32_t ny, int32_t horizon, float *obs_dev, float *obs_trace_dev, float *reward_trace_dev, uint8_t *done_trace_dev,
                                uint8_t *info_trace_dev, int32_t *action_trace_dev, void *stream) {
    if (!h) return MN_ERR_INVALID;
    double *traj = nullptr;
    const int trc = take_traj_trace(h, n_steps, &traj);      // first: the attachment is consumed even by a call refused below
    if (!obs_dev || n_steps < 1) return fail(h, MN_ERR_INVALID, "mn_rollout_pilot: obs_dev is NULL or n_steps < 1");
    if (h->params.precision != MN_PRECISION_F64)
        return fail(h, MN_ERR_INVALID, "mn_rollout_pilot: the pilot's episodes run only with MN_PRECISION_F64 (its candidates start from the float64 state)");
    const int arc = pilot_args_ok(h, "mn_rollout_pilot", T_dev, n_fields, nx, ny, horizon);
    if (arc) return arc;
    if (!field_of_env_dev && n_fields != h->A.n)
        return fail(h, MN_ERR_INVALID, "mn_rollout_pilot: without field_of_env_dev env i follows field i, so n_fields must equal the number of envs");
    if (trc) return trc;
    hipStream_t s = (hipStream_t)stream;
    return launch_episodes(h, s, [&] {
        mn_launch_rollout_pilot(h->A, h->P, n_steps, T_dev, field_of_env_dev, n_fields, nx, ny, horizon, obs_dev, obs_trace_dev, reward_trace_dev,
                                done_trace_dev, info_trace_dev, action_trace_dev, traj, s);
    });
}

// ---- pictures: nothing in the handle is written (mn_render.hip) -----------------------------------------------------------------------------------
static const char *render_canvas_error(const void *pixels_dev, int32_t n_images, int32_t width, int32_t height, const double *view) {
    if (!pixels_dev) return "render: pixels_dev is NULL";
    if (!view) return "render: view is NULL";
    if (n_images < 1 || width < 1 || height < 1) return "render: n_images, width and height must be at least 1";
    if ((int64_t)width * height * n_images >= ((int64_t)1 << 31)) return "render: width * height * n_images must stay below 2^31";
    for (int i = 0; i < 4; ++i) if (!(view[i] - view[i] == 0.0)) return "render: the view has a non-finite entry";
    if (!(view[2] > view[0]) || !(view[3] > view[1])) return "render: the view needs x1 > x0 and y1 > y0";
    return nullptr;
}

extern "C" int mn_render_worlds(mn_handle *h, const int32_t *env_of_image_dev, int32_t env0, int32_t n_images, int32_t width, int32_t height,
                                const double view[4], const mn_render_style *style, uint32_t *pixels_dev, void *stream) {
    hipStream_t s = (hipStream_t)stream;
    if (!h) return fail(nullptr, MN_ERR_INVALID, "mn_render_worlds: NULL handle");
    if (!style) return fail(h, MN_ERR_INVALID, "mn_render_worlds: style is NULL");
    if (const char *e = render_canvas_error(pixels_dev, n_images, width, height, view)) return fail(h, MN_ERR_INVALID, e);
    if (style->n_levels < 1 || style->n_levels > MN_RENDER_MAX_LEVELS) return fail(h, MN_ERR_INVALID, "mn_render_worlds: n_levels outside [1, 32]");
    if (style->lic_steps < 0 || style->lic_steps > MN_RENDER_MAX_LIC_STEPS) return fail(h, MN_ERR_INVALID, "mn_render_worlds: lic_steps outside [0, 64]");
    if (style->lic_floor < 0 || style->lic_floor > 255) return fail(h, MN_ERR_INVALID, "mn_render_worlds: lic_floor outside [0, 255]");
    if (!(style->v_max > 0.0)) return fail(h, MN_ERR_INVALID, "mn_render_worlds: v_max must be above 0");
    if (style->max_workgroups < 0) return fail(h, MN_ERR_INVALID, "mn_render_worlds: max_workgroups is negative");
    if (!env_of_image_dev && (env0 < 0 || env0 >= h->A.n)) {
        char b[128];
        snprintf(b, sizeof(b), "mn_render_worlds: env0 = %d is outside [0, %d) and no env_of_image array is given", env0, h->A.n);
        return fail(h, MN_ERR_INVALID, b);
    }
    join_reset(h, s);
    MN_ON_DEVICE(h);
    mn_launch_render_worlds(h->A, h->P, env_of_image_dev, env0, n_images, width, height, view, *style, pixels_dev, s);
    MN_HIP(h, hipGetLastError());
    return MN_OK;
}

extern "C" int mn_render_draw(uint32_t *pixels_dev, int32_t n_images, int32_t width, int32_t height, const double view[4], const mn_render_prim *prims_dev,
                              int64_t n_prims, void *stream) {
    mn_handle *none = nullptr;
    if (const char *e = render_canvas_error(pixels_dev, n_images, width, height, view)) return fail(none, MN_ERR_INVALID, e);
    if (n_prims < 0) return fail(none, MN_ERR_INVALID, "mn_render_draw: n_prims is negative");
    if (n_prims == 0) return MN_OK;
    if (!prims_dev) return fail(none, MN_ERR_INVALID, "mn_render_draw: prims_dev is NULL");
    mn_launch_render_draw(pixels_dev, n_images, width, height, view, prims_dev, n_prims, (hipStream_t)stream);
    MN_HIP(none, hipGetLastError());
    return MN_OK;
}

extern "C" int mn_render_font(uint8_t *out) {
    mn_handle *none = nullptr;
    if (!out) return fail(none, MN_ERR_INVALID, "mn_render_font: out is NULL");
    memcpy(out, MNR_FONT, sizeof(MNR_FONT));
    return MN_OK;
}

extern "C" int mn_get_state(mn_handle *h, int32_t first, int32_t count, double *state, int32_t *ep_t, int64_t *tot_t) {
    int rc = range_ok(h, first, count);
    if (rc) return rc;
    if (count == 0) return MN_OK;
    MN_HIP(h, hipDeviceSynchronize());
    if (state) {
        std::vector<double> v(count);
        const double *src[6] = {h->A.x, h->A.y, h->A.theta, h->A.speed, h->A.vx, h->A.vy};
        for (int k = 0; k < 6; ++k) {
            MN_HIP(h, hipMemcpy(v.data(), src[k] + first, (size_t)count * 8, hipMemcpyDeviceToHost));
            for (int i = 0; i < count; ++i) state[(size_t)i * 6 + k] = v[i];
        }
    }
    if (ep_t) MN_HIP(h, hipMemcpy(ep_t, h->A.ep_t + first, (size_t)count * 4, hipMemcpyDeviceToHost));
    if (tot_t) MN_HIP(h, hipMemcpy(tot_t, h->A.tot_t + first, (size_t)count * 8, hipMemcpyDeviceToHost));
    return MN_OK;
}

extern "C" int mn_set_state(mn_handle *h, int32_t first, int32_t count, const double *state, const int32_t *ep_t,
                            const int64_t *tot_t) {
    int rc = range_ok(h, first, count);
    if (rc) return rc;
    if (count == 0) return MN_OK;
    MN_HIP(h, hipDeviceSynchronize());
    if (state) {
        std::vector<double> v(count);
        double *dst[6] = {h->A.x, h->A.y, h->A.theta, h->A.speed, h->A.vx, h->A.vy};
        for (int k = 0; k < 6; ++k) {
            for (int i = 0; i < count; ++i) v[i] = state[(size_t)i * 6 + k];
            MN_HIP(h, hipMemcpy(dst[k] + first, v.data(), (size_t)count * 8, hipMemcpyHostToDevice));
        }
    }
    if (ep_t) MN_HIP(h, hipMemcpy(h->A.ep_t + first, ep_t, (size_t)count * 4, hipMemcpyHostToDevice));
    if (tot_t) MN_HIP(h, hipMemcpy(h->A.tot_t + first, tot_t, (size_t)count * 8, hipMemcpyHostToDevice));
    return MN_OK;
}

// ---- snapshot and restore (mn_state.hip; blob layout in mn_internal.h) ------------------------------------------------------------
// Every member of mn_handle, and whether a snapshot carries it:
//   A (the device arrays)        carried: pose, episode constants, ep_t / tot_t / counts, both sets of world tables, MT rows and positions, both halves of the
//                                done-queue.  NOT carried: obs64 / rew64 / traj (last-step outputs kept for parity reads only)
//   P, params                    validated, not restored: the blob loads only into a handle with the same params (the lane counts aside: results do not depend
//                                on them) and the same schedule; P.debug_skip exists in ablation builds only
//   step_parity, last_parity     carried: which half of the done-queue the next step fills / the next reset drains
//   tick                         carried; `ready` is zeroed by the load launch (its words are only ever compared with ticks handed out later)
//   peak_dev, *seen_host         carried (the decaying episode peak the reset placement reads); async_ready decides whether there is one
//   under_act_max, owed_max_rows carried: the placement thresholds (mn_set_reset_under_act_max, mn_set_reset_owed_max_rows)
//   reset_pending, reset_owed, owed_obs, owed_stream    always settled before a save or a load: nothing to carry
//   seeds_dev, mask_count, list_scratch, peek_scratch   scratch, rewritten by every call that reads it
//   obs64_buf, rew64_buf, traj_trace*, side_delay_us, profiling events and counters, side stream, events, device, allocs, err    configuration of the
//                                process or of a test, not state of the envs
static void state_header(const mn_handle *h, MnStateHeader *o) {
    memset(o, 0, sizeof(*o));
    o->magic = MN_STATE_MAGIC; o->version = MN_STATE_VERSION;
    o->n = h->A.n; o->precision = h->params.precision;
    o->bytes = mn_state_layout_bytes(h->A.n, h->A.qcap);
    o->header_bytes = MN_STATE_HEADER_BYTES; o->qcap = h->A.qcap;
    o->params = h->params;
    o->n_stages = h->P.n_stages; o->timestep_scale = h->P.timestep_scale;
    for (int i = 0; i < h->P.n_stages; ++i) {
        o->sched_t[i] = h->P.sched_t[i]; o->sched_nc[i] = h->P.sched_nc[i]; o->sched_no[i] = h->P.sched_no[i]; o->sched_md[i] = h->P.sched_md[i];
    }
    o->step_parity = h->step_parity; o->last_parity = h->last_parity;
    o->tick = h->tick;
    o->under_act_max = h->under_act_max; o->owed_max_rows = h->owed_max_rows;
    o->has_peak = h->async_ready ? 1u : 0u;
    o->peak = 0u; o->seen = 0xffffffffu;      // (with has_peak the save launch reads both on the device)
}

// the first field in which the blob's params / schedule differ from the handle's, or NULL
static const char *state_first_difference(const MnStateHeader &b, const MnStateHeader &m, char *buf, size_t len) {
    struct F { const char *name; size_t off, size; };
#define PF(f) {"params." #f, offsetof(mn_params, f), sizeof(((mn_params *)0)->f)}
    static const F fields[] = {PF(width), PF(height), PF(core_r), PF(v_rel_max), PF(p), PF(v_range), PF(obs_r_range), PF(clear_r), PF(goal_dis), PF(timestep_penalty),
                               PF(collision_penalty), PF(goal_reward), PF(discount), PF(min_start_goal_dis), PF(init_theta), PF(init_speed), PF(dt), PF(robot_r),
                               PF(max_speed), PF(a), PF(w), PF(sonar_range), PF(sonar_angle), PF(num_cores), PF(num_obs), PF(reset_start_and_goal),
                               PF(random_reset_state), PF(set_boundary), PF(max_episode_steps), PF(N), PF(num_beams)};
#undef PF
    for (const F &f : fields)
        if (memcmp((const char *)&b.params + f.off, (const char *)&m.params + f.off, f.size) != 0) return f.name;
    if (b.n_stages != m.n_stages) return "schedule.n_stages";
    if (memcmp(&b.timestep_scale, &m.timestep_scale, 8) != 0) return "schedule.timestep_scale";
    for (int i = 0; i < m.n_stages; ++i) {
        const char *what = b.sched_t[i] != m.sched_t[i] ? "timesteps" : b.sched_nc[i] != m.sched_nc[i] ? "num_cores" : b.sched_no[i] != m.sched_no[i] ? "num_obs"
                           : memcmp(&b.sched_md[i], &m.sched_md[i], 8) != 0 ? "min_start_goal_dis" : nullptr;
        if (what) { snprintf(buf, len, "schedule.%s[%d]", what, i); return buf; }
    }
    return nullptr;
}

extern "C" int64_t mn_state_bytes(const mn_handle *h) { return h ? mn_state_layout_bytes(h->A.n, h->A.qcap) : (int64_t)MN_ERR_INVALID; }

static int state_args_ok(mn_handle *h, const void *blob_dev, int64_t bytes, const char *who) {
    char b[200];
    if (!h) { snprintf(b, sizeof(b), "%s: NULL handle", who); return fail(nullptr, MN_ERR_INVALID, b); }
    if (!blob_dev) { snprintf(b, sizeof(b), "%s: blob_dev is NULL", who); return fail(h, MN_ERR_INVALID, b); }
    if ((uintptr_t)blob_dev & 15) { snprintf(b, sizeof(b), "%s: blob_dev must be 16-byte aligned (the RNG rows move as 128-bit vectors)", who); return fail(h, MN_ERR_INVALID, b); }
    const int64_t need = mn_state_layout_bytes(h->A.n, h->A.qcap);
    if (bytes < need) {
        snprintf(b, sizeof(b), "%s: the buffer has %lld bytes, the handle's state needs %lld (mn_state_bytes)", who, (long long)bytes, (long long)need);
        return fail(h, MN_ERR_INVALID, b);
    }
    return MN_OK;
}

extern "C" int mn_state_save(mn_handle *h, void *blob_dev, int64_t bytes, void *stream) {
    int rc = state_args_ok(h, blob_dev, bytes, "mn_state_save");
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    join_reset(h, s);      // an owed reset is launched here, a pending one joined: the snapshot is of the state every other entry point would see
    MN_ON_DEVICE(h);
    MnStateHeader hdr;
    state_header(h, &hdr);
    mn_launch_state(true, h->A, hdr, blob_dev, h->peak_dev, h->seen_dev, nullptr, s);
    MN_HIP(h, hipGetLastError());
    return MN_OK;
}

extern "C" int mn_state_load(mn_handle *h, const void *blob_dev, int64_t bytes, void *stream) {
    int rc = state_args_ok(h, blob_dev, bytes, "mn_state_load");
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    join_reset(h, s);
    MN_ON_DEVICE(h);
    MnStateHeader mine, blob;
    state_header(h, &mine);
    MN_HIP(h, hipMemcpyAsync(&blob, blob_dev, sizeof(blob), hipMemcpyDeviceToHost, s));
    MN_HIP(h, hipStreamSynchronize(s));
    char b[256], fb[64];
    if (blob.magic != MN_STATE_MAGIC) {
        snprintf(b, sizeof(b), "mn_state_load: not a state blob (magic word 0x%08x, expected 0x%08x)", blob.magic, MN_STATE_MAGIC);
        return fail(h, MN_ERR_INVALID, b);
    }
    if (blob.version != MN_STATE_VERSION) {
        snprintf(b, sizeof(b), "mn_state_load: blob format version %u, this library reads version %u", blob.version, MN_STATE_VERSION);
        return fail(h, MN_ERR_INVALID, b);
    }
    if (blob.n != mine.n) {
        snprintf(b, sizeof(b), "mn_state_load: the blob holds n = %d envs, the handle %d", blob.n, mine.n);
        return fail(h, MN_ERR_INVALID, b);
    }
    if (blob.precision != mine.precision) {
        snprintf(b, sizeof(b), "mn_state_load: the blob was saved with precision %d, the handle has %d", blob.precision, mine.precision);
        return fail(h, MN_ERR_INVALID, b);
    }
    if (blob.bytes != mine.bytes || blob.header_bytes != mine.header_bytes || blob.qcap != mine.qcap)
        return fail(h, MN_ERR_INVALID, "mn_state_load: the blob's byte count, header size or queue capacity is not what this library lays out for the handle");
    const char *diff = state_first_difference(blob, mine, fb, sizeof(fb));
    if (diff) {
        snprintf(b, sizeof(b), "mn_state_load: the blob was saved from a handle with another %s", diff);
        return fail(h, MN_ERR_INVALID, b);
    }
    // accepted: from here on the handle changes
    if (blob.has_peak && (rc = ensure_async(h)) != MN_OK) return rc;
    h->step_parity = blob.step_parity; h->last_parity = blob.last_parity;
    h->tick = blob.tick;
    h->under_act_max = blob.under_act_max; h->owed_max_rows = blob.owed_max_rows;
    if (h->seen_host) *h->seen_host = blob.seen;      // (the stream is idle: no reset launch of it is still to write the word)
    mn_launch_state(false, h->A, blob, const_cast<void *>(blob_dev), h->peak_dev, h->seen_dev, h->ready, s);
    MN_HIP(h, hipGetLastError());
    return MN_OK;
}

extern "C" int mn_get_obs64(mn_handle *h, int32_t first, int32_t count, double *out) {
    int rc = range_ok(h, first, count);
    if (rc) return rc;
    if (count == 0) return MN_OK;
    if (!out) return MN_ERR_INVALID;
    if (!h->A.obs64) return fail(h, MN_ERR_INVALID, "float64 observations are kept only with MN_PRECISION_F64 after mn_enable_obs64(h, 1)");
    MN_HIP(h, hipDeviceSynchronize());
    MN_HIP(h, hipMemcpy(out, h->A.obs64 + (size_t)first * MN_OBS_DIM, (size_t)count * MN_OBS_DIM * 8, hipMemcpyDeviceToHost));
    return MN_OK;
}

extern "C" int mn_get_reward64(mn_handle *h, int32_t first, int32_t count, double *out) {
    int rc = range_ok(h, first, count);
    if (rc) return rc;
    if (count == 0) return MN_OK;
    if (!out) return MN_ERR_INVALID;
    if (!h->A.rew64) return fail(h, MN_ERR_INVALID, "float64 rewards are kept only with MN_PRECISION_F64 after mn_enable_obs64(h, 1)");
    MN_HIP(h, hipDeviceSynchronize());
    MN_HIP(h, hipMemcpy(out, h->A.rew64 + first, (size_t)count * 8, hipMemcpyDeviceToHost));
    return MN_OK;
}

extern "C" int mn_enable_obs64(mn_handle *h, int32_t on) {
    if (!h || on < 0 || on > 1) return MN_ERR_INVALID;
    MN_ON_DEVICE(h);
    if (h->params.precision != MN_PRECISION_F64) return fail(h, MN_ERR_INVALID, "float64 observation copies exist only with MN_PRECISION_F64");
    MN_HIP(h, hipDeviceSynchronize());
    if (!on) { h->A.obs64 = nullptr; h->A.rew64 = nullptr; return sync_arrays(h); }      // the buffers stay owned by the handle
    if (!h->obs64_buf) {
        int rc = dev_alloc(h, &h->obs64_buf, (size_t)h->A.npad * MN_OBS_DIM);
        if (rc == MN_OK) rc = dev_alloc(h, &h->rew64_buf, (size_t)h->A.npad);
        if (rc) return rc;
    }
    h->A.obs64 = h->obs64_buf; h->A.rew64 = h->rew64_buf;
    return sync_arrays(h);
}

extern "C" int mn_enable_trajectory(mn_handle *h, int32_t max_substeps) {
    if (!h || max_substeps < 1 || max_substeps > 1000) return MN_ERR_INVALID;
    MN_ON_DEVICE(h);
    if (h->params.precision != MN_PRECISION_F64) return fail(h, MN_ERR_INVALID, "sub-step trajectories are recorded only with MN_PRECISION_F64");
    if (h->A.traj && h->A.traj_n >= max_substeps) return MN_OK;
    MN_HIP(h, hipDeviceSynchronize());
    int rc = dev_alloc(h, &h->A.traj, (size_t)h->A.npad * max_substeps * 2);   // an earlier, smaller buffer stays owned by the handle
    if (rc) return rc;
    h->A.traj_n = max_substeps;
    return sync_arrays(h);
}

extern "C" int mn_get_trajectory(mn_handle *h, int32_t first, int32_t count, int32_t n_substeps, double *out) {
    int rc = range_ok(h, first, count);
    if (rc) return rc;
    if (count == 0) return MN_OK;
    if (!out || n_substeps < 1) return MN_ERR_INVALID;
    if (!h->A.traj || n_substeps > h->A.traj_n) return fail(h, MN_ERR_INVALID, "call mn_enable_trajectory(h, >= n_substeps) before stepping");
    MN_HIP(h, hipDeviceSynchronize());
    MN_HIP(h, hipMemcpy2D(out, (size_t)n_substeps * 16, h->A.traj + (size_t)first * h->A.traj_n * 2, (size_t)h->A.traj_n * 16,
                          (size_t)n_substeps * 16, count, hipMemcpyDeviceToHost));
    return MN_OK;
}

extern "C" int mn_peek_next_double(mn_handle *h, int32_t first, int32_t count, double *out) {
    int rc = range_ok(h, first, count);
    if (rc) return rc;
    if (count == 0) return MN_OK;
    if (!out) return MN_ERR_INVALID;
    MN_HIP(h, hipDeviceSynchronize());
    mn_launch_peek(h->A, first, count, h->peek_scratch, nullptr);
    MN_HIP(h, hipGetLastError());
    MN_HIP(h, hipMemcpy(out, h->peek_scratch, (size_t)count * 8, hipMemcpyDeviceToHost));
    return MN_OK;
}

// Test hook: the first `bytes` bytes of one of the handle's raw device arrays, as they are (padding included) -- what no other accessor hands out: the RNG
// rows and positions, and the compact tables the mixed-precision step kernel reads.  Waits for the device first, like the other host accessors.
extern "C" int mn_debug_read(mn_handle *h, int32_t field, void *out, int64_t bytes) {
    if (!h || !out || bytes < 0) return MN_ERR_INVALID;
    MN_ON_DEVICE(h);
    const size_t np = (size_t)h->A.npad;
    const void *src[MN_DEBUG_N_FIELDS] = {h->A.mt, h->A.mt_pos, h->A.qcx, h->A.qcy, h->A.qcg, h->A.qox, h->A.qoy, h->A.qor};
    const size_t size[MN_DEBUG_N_FIELDS] = {np * MT_WORDS * 4, np * 4, np * MN_MAX_CORES * 4, np * MN_MAX_CORES * 4, np * MN_MAX_CORES * 4,
                                            np * MN_MAX_OBS * 4, np * MN_MAX_OBS * 4, np * MN_MAX_OBS * 4};
    if (field < 0 || field >= MN_DEBUG_N_FIELDS || (size_t)bytes > size[field]) return fail(h, MN_ERR_INVALID, "mn_debug_read: unknown field, or more bytes than it has");
    MN_HIP(h, hipDeviceSynchronize());
    MN_HIP(h, hipMemcpy(out, src[field], (size_t)bytes, hipMemcpyDeviceToHost));
    return MN_OK;
}

extern "C" int mn_profile_begin(mn_handle *h, int32_t max_launches) {
    if (!h || max_launches < 0) return MN_ERR_INVALID;
    while ((int)h->ev.size() < 2 * max_launches) {
        hipEvent_t e;
        MN_HIP(h, hipEventCreate(&e));
        h->ev.push_back(e);
    }
    while ((int)h->ev_reset.size() < 2 * max_launches) {
        hipEvent_t e;
        MN_HIP(h, hipEventCreate(&e));
        h->ev_reset.push_back(e);
    }
    h->prof_max = max_launches;
    h->prof_n = 0;
    h->prof_reset_n = 0;
    return MN_OK;
}

// The mn_reset_done launches of the same window (call BEFORE mn_profile_end, which closes the window).
extern "C" int mn_profile_reset_end(mn_handle *h, void *stream, double *mean_ms, int32_t *launches) {
    if (!h) return MN_ERR_INVALID;
    MN_HIP(h, hipStreamSynchronize((hipStream_t)stream));
    if (h->side) MN_HIP(h, hipStreamSynchronize(h->side));      // (launches of mn_reset_done_async are timed on the handle's own stream)
    double sum = 0.0;
    for (int i = 0; i < h->prof_reset_n; ++i) {
        float ms = 0.f;
        MN_HIP(h, hipEventElapsedTime(&ms, h->ev_reset[2 * i], h->ev_reset[2 * i + 1]));
        sum += ms;
    }
    if (mean_ms) *mean_ms = h->prof_reset_n ? sum / h->prof_reset_n : 0.0;
    if (launches) *launches = h->prof_reset_n;
    h->prof_reset_n = 0;
    return MN_OK;
}

extern "C" int mn_profile_end(mn_handle *h, void *stream, double *mean_ms, int32_t *launches) {
    if (!h) return MN_ERR_INVALID;
    MN_HIP(h, hipStreamSynchronize((hipStream_t)stream));
    double sum = 0.0;
    for (int i = 0; i < h->prof_n; ++i) {
        float ms = 0.f;
        MN_HIP(h, hipEventElapsedTime(&ms, h->ev[2 * i], h->ev[2 * i + 1]));
        sum += ms;
    }
    if (mean_ms) *mean_ms = h->prof_n ? sum / h->prof_n : 0.0;
    if (launches) *launches = h->prof_n;
    h->prof_max = 0;
    h->prof_n = 0;
    h->prof_reset_n = 0;
    return MN_OK;
}
