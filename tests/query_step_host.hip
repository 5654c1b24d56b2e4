// query_step_host.hip -- the what-if step of csrc/mn_query_step_body.h on the CPU: a stand-alone program for
// tests/test_query_step_cpu.py (hipcc --cuda-host-only -ffp-contract=off; the body is __host__ __device__, so this is the arithmetic
// the kernel runs, compiled for the host).  No GPU call is made.
//
//   query_step_host IN OUT
// IN:  int32 n_rows, int32 pad, mn_params (raw), then n_rows records of
//        int32 n_cores, n_obs, action, episode_timesteps; double cores[8][3] (x, y, +Gamma if clockwise else -Gamma),
//        obstacles[10][3] (x, y, r), goal[2], state[6]
// OUT: n_rows records of 35 doubles: state[6], obs[26], reward, done, info
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "mn_query_step_body.h"

struct Record {
    int32_t nc, no, action, ep_t;
    double cores[MN_MAX_CORES][3], obst[MN_MAX_OBS][3], goal[2], state[6];
};

struct HostWorld {
    const double (*o)[3];
    void obstacle(int k, double &x, double &y, double &r) const { x = o[k][0]; y = o[k][1]; r = o[k][2]; }
};
struct HostRow {
    double *o;
    void head(double a, double b, double c, double d) { o[0] = a; o[1] = b; o[2] = c; o[3] = d; }
    void beam(int i, double bx, double by) { o[4 + 2 * i] = bx; o[5 + 2 * i] = by; }
};
struct HostCores {
    const MnqCores &W;
    void cores(MnqCores &out) const { out = W; }
};
struct NoTraj {
    void point(int, double, double) {}
};

// the fields of MnDev the query body reads, as mn_capi.hip's derive() forms them
static void derive(const mn_params &p, MnDev &d) {
    memset(&d, 0, sizeof(d));
    d.width = p.width; d.height = p.height; d.core_r = p.core_r; d.goal_dis = p.goal_dis;
    d.timestep_penalty = p.timestep_penalty; d.collision_penalty = p.collision_penalty; d.goal_reward = p.goal_reward;
    d.dt = p.dt; d.robot_r = p.robot_r; d.max_speed = p.max_speed;
    double amax = p.a[0];
    for (int i = 0; i < 3; ++i) { d.a[i] = p.a[i]; d.w[i] = p.w[i]; if (p.a[i] > amax) amax = p.a[i]; }
    d.k_drag = amax / p.max_speed;
    d.sonar_range = p.sonar_range;
    const double phi = p.sonar_angle / (p.num_beams - 1), a0 = -p.sonar_angle / 2;
    for (int i = 0; i < MN_NUM_BEAMS; ++i) d.beam_rel[i] = a0 + i * phi;
    d.two_pi = 2 * M_PI;
    d.two_pi_r_r = 2 * M_PI * p.core_r * p.core_r;
    d.set_boundary = p.set_boundary; d.max_episode_steps = p.max_episode_steps; d.N = p.N;
}

int main(int argc, char **argv) {
    if (argc != 3) { fprintf(stderr, "usage: %s IN OUT\n", argv[0]); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    int32_t head[2];
    mn_params p;
    if (fread(head, sizeof(head), 1, f) != 1 || fread(&p, sizeof(p), 1, f) != 1 || head[0] < 0) { fprintf(stderr, "short header\n"); return 2; }
    std::vector<Record> rec((size_t)head[0]);
    if (head[0] && fread(rec.data(), sizeof(Record), rec.size(), f) != rec.size()) { fprintf(stderr, "short file\n"); return 2; }
    fclose(f);
    if (p.num_beams != MN_NUM_BEAMS || p.N < 1 || p.N > 1000) { fprintf(stderr, "bad parameters\n"); return 2; }
    MnDev P;
    derive(p, P);
    std::vector<double> out(rec.size() * 35);
    for (size_t i = 0; i < rec.size(); ++i) {
        const Record &r = rec[i];
        double *o = &out[i * 35];
        if (r.nc < 0 || r.nc > MN_MAX_CORES || r.no < 0 || r.no > MN_MAX_OBS) { fprintf(stderr, "record %zu: bad counts\n", i); return 2; }
        MnqCores W;
        W.nc = r.nc;
        for (int k = 0; k < MN_MAX_CORES; ++k) { W.cx[k] = r.cores[k][0]; W.cy[k] = r.cores[k][1]; W.cg[k] = r.cores[k][2]; }
        const HostWorld w = {r.obst};
        MnqRobot rb = {r.state[0], r.state[1], r.state[2], r.state[3], r.state[4], r.state[5]};
        HostRow row = {o + 6};
        NoTraj traj;
        double reward = __builtin_nan("");
        int info = MN_QUERY_INFO_BAD_STATE;
        if (mnq_state_ok(rb) && r.action >= 0 && r.action < MN_NUM_ACTIONS) {
            info = mnq_step(HostCores{W}, w, r.no, r.goal[0], r.goal[1], P, r.action, r.ep_t, rb, reward, traj);
            mnq_observe(w, r.no, r.goal[0], r.goal[1], P, rb.x, rb.y, rb.theta, rb.vx, rb.vy, row);
        } else {
            for (int k = 0; k < 35; ++k) o[k] = __builtin_nan("");
            rb = {o[0], o[0], o[0], o[0], o[0], o[0]};
        }
        o[0] = rb.x; o[1] = rb.y; o[2] = rb.theta; o[3] = rb.speed; o[4] = rb.vx; o[5] = rb.vy;
        o[32] = reward; o[33] = info != MN_INFO_NORMAL; o[34] = info;
    }
    f = fopen(argv[2], "wb");
    if (!f) { perror(argv[2]); return 2; }
    if (!out.empty() && fwrite(out.data(), sizeof(double), out.size(), f) != out.size()) { fprintf(stderr, "short write\n"); return 2; }
    fclose(f);
    return 0;
}
