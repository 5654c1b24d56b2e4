// pilot_host.hip -- the field pilot's rule (csrc/mn_pilot_body.h on csrc/mn_query_step_body.h) on the CPU: a stand-alone program for
// tests/test_pilot_cpu.py and the reference count of tests/test_pilot_gpu.py (hipcc --cuda-host-only -ffp-contract=off; the bodies are
// __host__ __device__, so this is the arithmetic the kernels run, compiled for the host).  No GPU call is made.
//
//   pilot_host [--episodes] IN OUT
// IN:  int32 n_worlds, n_fields, nx, ny, H, n_queries, max_steps, pad; mn_params (raw); n_worlds records of int32 n_cores, n_obs (n_cores < 0: no
//      such world), double cores[8][3] (x, y, +Gamma if clockwise else -Gamma), obstacles[10][3] (x, y, r), start[2], goal[2]; the fields, double
//      [n_fields][ny][nx] (the time-field host program's T); n_queries records of int32 world, field, episode_timesteps, pad, double state[6].
// OUT: per query double end[9][6] (the nine end states), score[9], tint[9] (Tint at the nine end positions), int32 n[9], info[9], action, flag.
//      A poisoned query: NaN doubles, n 0, info = flag, action -1.
// --episodes: every query is an episode's start; the pilot drives it with mnq_step for at most max_steps steps.
// OUT: per query int32 success, steps, info (the last step's), flag, then int32 actions[max_steps] (-1 behind the end).
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "mn_pilot_body.h"

struct WorldRec {
    int32_t nc, no;
    double cores[MN_MAX_CORES][3], obst[MN_MAX_OBS][3], start[2], goal[2];
};
struct QueryRec {
    int32_t world, field, ep_t, pad;
    double state[6];
};
struct OutRec {
    double end[MN_NUM_ACTIONS][6], score[MN_NUM_ACTIONS], tint[MN_NUM_ACTIONS];
    int32_t n[MN_NUM_ACTIONS], info[MN_NUM_ACTIONS], action, flag;
};
struct HostWorld {
    const double (*o)[3];
    void obstacle(int k, double &x, double &y, double &r) const { x = o[k][0]; y = o[k][1]; r = o[k][2]; }
};
struct HostCores {
    const MnqCores &W;
    void cores(MnqCores &out) const { out = W; }
};
struct HostField {
    const double *t;
    double T(int c) const { return t[c]; }
};

// the fields of MnDev the bodies read, as mn_capi.hip's derive() forms them
static void derive(const mn_params &p, MnDev &d) {
    memset(&d, 0, sizeof(d));
    d.width = p.width; d.height = p.height; d.core_r = p.core_r; d.goal_dis = p.goal_dis;
    d.timestep_penalty = p.timestep_penalty; d.collision_penalty = p.collision_penalty; d.goal_reward = p.goal_reward;
    d.dt = p.dt; d.robot_r = p.robot_r; d.max_speed = p.max_speed;
    double amax = p.a[0];
    for (int i = 0; i < 3; ++i) { d.a[i] = p.a[i]; d.w[i] = p.w[i]; if (p.a[i] > amax) amax = p.a[i]; }
    d.k_drag = amax / p.max_speed;
    d.two_pi = 2 * M_PI;
    d.two_pi_r_r = 2 * M_PI * p.core_r * p.core_r;
    d.set_boundary = p.set_boundary; d.max_episode_steps = p.max_episode_steps; d.N = p.N;
}

struct Pilot {
    const MnDev &P;
    const std::vector<WorldRec> &worlds;
    const std::vector<double> &fields;
    int n_fields, nx, ny, H;

    int flag_of(const QueryRec &q) const {
        const MnqRobot r = {q.state[0], q.state[1], q.state[2], q.state[3], q.state[4], q.state[5]};
        if (q.world < 0 || q.world >= (int)worlds.size() || worlds[q.world].nc < 0) return MN_QUERY_FLAG_BAD_ENV;
        if (q.field < 0 || q.field >= n_fields) return MN_PILOT_FLAG_BAD_FIELD;
        if (!mnq_state_ok(r)) return MN_QUERY_INFO_BAD_STATE;
        const double t0 = fields[(size_t)q.field * nx * ny];
        return t0 != t0 ? MN_PILOT_FLAG_BAD_FIELD : 0;
    }
    // the nine candidates of a healthy query and the choice
    int act(const QueryRec &q, const MnqRobot &r0, int t, OutRec *o) const {
        const WorldRec &wr = worlds[q.world];
        MnqCores W;
        W.nc = wr.nc;
        for (int k = 0; k < MN_MAX_CORES; ++k) { W.cx[k] = wr.cores[k][0]; W.cy[k] = wr.cores[k][1]; W.cg[k] = wr.cores[k][2]; }
        const HostWorld w = {wr.obst};
        const HostField F = {&fields[(size_t)q.field * nx * ny]};
        double bs = 0.0;
        int brem = 0, ba = -1;
        for (int a = 0; a < MN_NUM_ACTIONS; ++a) {
            MnqRobot r = r0;
            int n, info;
            const double score = mnp_candidate(HostCores{W}, w, wr.no, wr.goal[0], wr.goal[1], P, F, nx, ny, H, a, t, r, n, info);
            if (ba < 0 || mnp_better(score, H - n, a, bs, brem, ba)) { bs = score; brem = H - n; ba = a; }
            if (o) {
                const double e[6] = {r.x, r.y, r.theta, r.speed, r.vx, r.vy};
                memcpy(o->end[a], e, sizeof(e));
                o->score[a] = score; o->tint[a] = mnp_tint(F, nx, ny, P, r.x, r.y); o->n[a] = n; o->info[a] = info;
            }
        }
        return ba;
    }
    int step(const QueryRec &q, int action, int t, MnqRobot &r) const {
        const WorldRec &wr = worlds[q.world];
        MnqCores W;
        W.nc = wr.nc;
        for (int k = 0; k < MN_MAX_CORES; ++k) { W.cx[k] = wr.cores[k][0]; W.cy[k] = wr.cores[k][1]; W.cg[k] = wr.cores[k][2]; }
        const HostWorld w = {wr.obst};
        MnpNoTraj traj;
        double reward;
        return mnq_step(HostCores{W}, w, wr.no, wr.goal[0], wr.goal[1], P, action, t, r, reward, traj);
    }
};

int main(int argc, char **argv) {
    const bool episodes = argc == 4 && !strcmp(argv[1], "--episodes");
    if (argc != 3 && !episodes) { fprintf(stderr, "usage: %s [--episodes] IN OUT\n", argv[0]); return 2; }
    const char *in = argv[argc - 2], *out_path = argv[argc - 1];
    FILE *f = fopen(in, "rb");
    if (!f) { perror(in); return 2; }
    int32_t head[8];
    mn_params p;
    if (fread(head, sizeof(head), 1, f) != 1 || fread(&p, sizeof(p), 1, f) != 1) { fprintf(stderr, "short header\n"); return 2; }
    const int n_worlds = head[0], n_fields = head[1], nx = head[2], ny = head[3], H = head[4], nq = head[5], max_steps = head[6];
    if (n_worlds < 1 || n_fields < 1 || nx < 1 || ny < 1 || (int64_t)nx * ny > MN_TIME_FIELD_MAX_CELLS || H < 1 || H > MN_PILOT_MAX_HORIZON || nq < 0 ||
        (episodes && max_steps < 1) || p.N < 1 || p.N > 1000) {
        fprintf(stderr, "arguments mn_pilot_act would refuse\n"); return 2;
    }
    std::vector<WorldRec> worlds((size_t)n_worlds);
    std::vector<double> fields((size_t)n_fields * nx * ny);
    std::vector<QueryRec> qs((size_t)nq);
    if (fread(worlds.data(), sizeof(WorldRec), worlds.size(), f) != worlds.size() || fread(fields.data(), 8, fields.size(), f) != fields.size() ||
        (nq && fread(qs.data(), sizeof(QueryRec), qs.size(), f) != qs.size())) { fprintf(stderr, "short file\n"); return 2; }
    fclose(f);
    for (const WorldRec &w : worlds)
        if (w.nc > MN_MAX_CORES || w.no < 0 || w.no > MN_MAX_OBS) { fprintf(stderr, "bad counts\n"); return 2; }
    MnDev P;
    derive(p, P);
    const Pilot pilot = {P, worlds, fields, n_fields, nx, ny, H};
    f = fopen(out_path, "wb");
    if (!f) { perror(out_path); return 2; }
    const double nan = __builtin_nan("");
    if (!episodes) {
        std::vector<OutRec> out((size_t)nq);
        for (int i = 0; i < nq; ++i) {
            const QueryRec &q = qs[i];
            OutRec &o = out[i];
            const int flag = pilot.flag_of(q);
            o.flag = flag;
            if (flag) {
                for (int a = 0; a < MN_NUM_ACTIONS; ++a) {
                    for (int k = 0; k < 6; ++k) o.end[a][k] = nan;
                    o.score[a] = nan; o.tint[a] = nan; o.n[a] = 0; o.info[a] = flag;
                }
                o.action = -1;
                continue;
            }
            const MnqRobot r = {q.state[0], q.state[1], q.state[2], q.state[3], q.state[4], q.state[5]};
            o.action = pilot.act(q, r, q.ep_t, &o);
        }
        if (nq && fwrite(out.data(), sizeof(OutRec), out.size(), f) != out.size()) { fprintf(stderr, "short write\n"); return 2; }
    } else {
        std::vector<int32_t> out((size_t)nq * (4 + max_steps), -1);
        for (int i = 0; i < nq; ++i) {
            const QueryRec &q = qs[i];
            int32_t *o = &out[(size_t)i * (4 + max_steps)];
            const int flag = pilot.flag_of(q);
            o[0] = 0; o[1] = 0; o[2] = flag ? MN_QUERY_INFO_BAD_STATE : MN_INFO_NORMAL; o[3] = flag;
            if (flag) continue;
            MnqRobot r = {q.state[0], q.state[1], q.state[2], q.state[3], q.state[4], q.state[5]};
            int t = q.ep_t, info = MN_INFO_NORMAL, steps = 0;
            while (steps < max_steps && info == MN_INFO_NORMAL) {
                if (!mnq_state_ok(r)) { info = MN_QUERY_INFO_BAD_STATE; break; }
                const int a = pilot.act(q, r, t, nullptr);
                info = pilot.step(q, a, t, r);
                o[4 + steps] = a;
                ++steps; ++t;
            }
            o[0] = info == MN_INFO_REACH_GOAL; o[1] = steps; o[2] = info;
        }
        if (fwrite(out.data(), 4, out.size(), f) != out.size()) { fprintf(stderr, "short write\n"); return 2; }
    }
    fclose(f);
    return 0;
}
