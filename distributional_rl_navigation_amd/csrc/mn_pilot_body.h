// mn_pilot_body.h -- the field pilot's decision rule for ONE robot in ONE world (gfx950; mn_pilot.hip): look H steps ahead with each of the nine
// actions under the real dynamics (mnq_step, mn_query_step_body.h: the reference's own float64 step) and score the landing point with the world's
// minimum-time-to-goal field T (mn_time_field), interpolated.  The global dynamic-window rule; stated operation for operation in
// include/marinenav_hip.h ("Field pilot").
//   candidate a:  copy the state, run mnq_step with action a and the counters t, t + 1, ... up to H times, stop behind the first step whose info
//                 is not MN_INFO_NORMAL -- what mn_query_rollout does with MN_QUERY_ACTIONS_CONSTANT, its per-step state check included.
//   score_a:      n_a step_time for REACH_GOAL; +inf for COLLISION, OUT_OF_BOUNDARY (and a state that left the finite numbers);
//                 n_a step_time + Tint(x_a, y_a) for NORMAL and TOO_LONG.  step_time = (double)N * dt.
//   choice:       the least key (score_a, H - n_a, a), lexicographic.
// Everything here is __host__ __device__ and holds no indexed private array: a candidate is a handful of scalars, the field is read where it is
// needed (`F.T(c)`: a global read on the device).  Every operation is an IEEE float64 add, multiply, divide, floor or comparison in the order
// written (contraction off), so host and device give the same words.
#pragma once
#include "mn_query_step_body.h"

struct MnpNoTraj {
    MNQ_HD void point(int, double, double) {}
};

// The interpolated field value at (x, y).  `F.T(c)` is the field's word of cell c = j nx + i.
template <class Field>
MNQ_HD double mnp_tint(const Field &F, int nx, int ny, const MnDev &P, double x, double y) {
    const double inf = (double)INFINITY;
    if (!(x >= 0.0 && x <= P.width && y >= 0.0 && y <= P.height)) return inf;      // (a NaN is outside)
    const double hx = P.width / (double)nx, hy = P.height / (double)ny;
    // the containing cell: floor, and the far edge belongs to the last cell (maps._cells_of)
    int i = (int)floor(x / hx), j = (int)floor(y / hy);
    i = i < 0 ? 0 : (i > nx - 1 ? nx - 1 : i);
    j = j < 0 ? 0 : (j > ny - 1 ? ny - 1 : j);
    double v = F.T(j * nx + i);
    if (nx > 1 && ny > 1) {
        const double u = x / hx - 0.5, w = y / hy - 0.5;
        int i0 = (int)floor(u), j0 = (int)floor(w);
        i0 = i0 < 0 ? 0 : (i0 > nx - 2 ? nx - 2 : i0);
        j0 = j0 < 0 ? 0 : (j0 > ny - 2 ? ny - 2 : j0);
        double fx = u - (double)i0, fy = w - (double)j0;
        fx = fx < 0.0 ? 0.0 : (fx > 1.0 ? 1.0 : fx);
        fy = fy < 0.0 ? 0.0 : (fy > 1.0 ? 1.0 : fy);
        const double T00 = F.T(j0 * nx + i0), T10 = F.T(j0 * nx + i0 + 1), T01 = F.T((j0 + 1) * nx + i0), T11 = F.T((j0 + 1) * nx + i0 + 1);
        if (fabs(T00) < inf && fabs(T10) < inf && fabs(T01) < inf && fabs(T11) < inf)
            v = (T00 * (1.0 - fx) + T10 * fx) * (1.0 - fy) + (T01 * (1.0 - fx) + T11 * fx) * fy;
    }
    return v == v ? v : inf;
}

// Candidate `action` from state `r` (stepped in place: it leaves as the end state) with the counter `t` before the first step.  The caller has
// checked mnq_state_ok(r) and 1 <= H.  Returns the score; n = the steps run, info = the last step's code.
template <class Cores, class World, class Field>
MNQ_HD double mnp_candidate(const Cores &cs, const World &w, int no, double gx, double gy, const MnDev &P, const Field &F, int nx, int ny, int H,
                            int action, int t, MnqRobot &r, int &n, int &info) {
    MnpNoTraj traj;
    double reward;
    n = 0;
    info = MN_INFO_NORMAL;
    for (int k = 0; k < H; ++k) {
        n = k + 1;
        if (!mnq_state_ok(r)) { info = MN_QUERY_INFO_BAD_STATE; break; }      // (a position on a vortex core: mn_query_rollout's rule)
        info = mnq_step(cs, w, no, gx, gy, P, action, t + k, r, reward, traj);
        if (info != MN_INFO_NORMAL) break;
    }
    const double step_time = (double)P.N * P.dt;
    const double base = (double)n * step_time;
    if (info == MN_INFO_REACH_GOAL) return base;
    if (info == MN_INFO_NORMAL || info == MN_INFO_TOO_LONG) return base + mnp_tint(F, nx, ny, P, r.x, r.y);
    return (double)INFINITY;
}

// key (score, rem = H - n, a) < key (bscore, brem, ba), lexicographic.  Scores are never NaN.
MNQ_HD bool mnp_better(double score, int rem, int a, double bscore, int brem, int ba) {
    return score < bscore || (score == bscore && (rem < brem || (rem == brem && a < ba)));
}
