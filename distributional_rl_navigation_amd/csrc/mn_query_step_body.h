// mn_query_step_body.h -- ONE MarineNavEnv.step of ONE robot placed by hand in ONE world, without a handle row behind it
// (gfx950; mn_query_step.hip).
//
// Restates MarineNavEnv.step (marinenav_env.py:199-262) with Robot.update_state (robot.py:102-123) LITERALLY, in the reference's
// order, on top of the pieces of mn_query_body.h: the same float64 operations as the reference, not the step
// kernel's well-conditioned forms (mn_step_body.h), so a what-if step is held to the reference to 1e-9 on every output.
//   dis_before -> N x (current at the pre-move position, velocity from the pre-update speed and heading, move, speed with drag and
//   clip, heading and wrap) -> dis_after -> reward -> the termination ladder (boundary, too long, collision, goal).
// The observation of the state a step leaves is mnq_observe(x, y, theta, vx, vy): (vx, vy) is the LAGGING velocity, the one the
// last sub-step moved with, rotated by the FINAL heading.  It is not part of mnq_step: the ladder needs only the flag bits, which
// mnq_flags forms by the same operations as mnq_observe's first pass, so a caller runs the sonar only where a row leaves.
// Everything here is __host__ __device__ and holds no indexed private array (see mn_query_body.h).
#pragma once
#include "mn_query_body.h"

// x, y, theta, speed, velocity_x, velocity_y: the columns of mn_get_state
struct MnqRobot { double x, y, theta, speed, vx, vy; };

// The reference wraps the heading with `while` loops (robot.py:120-123): a heading given by hand must not be able to spin a lane,
// so a state with a non-finite component or |theta| >= MNQ_THETA_MAX is not stepped (at most 1.6e5 turns of the loop below that).
// The velocity columns are not looked at: a step overwrites them before it reads them.
#define MNQ_THETA_MAX 1.0e6
MNQ_HD bool mnq_state_ok(const MnqRobot &r) {
    const double inf = (double)INFINITY;
    return fabs(r.x) < inf && fabs(r.y) < inf && fabs(r.speed) < inf && fabs(r.theta) < MNQ_THETA_MAX;
}

// The flag bits of a pose without the sonar: mnq_observe's first pass (check_collision, marinenav_env.py:329-336: only the obstacle
// with the NEAREST CENTRE is tested, first of equals; out_of_boundary; check_reach_goal :338-342), operation for operation.
template <class World>
MNQ_HD unsigned mnq_flags(const World &w, int no, double gx, double gy, const MnDev &P, double x, double y) {
    double bd2 = (double)INFINITY, br = 0.0;      // (nearest by the SQUARED distance: see mnq_observe)
    no = no < MN_MAX_OBS ? no : MN_MAX_OBS;
    for (int k = 0; k < no; ++k) {
        double ox, oy, orad;
        w.obstacle(k, ox, oy, orad);
        const double dx = ox - x, dy = oy - y;
        const double d2 = dx * dx + dy * dy;
        if (d2 < bd2) { bd2 = d2; br = orad; }
    }
    unsigned flags = 0;
    if (no > 0 && sqrt(bd2) <= br + P.robot_r) flags |= MN_QUERY_FLAG_COLLISION;
    if ((x < 0.0 || x > P.width) || (y < 0.0 || y > P.height)) flags |= MN_QUERY_FLAG_OUTSIDE;
    const double gdx = x - gx, gdy = y - gy;
    if (sqrt(gdx * gdx + gdy * gdy) <= P.goal_dis) flags |= MN_QUERY_FLAG_GOAL;
    return flags;
}

// One step.  `r` is stepped in place (r.vx, r.vy leave as the lagging velocity), `episode_timesteps` is the counter BEFORE the
// step's increment, `traj.point(i, x, y)` receives the position after sub-step i (marinenav_env.py:211-212).  The caller has
// checked mnq_state_ok(r) and 0 <= action < MN_NUM_ACTIONS.  Returns the info code (done = code != MN_INFO_NORMAL).
// `cs.cores(W)` hands out the world's cores once per sub-step: a holder that keeps them (scalar registers, host memory) copies them,
// one that does not (a world per lane on the device) reads the tables again instead of keeping 48 vector registers over the rollout.
template <class Cores, class World, class Traj>
MNQ_HD int mnq_step(const Cores &cs, const World &w, int no, double gx, double gy, const MnDev &P, int action, int episode_timesteps, MnqRobot &r,
                    double &reward_out, Traj &traj) {
    const int ai = action / 3, wi = action - 3 * ai;      // robot.py:55-56: actions = [(a, w) for a in self.a for w in self.w]
    const double acc = ai == 0 ? P.a[0] : (ai == 1 ? P.a[1] : P.a[2]);
    const double om = wi == 0 ? P.w[0] : (wi == 1 ? P.w[1] : P.w[2]);
    const double two_pi = 2 * 3.141592653589793;
    const double b0x = gx - r.x, b0y = gy - r.y;
    const double dis_before = sqrt(b0x * b0x + b0y * b0y);      // dist_to_goal
    for (int i = 0; i < P.N; ++i) {
        double cvx, cvy;
        MnqCores W;
        cs.cores(W);
        mnq_velocity(W, P, r.x, r.y, cvx, cvy);
        // robot.py:102-123
        r.vx = r.speed * cos(r.theta) + cvx;
        r.vy = r.speed * sin(r.theta) + cvy;
        r.x += r.vx * P.dt;
        r.y += r.vy * P.dt;
        r.speed += (acc - P.k_drag * r.speed) * P.dt;
        if (r.speed < 0.0) r.speed = 0.0;      // np.clip
        if (r.speed > P.max_speed) r.speed = P.max_speed;
        r.theta += om * P.dt;
        while (r.theta < 0.0) r.theta += two_pi;
        while (r.theta >= two_pi) r.theta -= two_pi;
        traj.point(i, r.x, r.y);
    }
    const double b1x = gx - r.x, b1y = gy - r.y;
    const double dis_after = sqrt(b1x * b1x + b1y * b1y);
    double reward = P.timestep_penalty;
    reward += dis_before - dis_after;
    const unsigned f = mnq_flags(w, no, gx, gy, P, r.x, r.y);
    int info = MN_INFO_NORMAL;
    if (P.set_boundary && (f & MN_QUERY_FLAG_OUTSIDE)) info = MN_INFO_OUT_OF_BOUNDARY;
    else if (episode_timesteps >= P.max_episode_steps) info = MN_INFO_TOO_LONG;
    else if (f & MN_QUERY_FLAG_COLLISION) { reward += P.collision_penalty; info = MN_INFO_COLLISION; }
    else if (f & MN_QUERY_FLAG_GOAL) { reward += P.goal_reward; info = MN_INFO_REACH_GOAL; }
    reward_out = reward;
    return info;
}
