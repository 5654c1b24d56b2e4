// mn_query_body.h -- the current field and the observation of ONE pose in ONE world, without stepping it (gfx950; mn_query.hip).
//
// Restates MarineNavEnv.get_velocity (marinenav_env.py:422-455) and get_observation (marinenav_env.py:273-326 with
// Robot.sonar_reflection, robot.py:125-198) LITERALLY: the same float64 operations in the same order as the reference, not the
// well-conditioned forms of the step kernel (mn_step_body.h).  The step kernel may pick its own arithmetic because it is held to the
// reference only to 1e-9 + 1e-12 K^2 on a beam of slope K = tan(angle); the queries are held to 1e-9 on every beam, the
// near-vertical ones included, where the reference's own slope form is 1e-7 away from the geometry: agreeing with it there means
// making ITS rounding errors, which are a function of the operands bit for bit.  Every operation below is an IEEE float64 add,
// multiply, divide or square root (correctly rounded on the device as on the host, contraction off), except tan / cos / sin:
//   * cos / sin enter only the rotation into the robot frame (an ulp there is 1e-14 m) and the sign test of robot.py:188;
//   * tan is the slope K, and an ulp of K re-rolls the slope form's rounding errors (3e-8 m at K = 667).  OCML's tan is not
//     correctly rounded, the host libm's practically is: mnq_tan evaluates tan in double-double arithmetic (relative error
//     ~2^-68 before the one final rounding), which gives the correctly rounded slope in all but ~1 of 10^4 arguments.
// Everything here is __host__ __device__.  The cores are indexed with compile-time constants only (fully unrolled loops) and the
// obstacles are read where they are needed, so the device build holds no indexed array: no scratch, no LDS.
#pragma once
#include <math.h>

#include "mn_internal.h"

#define MNQ_HD __host__ __device__ __forceinline__

// The vortex cores of one world, as the float64 master tables hold them (rows beyond the placed count are never used).
struct MnqCores {
    double cx[MN_MAX_CORES], cy[MN_MAX_CORES], cg[MN_MAX_CORES];   // cg = +Gamma if clockwise else -Gamma
    int nc;
};
// The obstacles are not held at all: mnq_observe asks its `World` for obstacle k when it needs it (w.obstacle(k, ox, oy, r): a
// table read on the device), because of a world's ten only the few within sonar reach of the pose are ever looked at twice.

// ---- double-double helpers (error-free transformations; need -ffp-contract=off, which the whole library has) -------------------
struct MnqDD { double hi, lo; };
MNQ_HD MnqDD mnq_two_sum(double a, double b) { const double s = a + b, bb = s - a; return {s, (a - (s - bb)) + (b - bb)}; }
MNQ_HD MnqDD mnq_quick_two_sum(double a, double b) { const double s = a + b; return {s, b - (s - a)}; }   // |a| >= |b|
MNQ_HD MnqDD mnq_dd_add(MnqDD a, MnqDD b) { const MnqDD s = mnq_two_sum(a.hi, b.hi); return mnq_quick_two_sum(s.hi, s.lo + (a.lo + b.lo)); }
MNQ_HD MnqDD mnq_dd_mul(MnqDD a, MnqDD b) {
    const double p = a.hi * b.hi;
    const double e = fma(a.hi, b.hi, -p) + (a.hi * b.lo + a.lo * b.hi);
    return mnq_quick_two_sum(p, e);
}
MNQ_HD MnqDD mnq_dd_mul_d(MnqDD a, double b) {
    const double p = a.hi * b;
    return mnq_quick_two_sum(p, fma(a.hi, b, -p) + a.lo * b);
}
// num / den rounded once to float64
MNQ_HD double mnq_dd_div(MnqDD num, MnqDD den) {
    const double q1 = num.hi / den.hi;
    const double p = q1 * den.hi, pe = fma(q1, den.hi, -p);
    const double rem = (((num.hi - p) - pe) + num.lo) - q1 * den.lo;
    return q1 + rem / den.hi;
}

// tan(a), correctly rounded in practice (see the head of this file).  Reduction a = k pi/2 + r, |r| <= pi/4, by Cody-Waite with a
// 33 + 33 + 53 bit pi/2 (k P1 and k P2 are exact for |k| < 2^20); sin r and cos r by their Taylor series in r^2, the first three
// correction terms in double-double, the tail (below 2^-18 of the result) in float64; tan = sin / cos or -cos / sin.
// |a| >= 1e6, infinities and NaN: the runtime's tan (a heading is wrapped into [0, 2 pi) by every step; the fan adds +-pi/3).
MNQ_HD double mnq_tan(double a) {
    if (!(fabs(a) < 1.0e6)) return tan(a);
    const double P1 = 0x1.921fb54400000p+0, P2 = 0x1.0b4611a600000p-34, P3 = 0x1.3198a2e037073p-69;
    const double k = rint(a * 0x1.45f306dc9c883p-1);
    const MnqDD t0 = mnq_two_sum(a, -(k * P1));
    const MnqDD t1 = mnq_two_sum(t0.hi, -(k * P2));
    const double p3 = k * P3, p3e = fma(k, P3, -p3);
    const MnqDD t2 = mnq_two_sum(t1.hi, -p3);
    const MnqDD r = mnq_quick_two_sum(t2.hi, ((t0.lo + t1.lo) + t2.lo) - p3e);
    const MnqDD x2 = mnq_dd_mul(r, r);
    const double z = x2.hi;
    // sin r = r + r * (x2 * (-1/3! + x2 * (1/5! + x2 * (-1/7! + x2 * Ts(z)))))
    double ts = 0x1.71b8ef6dcf572p-66;                      // 1/21!
    ts = fma(ts, z, -0x1.2f49b46814157p-57);                // 1/19!
    ts = fma(ts, z, 0x1.952c77030ad4ap-49);                 // 1/17!
    ts = fma(ts, z, -0x1.ae7f3e733b81fp-41);                // 1/15!
    ts = fma(ts, z, 0x1.6124613a86d09p-33);                 // 1/13!
    ts = fma(ts, z, -0x1.ae64567f544e4p-26);                // 1/11!
    ts = fma(ts, z, 0x1.71de3a556c734p-19);                 // 1/9!
    MnqDD ps = mnq_dd_add({-0x1.a01a01a01a01ap-13, -0x1.a01a01a01a01ap-73}, mnq_dd_mul_d(x2, ts));
    ps = mnq_dd_add({0x1.1111111111111p-7, 0x1.1111111111111p-63}, mnq_dd_mul(x2, ps));
    ps = mnq_dd_add({-0x1.5555555555555p-3, -0x1.5555555555555p-57}, mnq_dd_mul(x2, ps));
    const MnqDD sn = mnq_dd_add(r, mnq_dd_mul(r, mnq_dd_mul(x2, ps)));
    // 1 - cos r = x2 * (1/2! - x2 * (1/4! - x2 * (1/6! - x2 * U(z)))), U = 1/8! - z/10! + ...; tc = -U, and the nesting below
    // carries the alternating sign in the stored constants: 1/6! + x2 tc, then -(1/4!) + x2 (.), then 1/2! + x2 (.)
    double tc = 0x1.0ce396db7f853p-70;                      // 1/22!
    tc = fma(tc, z, -0x1.e542ba4020225p-62);                // 1/20!
    tc = fma(tc, z, 0x1.6827863b97d97p-53);                 // 1/18!
    tc = fma(tc, z, -0x1.ae7f3e733b81fp-45);                // 1/16!
    tc = fma(tc, z, 0x1.93974a8c07c9dp-37);                 // 1/14!
    tc = fma(tc, z, -0x1.1eed8eff8d898p-29);                // 1/12!
    tc = fma(tc, z, 0x1.27e4fb7789f5cp-22);                 // 1/10!
    tc = fma(tc, z, -0x1.a01a01a01a01ap-16);                // 1/8!
    MnqDD pc = mnq_dd_add({0x1.6c16c16c16c17p-10, -0x1.f49f49f49f49fp-65}, mnq_dd_mul_d(x2, tc));
    pc = mnq_dd_add({-0x1.5555555555555p-5, -0x1.5555555555555p-59}, mnq_dd_mul(x2, pc));
    pc = mnq_dd_add({0.5, 0.0}, mnq_dd_mul(x2, pc));
    const MnqDD xc = mnq_dd_mul(x2, pc);                     // = 1 - cos r
    const MnqDD cs = mnq_dd_add({1.0, 0.0}, {-xc.hi, -xc.lo});
    const long long ki = (long long)k;
    if (ki & 1) return mnq_dd_div({-cs.hi, -cs.lo}, sn);
    return mnq_dd_div(sn, cs);
}

// ---- get_velocity (marinenav_env.py:422-455) ------------------------------------------------------------------------------------
// The reference adds the cores up nearest first (the KDTree query only fixes that order; its "occlusion" loop :437-442 never
// skips a core).  A core's contribution does not depend on the order, so the eight contributions are formed
// first and then sorted by (distance, generation index) -- a 19-comparator network, every index a constant -- and added in order.
MNQ_HD void mnq_cmpx(double &da, int &ka, double &xa, double &ya, double &db, int &kb, double &xb, double &yb) {
    const bool sw = (db < da) || (db == da && kb < ka);
    const double d0 = sw ? db : da, d1 = sw ? da : db, x0 = sw ? xb : xa, x1 = sw ? xa : xb, y0 = sw ? yb : ya, y1 = sw ? ya : yb;
    const int k0 = sw ? kb : ka, k1 = sw ? ka : kb;
    da = d0; db = d1; xa = x0; xb = x1; ya = y0; yb = y1; ka = k0; kb = k1;
}
MNQ_HD void mnq_velocity(const MnqCores &W, const MnDev &P, double x, double y, double &vx_out, double &vy_out) {
    static_assert(MN_MAX_CORES == 8, "the sorting network below is the one for eight keys");
    double d[MN_MAX_CORES], ux[MN_MAX_CORES], uy[MN_MAX_CORES];
    int id[MN_MAX_CORES];
#pragma unroll
    for (int i = 0; i < MN_MAX_CORES; ++i) {
        double rx = W.cx[i] - x, ry = W.cy[i] - y;
        const double dis = sqrt(rx * rx + ry * ry);
        rx /= dis; ry /= dis;
        const bool clockwise = W.cg[i] > 0.0;
        const double Gamma = fabs(W.cg[i]);
        // marinenav_env.py:444-449: tangent = R rx, R = [[0,-1],[1,0]] (clockwise) or [[0,1],[-1,0]]
        const double tx = clockwise ? 0. * rx + -1. * ry : 0. * rx + 1. * ry;
        const double ty = clockwise ? 1. * rx + 0. * ry : -1. * rx + 0. * ry;
        // compute_speed (:461-465)
        const double speed = dis <= P.core_r ? Gamma / P.two_pi_r_r * dis : Gamma / (P.two_pi * dis);
        const bool placed = i < W.nc;
        d[i] = placed ? dis : (double)INFINITY;      // missing cores sort last and add +0
        ux[i] = placed ? tx * speed : 0.0;
        uy[i] = placed ? ty * speed : 0.0;
        id[i] = i;
    }
#define MNQ_CX(a, b) mnq_cmpx(d[a], id[a], ux[a], uy[a], d[b], id[b], ux[b], uy[b])
    MNQ_CX(0, 1); MNQ_CX(2, 3); MNQ_CX(4, 5); MNQ_CX(6, 7);
    MNQ_CX(0, 2); MNQ_CX(1, 3); MNQ_CX(4, 6); MNQ_CX(5, 7);
    MNQ_CX(1, 2); MNQ_CX(5, 6); MNQ_CX(0, 4); MNQ_CX(3, 7);
    MNQ_CX(1, 5); MNQ_CX(2, 6);
    MNQ_CX(1, 4); MNQ_CX(3, 6);
    MNQ_CX(2, 4); MNQ_CX(3, 5);
    MNQ_CX(3, 4);
#undef MNQ_CX
    double vx = 0.0, vy = 0.0;
#pragma unroll
    for (int q = 0; q < MN_MAX_CORES; ++q) { vx += ux[q]; vy += uy[q]; }
    vx_out = vx; vy_out = vy;
}

// ---- get_observation (marinenav_env.py:273-326, robot.py:125-198) and the flags ------------------------------------------------
// `w.obstacle(k, ox, oy, r)` hands out obstacle k of the world (generation order: it matters for the `break` quirk), `(gx, gy)` is
// its goal.  `out.head(o0, o1, o2, o3)` receives the velocity and the goal in the robot frame, `out.beam(i, bx, by)` beam i's
// reflection (0, 0 for a miss), in beam order: the caller stores them as they come, so no row is ever held in an indexed array.
// Returns the flag bits (independent of each other: they are not the done ladder of a step).
template <class World, class Out>
MNQ_HD unsigned mnq_observe(const World &w, int no, double gx, double gy, const MnDev &P, double x, double y, double theta, double velx,
                            double vely, Out &out) {
    // One pass over the obstacles for what does not depend on the beam:
    //  * check_collision (marinenav_env.py:329-336): only the obstacle with the NEAREST CENTRE is tested (first of equals);
    //  * which obstacles the sonar can reach at all.  One whose disc lies wholly beyond the range can only `continue` (no real
    //    root, or the nearer root farther than the range: robot.py:156,175,185) -- it can neither be accepted nor fire the `break`,
    //    so leaving it out of the scan changes nothing.  The 0.05 m margin covers the slope form's own error (1e-7 m at the
    //    steepest slope outside the snap window).
    unsigned reach_mask = 0;
    // (nearest by the SQUARED distance, as the KD-tree and MnLane::step find it: two d2 one ulp apart can share a rounded root)
    double bd2 = (double)INFINITY, br = 0.0;
    const double reach0 = P.sonar_range + 0.05;
    no = no < MN_MAX_OBS ? no : MN_MAX_OBS;
    for (int k = 0; k < no; ++k) {
        double ox, oy, orad;
        w.obstacle(k, ox, oy, orad);
        const double dx = ox - x, dy = oy - y, d2 = dx * dx + dy * dy, reach = reach0 + orad;
        if (d2 < bd2) { bd2 = d2; br = orad; }
        if (d2 <= reach * reach) reach_mask |= 1u << k;
    }
    unsigned flags = 0;
    if (no > 0 && sqrt(bd2) <= br + P.robot_r) flags |= MN_QUERY_FLAG_COLLISION;
    if ((x < 0.0 || x > P.width) || (y < 0.0 || y > P.height)) flags |= MN_QUERY_FLAG_OUTSIDE;
    const double gdx = x - gx, gdy = y - gy;
    if (sqrt(gdx * gdx + gdy * gdy) <= P.goal_dis) flags |= MN_QUERY_FLAG_GOAL;      // check_reach_goal (:338-342)

    const double c = cos(theta), s = sin(theta);
    // R_rw = [[c, s], [-s, c]], t_rw = -R_rw [x, y]
    const double tx = (-c) * x + (-s) * y;
    const double ty = (s) * x + (-c) * y;
    out.head(c * velx + s * vely, -s * velx + c * vely, (c * gx + s * gy) + tx, (-s * gx + c * gy) + ty);
    const double half_pi = 3.141592653589793 / 2, three_half_pi = 3 * 3.141592653589793 / 2;
    for (int bi = 0; bi < MN_NUM_BEAMS; ++bi) {
        const double angle = theta + P.beam_rel[bi];      // robot.py:134, not wrapped
        const bool vert = fabs(angle - half_pi) < 1e-03 || fabs(angle - three_half_pi) < 1e-03;
        double hx = 0.0, hy = 0.0, reflection_dist = (double)INFINITY;
        bool hit = false;
        if (reach_mask) {
            const double ca = cos(angle), sa = sin(angle);
            const double K = vert ? 0.0 : mnq_tan(angle);
            for (unsigned m = reach_mask; m;) {
                const int oi = __builtin_ctz(m);
                m &= m - 1;
                double ox, oy, orad;
                w.obstacle(oi, ox, oy, orad);
                double x1, x2, y1, y2;
                bool real;
                if (vert) {
                    const double M = orad * orad - (x - ox) * (x - ox);
                    real = !(M < 0.0);
                    x1 = x; x2 = x;
                    y1 = oy - sqrt(M); y2 = oy + sqrt(M);
                } else {
                    const double a = 1 + K * K;
                    const double b = 2 * K * (y - K * x - oy) - 2 * ox;
                    const double cc = ox * ox + (y - K * x - oy) * (y - K * x - oy) - orad * orad;
                    const double delta = b * b - 4 * a * cc;
                    real = !(delta < 0.0);
                    x1 = (-b - sqrt(delta)) / (2 * a);
                    x2 = (-b + sqrt(delta)) / (2 * a);
                    y1 = y + K * (x1 - x);
                    y2 = y + K * (x2 - x);
                }
                const double v1x = x1 - x, v1y = y1 - y, v2x = x2 - x, v2y = y2 - y;
                const double n1 = sqrt(v1x * v1x + v1y * v1y), n2 = sqrt(v2x * v2x + v2y * v2y);
                const bool first = n1 < n2;
                const double vx = first ? v1x : v2x, vy = first ? v1y : v2y, nv = first ? n1 : n2;
                if (!real || nv > P.sonar_range || vx * ca + vy * sa < 0.0) continue;      // robot.py:156,175,185,188
                if (hit && nv >= reflection_dist) break;      // robot.py:192-195: later obstacles are never examined
                reflection_dist = nv;
                hx = vx + x; hy = vy + y;
                hit = true;
            }
        }
        // marinenav_env.py:313-321: a miss is (0, 0), a hit R_rw p + t_rw
        out.beam(bi, hit ? (c * hx + s * hy) + tx : 0.0, hit ? (-s * hx + c * hy) + ty : 0.0);
    }
    return flags;
}
