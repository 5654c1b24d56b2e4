// mn_time_field_body.h -- the minimum-time-to-goal field of ONE world on a grid (Zermelo navigation on a 16-direction stencil): the rules of
// mn_time_field as include/marinenav_hip.h writes them out, on top of the query body's get_velocity (gfx950: mn_time_field.hip; CPU:
// tests/time_field_host.hip).
//
// Every operation is an IEEE float64 add, multiply, divide, square root or comparison (contraction off, as the whole library), so the host build, the
// device and a restatement from the header agree bit for bit.  Everything here is __host__ __device__ and holds no indexed array: the stencil's
// offsets are nibbles of two 64-bit constants, the loops over k are fully unrolled.
//
// The pieces, in the order a solve uses them:
//   mntf_cell        current, free flag and source flag of one cell (phase a)
//   mntf_cell_edges  the 16 edge times of one cell, +inf for an edge that does not exist or is infeasible (phase b)
//   mntf_relax       T(u) <- min(T(u), min_k w_k(u) + T(u + off_k)) for one cell, reading whatever values its neighbours hold (phase c)
//   mntf_dir         the least k that attains min_k w_k(u) + T(u + off_k), or 255 (phase d)
// The caller supplies the storage: a `Grid` with free(c), current(c, cx, cy), w(k, c) and T(c) over cells c = j * nx + i.
#pragma once
#include "mn_query_body.h"

#define MNTF_MAX_CELLS 16384
#define MNTF_DIRS 16
#define MNTF_NO_DIR 255

// offset k as nibbles (value + 2), k = 0 in the lowest: the four axis moves, the four diagonals, the eight knight moves, counter-clockwise from +x
//   k   0  1  2  3 |  4  5  6  7 |  8  9 10 11 12 13 14 15
//   dx  1  0 -1  0 |  1 -1 -1  1 |  2  1 -1 -2 -2 -1  1  2
//   dy  0  1  0 -1 |  1  1 -1 -1 |  1  2  2  1 -1 -2 -2 -1
#define MNTF_DX_NIBBLES 0x4310013431132123ull
#define MNTF_DY_NIBBLES 0x1001344311331232ull
MNQ_HD int mntf_dx(int k) { return (int)((MNTF_DX_NIBBLES >> (4 * k)) & 15) - 2; }
MNQ_HD int mntf_dy(int k) { return (int)((MNTF_DY_NIBBLES >> (4 * k)) & 15) - 2; }

// the two cells the segment of offset (dx, dy) crosses, relative to its start: a diagonal (dx, dy) crosses (dx, 0) and (0, dy), a knight move
// (2 sx, sy) crosses (sx, 0) and (sx, sy), a knight move (sx, 2 sy) crosses (0, sy) and (sx, sy); an axis move crosses nothing (both are its end)
MNQ_HD void mntf_crossed(int dx, int dy, int &ax, int &ay, int &bx, int &by) {
    const int sx = dx > 0 ? 1 : (dx < 0 ? -1 : 0), sy = dy > 0 ? 1 : (dy < 0 ? -1 : 0);
    if (dx == 2 || dx == -2) { ax = sx; ay = 0; bx = sx; by = sy; }
    else if (dy == 2 || dy == -2) { ax = 0; ay = sy; bx = sx; by = sy; }
    else if (dx != 0 && dy != 0) { ax = dx; ay = 0; bx = 0; by = dy; }
    else { ax = dx; ay = dy; bx = dx; by = dy; }
}

// Phase (a): the centre of cell (i, j), its current, whether it is free (EVERY placed obstacle farther than r + robot_r + clearance: with a NaN
// anywhere the comparison fails and the cell is blocked) and whether it is a source (free, and within goal_dis of the goal: check_reach_goal)
template <class World>
MNQ_HD void mntf_cell(const MnqCores &C, const World &w, int no, double gx, double gy, const MnDev &P, double hx, double hy, double clearance, int i,
                      int j, double &cx, double &cy, bool &is_free, bool &is_source) {
    const double x = ((double)i + 0.5) * hx, y = ((double)j + 0.5) * hy;
    mnq_velocity(C, P, x, y, cx, cy);
    bool fr = true;
    no = no < MN_MAX_OBS ? no : MN_MAX_OBS;
    for (int k = 0; k < no; ++k) {
        double ox, oy, orad;
        w.obstacle(k, ox, oy, orad);
        const double dx = ox - x, dy = oy - y;
        if (!(sqrt(dx * dx + dy * dy) > (orad + P.robot_r) + clearance)) fr = false;
    }
    const double gdx = x - gx, gdy = y - gy;
    is_free = fr;
    is_source = fr && sqrt(gdx * gdx + gdy * gdy) <= P.goal_dis;
}

// the time of one edge of offset (dx, dy) cells between cells whose currents are (cux, cuy) and (cvx, cvy), at vehicle speed s; +inf if infeasible
MNQ_HD double mntf_edge_time(int dx, int dy, double hx, double hy, double cux, double cuy, double cvx, double cvy, double s) {
    const double ex = (double)dx * hx, ey = (double)dy * hy;
    const double L = sqrt(ex * ex + ey * ey);
    const double ux = ex / L, uy = ey / L;
    const double cx = (cux + cvx) * 0.5, cy = (cuy + cvy) * 0.5;
    const double a = cx * ux + cy * uy;
    const double disc = (s * s - (cx * cx + cy * cy)) + a * a;
    const double g = a + sqrt(disc);
    return (disc >= 0.0 && g > 0.0) ? L / g : (double)INFINITY;      // (a NaN fails both)
}

// Phase (b): the 16 edge times of cell (i, j) go to put(k, w).  The edge exists iff the cell itself, its end and the two crossed cells are inside
// the grid and free.
template <class Grid, class Put>
MNQ_HD void mntf_cell_edges(const Grid &g, int nx, int ny, double hx, double hy, double s, int i, int j, Put &put) {
    const int c = j * nx + i;
    const bool own = g.free(c);
    double cux = 0.0, cuy = 0.0;
    if (own) g.current(c, cux, cuy);
#pragma unroll
    for (int k = 0; k < MNTF_DIRS; ++k) {
        const int dx = mntf_dx(k), dy = mntf_dy(k);
        int ax, ay, bx, by;
        mntf_crossed(dx, dy, ax, ay, bx, by);
        double w = (double)INFINITY;
        const int vi = i + dx, vj = j + dy;
        if (own && vi >= 0 && vi < nx && vj >= 0 && vj < ny) {      // (the crossed cells lie in the box the two ends span: inside as well)
            const int v = c + dy * nx + dx;
            if (g.free(v) && g.free(c + ay * nx + ax) && g.free(c + by * nx + bx)) {
                double cvx, cvy;
                g.current(v, cvx, cvy);
                w = mntf_edge_time(dx, dy, hx, hy, cux, cuy, cvx, cvy, s);
            }
        }
        put(k, w);
    }
}

// Phase (c), PULL form: the new value of cell c from whatever its neighbours hold now.  The neighbour of an edge time of +inf is not read (it may lie
// outside the grid), so every T(c + off) read is inside.  Returns true if the value fell.
template <class Grid>
MNQ_HD bool mntf_relax(const Grid &g, int nx, int c, double &t_out) {
    // straight-line on purpose: the 16 edge times are read first, back to back (constant indices: registers, not an indexed array), and an edge of
    // +inf reads the cell's own T instead of its neighbour's -- +inf + T is +inf and never wins --, so no load waits behind a branch
    double w[MNTF_DIRS];
#pragma unroll
    for (int k = 0; k < MNTF_DIRS; ++k) w[k] = g.w(k, c);
    const double t0 = g.T(c);
    double best = t0;
#pragma unroll
    for (int k = 0; k < MNTF_DIRS; ++k) {
        const double cand = w[k] + g.T(w[k] < (double)INFINITY ? c + mntf_dy(k) * nx + mntf_dx(k) : c);
        if (cand < best) best = cand;
    }
    t_out = best;
    return best < t0;
}

// Phase (d): the least k that attains min_k (w_k + T(c + off_k)); 255 where that minimum is +inf, for a blocked cell and for a source (the cells
// with T = 0: every other finite T is an edge time above zero plus a T).
template <class Grid>
MNQ_HD int mntf_dir(const Grid &g, int nx, int c) {
    if (!g.free(c) || g.T(c) == 0.0) return MNTF_NO_DIR;
    double best = (double)INFINITY;
    int dir = MNTF_NO_DIR;
#pragma unroll
    for (int k = 0; k < MNTF_DIRS; ++k) {
        const double w = g.w(k, c);
        if (w < (double)INFINITY) {
            const double cand = w + g.T(c + mntf_dy(k) * nx + mntf_dx(k));
            if (cand < best) { best = cand; dir = k; }
        }
    }
    return dir;
}
