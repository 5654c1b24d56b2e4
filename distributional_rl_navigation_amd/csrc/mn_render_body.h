// mn_render_body.h -- the raster rules of mn_render_worlds / mn_render_draw for ONE pixel and ONE primitive (gfx950; mn_render.hip).
//
// Written on top of mn_query_body.h: the flow colour of a pixel is mnq_velocity at its centre, the LIC streamline is mnq_velocity again at every
// Euler step.  The rules themselves are stated in include/marinenav_hip.h (and DESIGN section 29) and restated in numpy by tests/test_render_cpu.py;
// this file is their one implementation.  Every operation is an IEEE float64 add, multiply, divide, square root, floor or comparison, or integer
// arithmetic -- no trigonometric function, contraction off -- so the host build (tests/render_host.hip) and the device build give the same pixel
// words, by the argument at the head of mn_query_body.h.  Everything is __host__ __device__.  Nothing here holds an indexed private array: the
// palette is asked of the caller (`pal(level)`: LDS on the device), the obstacles of its `World` (`w.obstacle(k, ox, oy, r)`: a table read).
#pragma once
#include "mn_query_body.h"
#include "mn_render_font.h"

#define MNR_HD __host__ __device__ __forceinline__

struct MnrView {
    double x0, y0, x1, y1, sx, sy;
    int W, H;
};
MNR_HD MnrView mnr_view(const double v[4], int W, int H) { return {v[0], v[1], v[2], v[3], (v[2] - v[0]) / W, (v[3] - v[1]) / H, W, H}; }
MNR_HD bool mnr_finite(double a) { return a - a == 0.0; }

MNR_HD uint32_t mnr_noise(int c, int r, uint32_t seed) {
    uint32_t h = (uint32_t)c * 0x9E3779B1u ^ (uint32_t)r * 0x85EBCA77u ^ seed * 0xC2B2AE3Du;
    h ^= h >> 15; h *= 0x2C1B3C6Du; h ^= h >> 12; h *= 0x297A2D39u; h ^= h >> 15;
    return h >> 24;
}

// The whole word of pixel (c, r) of a world's image: field (with LIC), obstacles, markers.  `no` obstacles from `w`, start (stx, sty) and goal (gx, gy).
// The field colour and the streamline share ONE loop around ONE inlined mnq_velocity: the first evaluation, at the centre, gives the level and is the
// first Euler step of the + direction as well (the same function of the same point); the walk then goes on with +, starts again from the centre
// with -, and ends.  Lanes of a wavefront that are in different directions run the same instructions.
template <class World, class Palette>
MNR_HD uint32_t mnr_world_pixel(const MnqCores &C, const World &w, int no, double stx, double sty, double gx, double gy, const MnDev &P, const MnrView &V,
                                const mn_render_style &S, const Palette &pal, int c, int r) {
    const double x = V.x0 + (c + 0.5) * V.sx, y = V.y1 - (r + 0.5) * V.sy;
    uint32_t word;
    if (!(x >= 0.0 && x <= P.width && y >= 0.0 && y <= P.height)) {
        word = S.outside & 0xffffffu;
    } else {
        const int steps = S.lic ? S.lic_steps : 0;
        double u = c + 0.5, v = r + 0.5, s = 1.0;
        unsigned sum = mnr_noise(c, r, S.seed), count = 1;
        int k = 0;
        bool have_field = false;
        word = 0;
        for (;;) {
            double vx, vy;
            mnq_velocity(C, P, V.x0 + u * V.sx, V.y1 - v * V.sy, vx, vy);
            const double speed = sqrt(vx * vx + vy * vy);
            if (!have_field) {
                const double t = speed / S.v_max * S.n_levels;
                const int level = (!mnr_finite(t) || t >= (double)S.n_levels) ? S.n_levels - 1 : (int)floor(t);
                word = pal(level) & 0xffffffu;
                have_field = true;
            }
            bool go = k < steps && speed > 0.0 && mnr_finite(speed);
            if (go) {
                u = u + s * (S.hpx * vx / speed);
                v = v - s * (S.hpx * vy / speed);
                const double fu = floor(u), fv = floor(v);
                go = fu >= 0.0 && fu < (double)V.W && fv >= 0.0 && fv < (double)V.H;
                if (go) {
                    sum += mnr_noise((int)fu, (int)fv, S.seed);
                    count += 1;
                    go = ++k < steps;
                }
            }
            if (!go) {
                if (s < 0.0 || steps == 0) break;
                s = -1.0; u = c + 0.5; v = r + 0.5; k = 0;
            }
        }
        if (S.lic) {
            const unsigned g = (2 * sum + count) / (2 * count);
            const unsigned f = (unsigned)S.lic_floor + (255u - (unsigned)S.lic_floor) * g / 255u;
            const unsigned cr = (word >> 16 & 255u) * f / 255u, cg = (word >> 8 & 255u) * f / 255u, cb = (word & 255u) * f / 255u;
            word = cr << 16 | cg << 8 | cb;
        }
    }
    no = no < MN_MAX_OBS ? no : MN_MAX_OBS;
    for (int k = 0; k < no; ++k) {
        double ox, oy, orad;
        w.obstacle(k, ox, oy, orad);
        const double dx = x - ox, dy = y - oy;
        if (dx * dx + dy * dy <= orad * orad) { const uint32_t ow = 1u << 24 | (S.obstacle & 0xffffffu); word = ow > word ? ow : word; }
    }
    if (S.marker_r > 0.0) {
        const uint32_t mw = 2u << 24 | (S.marker & 0xffffffu);
        const double m2 = S.marker_r * S.marker_r;
        const double sdx = x - stx, sdy = y - sty, gdx = x - gx, gdy = y - gy;
        const double gd2 = gdx * gdx + gdy * gdy;
        const double rin = P.goal_dis - (V.sx > V.sy ? V.sx : V.sy);
        const bool ring = gd2 <= P.goal_dis * P.goal_dis && (rin <= 0.0 || gd2 >= rin * rin);
        if (sdx * sdx + sdy * sdy <= m2 || gd2 <= m2 || ring) word = mw > word ? mw : word;
    }
    return word;
}

// ---- primitives -----------------------------------------------------------------------------------------------------------------------------------
// A primitive is planned once (mnr_plan: its image range, its clipped geometry, how many work items it has per image) and then drawn item by item
// (mnr_item): the items of one (primitive, image) pair are independent of each other, so the caller may hand them to lanes in any order.
struct MnrPlan {
    int kind, i0, i1;        // images [i0, i1]
    long long per_image;     // items per image: samples of a segment, pixels of a box (DISC, RING, RECT, SECTOR), of a marker's square, of a glyph's cell
    double au, av, du, dv;   // SEGMENT: the clipped start and extent, pixel units.  SECTOR: (du, dv) = m, au = sqrt(m.m), av = the cosine c
    int n, hw;               // MARKER: n = shape, hw = arm.  GLYPH: hw = scale
    int c_lo, r_lo, bw;      // DISC / RING / RECT / SECTOR: the box.  MARKER: the square's top-left pixel and side.  GLYPH: the cell's top-left and width
    double cx, cy, rin2, rout2;      // RECT: the closed rectangle [cx, rin2] x [cy, rout2]
    int t;                   // MARKER: the stroke
    unsigned long long bits; // GLYPH: the 35 pixels of the character, bit 5 j + i = row j, column i
    uint32_t word;
};
#define MNR_ANCHOR_MAX 1048576.0      // 2^20: an anchor (MARKER, GLYPH) or a glyph offset farther out than this draws nothing

MNR_HD double mnr_clamp(double a, double lo, double hi) { return a < lo ? lo : (a > hi ? hi : a); }

// one edge of Liang-Barsky; false = rejected
MNR_HD bool mnr_lb_edge(double p, double q, double &t0, double &t1) {
    if (p == 0.0) return !(q < 0.0);
    const double r = q / p;
    if (p < 0.0) {
        if (r > t1) return false;
        if (r > t0) t0 = r;
    } else {
        if (r < t0) return false;
        if (r < t1) t1 = r;
    }
    return true;
}

// false: the primitive draws nothing
MNR_HD bool mnr_plan(const mn_render_prim &p, const MnrView &V, int n_images, MnrPlan &out) {
    out.kind = p.kind;
    out.i0 = p.image_first > 0 ? p.image_first : 0;
    out.i1 = p.image_last < n_images - 1 ? p.image_last : n_images - 1;
    out.word = p.color_z;
    out.per_image = 0;
    if (out.i0 > out.i1) return false;
    if (p.kind == MN_RENDER_SEGMENT) {
        const int hw = p.half_width_px < MN_RENDER_MAX_HALF_WIDTH ? p.half_width_px : MN_RENDER_MAX_HALF_WIDTH;
        const double m = hw + 1;
        const double au = (p.x0 - V.x0) / V.sx, av = (V.y1 - p.y0) / V.sy, bu = (p.x1 - V.x0) / V.sx, bv = (V.y1 - p.y1) / V.sy;
        const double du = bu - au, dv = bv - av;
        if (!(mnr_finite(au) && mnr_finite(av) && mnr_finite(bu) && mnr_finite(bv) && mnr_finite(du) && mnr_finite(dv))) return false;
        const double ulo = -m, uhi = V.W + m, vlo = -m, vhi = V.H + m;
        double t0 = 0.0, t1 = 1.0;
        if (!mnr_lb_edge(-du, au - ulo, t0, t1) || !mnr_lb_edge(du, uhi - au, t0, t1) || !mnr_lb_edge(-dv, av - vlo, t0, t1) ||
            !mnr_lb_edge(dv, vhi - av, t0, t1))
            return false;
        const double cau = mnr_clamp(au + t0 * du, ulo, uhi), cav = mnr_clamp(av + t0 * dv, vlo, vhi);
        const double cbu = mnr_clamp(au + t1 * du, ulo, uhi), cbv = mnr_clamp(av + t1 * dv, vlo, vhi);
        out.au = cau; out.av = cav; out.du = cbu - cau; out.dv = cbv - cav;
        const double eu = fabs(out.du), ev = fabs(out.dv);
        out.n = (int)ceil(eu > ev ? eu : ev);
        out.hw = hw;
        out.per_image = (long long)out.n + 1;
        return true;
    }
    if (p.kind == MN_RENDER_DISC || p.kind == MN_RENDER_RING) {
        const double rin = p.kind == MN_RENDER_RING ? p.x1 : 0.0, rout = p.kind == MN_RENDER_RING ? p.y1 : p.x1;
        if (!(mnr_finite(p.x0) && mnr_finite(p.y0) && mnr_finite(rin) && mnr_finite(rout)) || rin < 0.0 || rout < rin) return false;
        // a box that holds every pixel whose centre can pass the test (one pixel of slack each way), cut to the image IN FLOAT64, before any
        // conversion to an integer
        const double cl = floor((p.x0 - rout - V.x0) / V.sx) - 1.0, ch = floor((p.x0 + rout - V.x0) / V.sx) + 1.0;
        const double rl = floor((V.y1 - (p.y0 + rout)) / V.sy) - 1.0, rh = floor((V.y1 - (p.y0 - rout)) / V.sy) + 1.0;
        if (!(mnr_finite(cl) && mnr_finite(ch) && mnr_finite(rl) && mnr_finite(rh))) return false;
        if (ch < 0.0 || cl > V.W - 1.0 || rh < 0.0 || rl > V.H - 1.0) return false;
        const int c_lo = (int)mnr_clamp(cl, 0.0, V.W - 1.0), c_hi = (int)mnr_clamp(ch, 0.0, V.W - 1.0);
        const int r_lo = (int)mnr_clamp(rl, 0.0, V.H - 1.0), r_hi = (int)mnr_clamp(rh, 0.0, V.H - 1.0);
        out.c_lo = c_lo; out.r_lo = r_lo; out.bw = c_hi - c_lo + 1;
        out.cx = p.x0; out.cy = p.y0; out.rin2 = rin * rin; out.rout2 = rout * rout;
        out.per_image = (long long)out.bw * (r_hi - r_lo + 1);
        return true;
    }
    if (p.kind == MN_RENDER_RECT || p.kind == MN_RENDER_SECTOR) {
        if (!(mnr_finite(p.x0) && mnr_finite(p.y0) && mnr_finite(p.x1) && mnr_finite(p.y1))) return false;
        // both kinds fill the same fields below, each once, whatever the kind: a store that is in one branch only keeps the plan in memory
        const bool rect = p.kind == MN_RENDER_RECT;
        const double mx = p.x1 - p.x0, my = p.y1 - p.y0, mm = mx * mx + my * my;
        if (!rect && (p.half_width_px > 32768 || !mnr_finite(mm) || mm == 0.0)) return false;
        const double rad = rect ? 0.0 : sqrt(mm);
        const double xa = rect ? p.x0 : p.x0 - rad, xb = rect ? p.x1 : p.x0 + rad, ya = rect ? p.y0 : p.y0 - rad, yb = rect ? p.y1 : p.y0 + rad;
        const double xl = xa < xb ? xa : xb, xh = xa < xb ? xb : xa, yl = ya < yb ? ya : yb, yh = ya < yb ? yb : ya;
        out.cx = rect ? xl : p.x0; out.cy = rect ? yl : p.y0; out.rin2 = rect ? xh : 0.0; out.rout2 = rect ? yh : mm;
        out.du = mx; out.dv = my; out.au = rad; out.av = p.half_width_px / 16384.0 - 1.0;
        // the box of DISC: one pixel of slack each way, cut to the image in float64 before any conversion to an integer
        const double cl = floor((xl - V.x0) / V.sx) - 1.0, ch = floor((xh - V.x0) / V.sx) + 1.0;
        const double rl = floor((V.y1 - yh) / V.sy) - 1.0, rh = floor((V.y1 - yl) / V.sy) + 1.0;
        if (!(mnr_finite(cl) && mnr_finite(ch) && mnr_finite(rl) && mnr_finite(rh))) return false;
        if (ch < 0.0 || cl > V.W - 1.0 || rh < 0.0 || rl > V.H - 1.0) return false;
        const int c_lo = (int)mnr_clamp(cl, 0.0, V.W - 1.0), c_hi = (int)mnr_clamp(ch, 0.0, V.W - 1.0);
        const int r_lo = (int)mnr_clamp(rl, 0.0, V.H - 1.0), r_hi = (int)mnr_clamp(rh, 0.0, V.H - 1.0);
        out.c_lo = c_lo; out.r_lo = r_lo; out.bw = c_hi - c_lo + 1;
        out.per_image = (long long)out.bw * (r_hi - r_lo + 1);
        return true;
    }
    if (p.kind == MN_RENDER_MARKER || p.kind == MN_RENDER_GLYPH) {
        const double au = (p.x0 - V.x0) / V.sx, av = (V.y1 - p.y0) / V.sy;
        if (!(fabs(au) <= MNR_ANCHOR_MAX && fabs(av) <= MNR_ANCHOR_MAX)) return false;      // (a NaN fails the comparison)
        const int cu = (int)floor(au), cv = (int)floor(av);
        if (p.kind == MN_RENDER_MARKER) {
            const int h = p.half_width_px < MN_RENDER_MAX_HALF_WIDTH ? p.half_width_px : MN_RENDER_MAX_HALF_WIDTH;
            if (!(p.x1 == 0.0 || p.x1 == 1.0 || p.x1 == 2.0) || !mnr_finite(p.y1)) return false;
            out.n = (int)p.x1; out.hw = h; out.t = (int)mnr_clamp(p.y1, 0.0, (double)h);
            out.c_lo = cu - h; out.r_lo = cv - h; out.bw = 2 * h + 1;
            out.per_image = (long long)out.bw * out.bw;
            return true;
        }
        const int code = p.half_width_px & 255, scale = p.half_width_px >> 8;
        if (code <= MNR_FONT_FIRST || code >= MNR_FONT_FIRST + MNR_FONT_COUNT || scale < 1 || scale > 8) return false;
        const double ox = floor(p.x1), oy = floor(p.y1);
        if (!(fabs(ox) <= MNR_ANCHOR_MAX && fabs(oy) <= MNR_ANCHOR_MAX)) return false;
        unsigned long long bits = 0;      // the code is the same in all lanes: seven byte reads at a uniform address, no indexed private copy
        for (int j = 0; j < MNR_FONT_ROWS; ++j) {
            const unsigned row = MNR_FONT[code - MNR_FONT_FIRST][j];
            for (int i = 0; i < MNR_FONT_COLS; ++i) bits |= (unsigned long long)(row >> (MNR_FONT_COLS - 1 - i) & 1u) << (MNR_FONT_COLS * j + i);
        }
        out.bits = bits; out.hw = scale;
        out.c_lo = cu + (int)ox; out.r_lo = cv + (int)oy; out.bw = MNR_FONT_COLS * scale;
        out.per_image = (long long)out.bw * (MNR_FONT_ROWS * scale);
        return true;
    }
    return false;
}

// item j in [0, per_image) of a planned primitive: `put(c, r)` for every pixel it takes, all of them inside the image
template <class Put>
MNR_HD void mnr_item(const MnrPlan &L, const MnrView &V, long long j, Put &put) {
    if (L.kind == MN_RENDER_SEGMENT) {
        const double pu = L.n ? L.au + L.du * (double)j / L.n : L.au, pv = L.n ? L.av + L.dv * (double)j / L.n : L.av;
        const int cc = (int)floor(pu), cr = (int)floor(pv);      // inside the grown rectangle: |.| <= max(W, H) + hw + 1
        const int c0 = cc - L.hw > 0 ? cc - L.hw : 0, c1 = cc + L.hw < V.W - 1 ? cc + L.hw : V.W - 1;
        const int r0 = cr - L.hw > 0 ? cr - L.hw : 0, r1 = cr + L.hw < V.H - 1 ? cr + L.hw : V.H - 1;
        for (int r = r0; r <= r1; ++r)
            for (int c = c0; c <= c1; ++c) put(c, r);
    } else {      // a box, a square or a cell: item j is one of its pixels
        const int pc = (int)(j % L.bw), pr = (int)(j / L.bw);
        const int c = L.c_lo + pc, r = L.r_lo + pr;
        if (c < 0 || c >= V.W || r < 0 || r >= V.H) return;
        if (L.kind == MN_RENDER_MARKER) {
            const int du = pc < L.hw ? L.hw - pc : pc - L.hw, dv = pr < L.hw ? L.hw - pr : pr - L.hw;      // |du|, |dv|
            const int dd = du < dv ? dv - du : du - dv;
            if (L.n == 0 || (L.n == 1 && (du <= L.t || dv <= L.t)) || (L.n == 2 && dd <= L.t)) put(c, r);
        } else if (L.kind == MN_RENDER_GLYPH) {
            if (L.bits >> (MNR_FONT_COLS * (pr / L.hw) + pc / L.hw) & 1ull) put(c, r);
        } else {
            const double x = V.x0 + (c + 0.5) * V.sx, y = V.y1 - (r + 0.5) * V.sy;
            if (L.kind == MN_RENDER_RECT) {
                if (x >= L.cx && x <= L.rin2 && y >= L.cy && y <= L.rout2) put(c, r);
            } else {
                const double dx = x - L.cx, dy = y - L.cy;
                const double d2 = dx * dx + dy * dy;
                if (L.kind == MN_RENDER_SECTOR) {
                    if (d2 <= L.rout2 && (d2 == 0.0 || dx * L.du + dy * L.dv >= L.av * sqrt(d2) * L.au)) put(c, r);
                } else if (d2 <= L.rout2 && d2 >= L.rin2) put(c, r);
            }
        }
    }
}
