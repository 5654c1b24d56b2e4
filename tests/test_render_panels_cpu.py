"""The plot primitives of mn_render_draw (RECT, MARKER, GLYPH, SECTOR), the text / number builders and the side panels of render_panels.py, as far
as they go without a GPU.  The raster body is __host__ __device__, so tests/render_host.hip (built here as tests/test_render_cpu.py builds it) runs
the new kinds on the CPU; they are compared with an independent numpy restatement of the rules in include/marinenav_hip.h, written here from the
rules.  Bound: EQUAL pixel words, every pixel.  MARKER and GLYPH are integer rules behind one floor: nothing is left out.  For RECT and SECTOR the
twin marks threshold-fragile pixels (a pixel centre within 1e-9 of a rectangle edge; |d.d - m.m| < 1e-9 or the angle test within 1e-9 of equality),
at most 4 per image, which the comparison may leave out; their number is printed.  The font is read through mn_render_font and not repeated here."""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import test_render_cpu as H      # noqa: E402

W, HGT, VIEW, IMAGES, FILL = H.PRIM_W, H.PRIM_H, H.PRIM_VIEW, H.PRIM_IMAGES, H.FILL
RECT, MARKER, GLYPH, SECTOR = 4, 5, 6, 7
ANCHOR_MAX = float(1 << 20)


@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    if not os.path.exists(H.HIPCC):
        pytest.skip("no hipcc")
    return H.build_host(tmp_path_factory.mktemp("render_host_panels"))


@pytest.fixture(scope="module")
def font():
    from distributional_rl_navigation_amd import render
    return render.font()


# ---- the twin ---------------------------------------------------------------------------------------------------------------------------------------
def twin_draw(pixels, view, prims, font):
    """`prims` (render.PRIM_DTYPE) into `pixels` [I][H][W] uint32 by the rules; the three old kinds by tests/test_render_cpu.py's twin.  Returns
    fragile [I][H][W] bool: the pixels of RECT and SECTOR records whose test is within 1e-9 of its threshold."""
    I, Hh, Ww = pixels.shape
    x0, y0, x1, y1 = (float(a) for a in view)
    sx, sy = (x1 - x0) / Ww, (y1 - y0) / Hh
    c, r = np.meshgrid(np.arange(Ww), np.arange(Hh), indexing="xy")
    X, Y = x0 + (c + 0.5) * sx, y1 - (r + 0.5) * sy
    fragile = np.zeros(pixels.shape, bool)
    fin = math.isfinite

    def put_mask(i0, i1, hit, word):
        pixels[i0:i1 + 1][:, hit] = np.maximum(pixels[i0:i1 + 1][:, hit], np.uint32(word))

    def anchor(px, py):
        with np.errstate(all="ignore"):
            au, av = float(np.float64(px - x0) / np.float64(sx)), float(np.float64(y1 - py) / np.float64(sy))
        if not (abs(au) <= ANCHOR_MAX and abs(av) <= ANCHOR_MAX):
            return None
        return math.floor(au), math.floor(av)

    for p in prims:
        kind = int(p["kind"])
        if kind < 3:
            H.twin_draw(pixels, view, np.array([p], dtype=prims.dtype))
            continue
        i0, i1 = max(int(p["image_first"]), 0), min(int(p["image_last"]), I - 1)
        if i0 > i1:
            continue
        word, hw = int(p["color_z"]), int(p["half_width_px"])
        ax, ay, bx, by = float(p["x0"]), float(p["y0"]), float(p["x1"]), float(p["y1"])
        if kind == RECT:
            if not all(fin(q) for q in (ax, ay, bx, by)):
                continue
            xl, xh, yl, yh = min(ax, bx), max(ax, bx), min(ay, by), max(ay, by)
            hit = (X >= xl) & (X <= xh) & (Y >= yl) & (Y <= yh)
            near = ((np.abs(X - xl) < 1e-9) | (np.abs(X - xh) < 1e-9)) & (Y >= yl - 1e-9) & (Y <= yh + 1e-9)
            near |= ((np.abs(Y - yl) < 1e-9) | (np.abs(Y - yh) < 1e-9)) & (X >= xl - 1e-9) & (X <= xh + 1e-9)
            fragile[i0:i1 + 1] |= near
            put_mask(i0, i1, hit, word)
        elif kind == MARKER:
            a = anchor(ax, ay)
            if a is None or bx not in (0.0, 1.0, 2.0) or not fin(by):
                continue
            h = min(hw, 8)
            t = min(max(int(by), 0), h)
            for dv in range(-h, h + 1):
                for du in range(-h, h + 1):
                    take = bx == 0.0 or (bx == 1.0 and (abs(du) <= t or abs(dv) <= t)) or (bx == 2.0 and abs(abs(du) - abs(dv)) <= t)
                    cc, rr = a[0] + du, a[1] + dv
                    if take and 0 <= cc < Ww and 0 <= rr < Hh:
                        pixels[i0:i1 + 1, rr, cc] = np.maximum(pixels[i0:i1 + 1, rr, cc], np.uint32(word))
        elif kind == GLYPH:
            a = anchor(ax, ay)
            code, scale = hw & 255, hw >> 8
            if a is None or not 33 <= code <= 126 or not 1 <= scale <= 8 or not (fin(bx) and fin(by)):
                continue
            ox, oy = math.floor(bx), math.floor(by)
            if abs(ox) > ANCHOR_MAX or abs(oy) > ANCHOR_MAX:
                continue
            L, T = a[0] + ox, a[1] + oy
            for j in range(7):
                for i in range(5):
                    if int(font[code - 32][j]) >> (4 - i) & 1:
                        c0, c1, r0, r1 = max(L + i * scale, 0), min(L + (i + 1) * scale, Ww), max(T + j * scale, 0), min(T + (j + 1) * scale, Hh)
                        if c0 < c1 and r0 < r1:
                            pixels[i0:i1 + 1, r0:r1, c0:c1] = np.maximum(pixels[i0:i1 + 1, r0:r1, c0:c1], np.uint32(word))
        elif kind == SECTOR:
            if hw > 32768 or not all(fin(q) for q in (ax, ay, bx, by)):
                continue
            with np.errstate(all="ignore"):
                mx, my = np.float64(bx) - np.float64(ax), np.float64(by) - np.float64(ay)
                mm = mx * mx + my * my
                if not np.isfinite(mm) or mm == 0.0:
                    continue
                cos = np.float64(hw) / 16384.0 - 1.0
                dx, dy = X - ax, Y - ay
                dd = dx * dx + dy * dy
                dm, rhs = dx * mx + dy * my, cos * np.sqrt(dd) * np.sqrt(mm)
                hit = (dd <= mm) & ((dd == 0.0) | (dm >= rhs))
                fragile[i0:i1 + 1] |= (np.abs(dd - mm) < 1e-9) | ((dd <= mm + 1e-9) & (np.abs(dm - rhs) < 1e-9))
            put_mask(i0, i1, hit, word)
    return fragile


# ---- the cases, shared with tests/test_render_panels_gpu.py ----------------------------------------------------------------------------------------
def panel_cases():
    """name -> record array (render.PRIM_DTYPE) over the 80 x 48 canvas of 3 images, half a world unit per pixel."""
    from distributional_rl_navigation_amd import render
    nan, inf = float("nan"), float("inf")

    def rec(rows):
        a = np.zeros(len(rows), dtype=render.PRIM_DTYPE)
        for i, row in enumerate(rows):
            a[i] = row
        return a
    red, green, blue, grey = render.word(0xFF0000, 4), render.word(0x00FF00, 4), render.word(0x0000FF, 5), render.word(0x999999, 3)
    px = lambda c, r: (0.25 + 0.5 * c, 23.75 - 0.5 * r)      # the centre of pixel (column c, row r)
    cases = {}
    cases["rect_corner_orders"] = rec([(3.1, 4.2, 12.7, 9.9, 0, 0, red, RECT, 0), (12.7, 14.2, 3.1, 19.9, 0, 0, green, RECT, 0), (23.1, 9.9, 32.7, 4.2, 1, 1, red, RECT, 0),
                                       (32.7, 19.9, 23.1, 14.2, 1, 2, blue, RECT, 7)])
    cases["rect_degenerate"] = rec([px(20, 20) + px(20, 20) + (0, 0, red, RECT, 0), (10.3, 10.3, 10.3, 10.3, 0, 0, green, RECT, 0),
                                    (5.2, 2.1, 5.3, 9.1, 1, 1, blue, RECT, 0), (7.1, 3.3, 30.2, 3.3, 2, 2, red, RECT, 0), (7.1, 3.2, 30.2, 3.3, 2, 2, green, RECT, 0)])
    cases["rect_edges"] = rec([(-3.0, 5.1, 2.1, 8.2, 0, 0, red, RECT, 0), (38.1, 5.1, 45.0, 8.2, 0, 0, green, RECT, 0), (10.1, -4.0, 14.2, 1.1, 1, 1, blue, RECT, 0),
                               (10.1, 22.1, 14.2, 30.0, 1, 1, red, RECT, 0), (-9.0, -9.0, -1.0, -1.0, 2, 2, red, RECT, 0), (41.0, 3.0, 50.0, 9.0, 2, 2, red, RECT, 0)])
    cases["rect_huge"] = rec([(-1e300, -1e300, 1e300, 1e300, 0, 0, red, RECT, 0), (1e300, 3.1, 20.1, 5.2, 1, 1, green, RECT, 0), (8.1, -1e300, 9.2, 1e300, 2, 2, blue, RECT, 0),
                              (1e300, 1e300, 2e300, 2e300, 0, 2, blue, RECT, 0)])
    cases["rect_nan"] = rec([(nan, 2.0, 30.0, 20.0, 0, 2, red, RECT, 0), (2.0, nan, 30.0, 20.0, 0, 2, red, RECT, 0), (2.0, 2.0, nan, 20.0, 0, 2, red, RECT, 0),
                             (2.0, 2.0, 30.0, nan, 0, 2, red, RECT, 0), (2.0, 2.0, inf, 20.0, 0, 2, red, RECT, 0), (-inf, 2.0, 30.0, 20.0, 0, 2, red, RECT, 0)])
    rows = []
    for s, shape in enumerate((0.0, 1.0, 2.0)):
        for k, h in enumerate((0, 1, 3, 8, 9)):
            for img, t in enumerate((0.0, 1.0, 20.0)):
                rows.append((4.1 + 8.0 * k, 4.1 + 8.0 * s, shape, t, img, img, (red, green, blue)[s], MARKER, h))
    cases["marker_shapes"] = rec(rows)
    rows = []
    for img, (shape, t) in enumerate(((2.0, 1.0), (1.0, 0.0), (0.0, 0.0))):
        for c, r in ((0, 0), (79, 0), (0, 47), (79, 47), (-1, -1), (80, -1), (-1, 48), (80, 48), (40, -4), (-9, 20)):
            rows.append(px(c, r) + (shape, t, img, img, red, MARKER, 3))
    cases["marker_corners"] = rec(rows)
    cases["marker_bad"] = rec([(20.0, 12.0, 3.0, 1.0, 0, 2, red, MARKER, 3), (20.0, 12.0, 0.5, 1.0, 0, 2, red, MARKER, 3), (20.0, 12.0, nan, 1.0, 0, 2, red, MARKER, 3),
                               (20.0, 12.0, -1.0, 1.0, 0, 2, red, MARKER, 3), (1e300, 12.0, 0.0, 1.0, 0, 2, red, MARKER, 3), (20.0, -1e300, 0.0, 1.0, 0, 2, red, MARKER, 3),
                               (nan, 12.0, 0.0, 1.0, 0, 2, red, MARKER, 3), (20.0, inf, 0.0, 1.0, 0, 2, red, MARKER, 3), (20.0, 12.0, 1.0, nan, 0, 2, red, MARKER, 3),
                               (20.0, 12.0, 1.0, inf, 0, 2, red, MARKER, 3), (0.5 * ANCHOR_MAX + 1.0, 12.0, 0.0, 0.0, 0, 2, red, MARKER, 8)])
    cases["marker_stroke_edge"] = rec([(10.0, 12.0, 1.0, -3.0, 0, 0, red, MARKER, 4), (20.0, 12.0, 2.0, 1.9, 0, 0, green, MARKER, 4), (30.0, 12.0, 1.0, 1e300, 0, 0, blue, MARKER, 4),
                                       (10.0, 12.0, 2.0, -1e300, 1, 1, red, MARKER, 65535), (0.5 * ANCHOR_MAX, 12.0, 0.0, 0.0, 1, 1, red, MARKER, 8)])
    cases["glyph_all_codes"] = rec([(1.0 + 3.0 * (k % 13), 23.0 - 4.0 * ((k % 32) // 13), 0.0, 0.0, k // 32, k // 32, red, GLYPH, (32 + k) | 1 << 8) for k in range(95)])
    rows = []
    for img, scale, x in ((0, 1, 2.0), (0, 2, 14.0), (1, 3, 2.0), (2, 8, 1.0)):
        for i, ch in enumerate("Ab9"):
            rows.append((x, 22.0, 6.0 * scale * i, 0.0, img, img, (red, green, blue)[i], GLYPH, ord(ch) | scale << 8))
    cases["glyph_scales"] = rec(rows)
    cases["glyph_edges"] = rec([px(0, 0) + (-4.0, -5.0, 0, 0, red, GLYPH, ord("#") | 2 << 8), px(79, 0) + (-3.0, -9.0, 0, 0, green, GLYPH, ord("#") | 2 << 8),
                                px(0, 47) + (-7.5, -6.2, 0, 0, blue, GLYPH, ord("#") | 2 << 8), px(79, 47) + (-2.0, -3.0, 0, 0, red, GLYPH, ord("#") | 2 << 8),
                                px(40, 0) + (0.0, -14.0, 1, 1, red, GLYPH, ord("#") | 2 << 8), px(40, 47) + (0.0, 1.0, 1, 1, red, GLYPH, ord("#") | 2 << 8),
                                px(0, 20) + (-10.0, 0.0, 1, 1, red, GLYPH, ord("#") | 2 << 8), px(79, 20) + (1.0, 0.0, 1, 1, red, GLYPH, ord("#") | 2 << 8),
                                px(-30, -30) + (29.0, 28.0, 2, 2, green, GLYPH, ord("W") | 3 << 8), px(100, 60) + (-30.0, -20.0, 2, 2, blue, GLYPH, ord("M") | 1 << 8)])
    cases["glyph_bad"] = rec([(20.0, 12.0, 0.0, 0.0, 0, 2, red, GLYPH, 31 | 1 << 8), (20.0, 12.0, 0.0, 0.0, 0, 2, red, GLYPH, 127 | 1 << 8), (20.0, 12.0, 0.0, 0.0, 0, 2, red, GLYPH, 32 | 1 << 8),
                              (20.0, 12.0, 0.0, 0.0, 0, 2, red, GLYPH, 255 | 1 << 8), (20.0, 12.0, 0.0, 0.0, 0, 2, red, GLYPH, 65), (20.0, 12.0, 0.0, 0.0, 0, 2, red, GLYPH, 65 | 9 << 8),
                              (20.0, 12.0, float(1 << 21), 0.0, 0, 2, red, GLYPH, 65 | 1 << 8), (20.0, 12.0, 0.0, -float(1 << 21), 0, 2, red, GLYPH, 65 | 1 << 8),
                              (20.0, 12.0, nan, 0.0, 0, 2, red, GLYPH, 65 | 1 << 8), (20.0, 12.0, 0.0, inf, 0, 2, red, GLYPH, 65 | 1 << 8), (nan, 12.0, 0.0, 0.0, 0, 2, red, GLYPH, 65 | 1 << 8),
                              (1e300, 12.0, 0.0, 0.0, 0, 2, red, GLYPH, 65 | 1 << 8), (20.0, 12.0, 1e300, 0.0, 0, 2, red, GLYPH, 65 | 1 << 8)])
    sonar = render.sector_cosine(0.9 * math.pi / 2)
    cases["sector_angles"] = rec([(20.1, 2.2, 20.1, 19.3, 0, 0, red, SECTOR, sonar), (20.1, 12.2, 26.3, 18.1, 1, 1, green, SECTOR, 16384), (5.1, 4.3, 33.3, 16.4, 2, 2, blue, SECTOR, 32760),
                                  (30.1, 12.2, 33.2, 8.3, 2, 2, red, SECTOR, 0), (6.1, 18.2, 9.3, 17.1, 1, 1, blue, SECTOR, 1)])
    cases["sector_outside_and_centre"] = rec([(-5.1, 12.2, 9.3, 13.1, 0, 0, red, SECTOR, sonar), (45.1, 30.2, 30.3, 14.1, 0, 0, green, SECTOR, 20000), px(30, 30) + (22.1, 12.3, 1, 1, blue, SECTOR, 30000),
                                              (100.0, 100.0, 101.0, 100.0, 0, 2, red, SECTOR, 0), (20.1, 12.2, 20.1 + 1e-3, 12.2, 2, 2, red, SECTOR, 0)])
    cases["sector_bad"] = rec([(20.0, 12.0, 20.0, 12.0, 0, 2, red, SECTOR, sonar), (20.0, 12.0, 1e300, 12.0, 0, 2, red, SECTOR, sonar), (20.0, 12.0, 25.0, 12.0, 0, 2, red, SECTOR, 32769),
                               (20.0, 12.0, 25.0, 12.0, 0, 2, red, SECTOR, 65535), (nan, 12.0, 25.0, 12.0, 0, 2, red, SECTOR, sonar), (20.0, 12.0, 25.0, inf, 0, 2, red, SECTOR, sonar),
                               (1e300, 1e300, 1e300, 1e300, 0, 2, red, SECTOR, sonar), (20.0, 12.0, 20.0, -1e200, 0, 2, red, SECTOR, sonar)])
    rows = []
    for y, (kind, a, b, hw) in enumerate(((RECT, 12.1, 14.2, 0), (MARKER, 2.0, 1.0, 3), (GLYPH, 0.0, 0.0, ord("R") | 2 << 8), (SECTOR, 16.1, 20.3, 20000))):
        cx, cy = (10.1, 4.1 + 5.0 * y)
        bx, by = (cx + 4.0, cy + 2.0) if kind == RECT else ((cx + 3.0, cy + 1.0) if kind == SECTOR else (a, b))
        for dx, (first, last) in enumerate(((2, 1), (-5, 99), (3, 7), (-9, -1), (1, 1))):
            ox = 0.0 if dx != 4 else 15.0
            rows.append((cx + ox, cy, bx + (ox if kind in (RECT, SECTOR) else 0.0), by, first, last, (red, green, blue, grey, red)[dx], kind, hw))
    cases["image_ranges_new_kinds"] = rec(rows)
    cases["equal_z"] = rec([(5.1, 5.1, 20.2, 15.2, 0, 0, render.word(0xFF0000, 4), RECT, 0), (12.1, 8.1, 30.2, 20.2, 0, 0, render.word(0x00FF00, 4), RECT, 0),
                            (10.1, 12.1, 2.0, 1.0, 0, 0, render.word(0x0000FF, 4), MARKER, 8), (20.1, 12.1, 0.0, 0.0, 0, 0, render.word(0xFFFF00, 4), GLYPH, ord("Z") | 4 << 8),
                            (20.1, 3.2, 20.1, 21.3, 1, 1, render.word(0xFFCCCC, 2), SECTOR, sonar), (10.1, 8.1, 30.2, 14.2, 1, 1, render.word(0x00FF00, 3), RECT, 0),
                            (14.1, 14.1, 0.0, 0.0, 1, 1, render.word(0x000000, 4), GLYPH, ord("g") | 3 << 8)])
    return cases


CASE_NAMES = ("rect_corner_orders", "rect_degenerate", "rect_edges", "rect_huge", "rect_nan", "marker_shapes", "marker_corners", "marker_bad", "marker_stroke_edge",
              "glyph_all_codes", "glyph_scales", "glyph_edges", "glyph_bad", "sector_angles", "sector_outside_and_centre", "sector_bad", "image_ranges_new_kinds",
              "equal_z")
DRAW_NOTHING = ("rect_nan", "marker_bad", "glyph_bad", "sector_bad")


@pytest.mark.parametrize("name", CASE_NAMES)
def test_new_kinds_equal_the_twin(host_program, tmp_path, font, name):
    prims = panel_cases()[name]
    got, items, most = H.run_host(host_program, tmp_path, name, W, HGT, VIEW, n_images=IMAGES, prims=prims, fill=FILL)
    want = np.full((IMAGES, HGT, W), FILL, dtype=np.uint32)
    fragile = twin_draw(want, VIEW, prims, font)
    diff = got != want
    per_image = fragile.reshape(IMAGES, -1).sum(axis=1)
    print(f"[{name}] {int((got != FILL).sum())} pixels drawn, {items} work items, at most {most} per primitive and image; {int(diff.sum())} differ from the twin, "
          f"threshold-fragile per image {per_image.tolist()}")
    assert (per_image <= 4).all(), per_image
    if name.startswith(("rect", "sector")):
        assert not (diff & ~fragile).any(), np.argwhere(diff & ~fragile)[:5]
    else:
        assert not diff.any(), np.argwhere(diff)[:5]
    assert most <= W * HGT      # a box is cut to the image whatever the record holds; a marker has at most 17 x 17 items, a glyph 40 x 56
    drawn = got != FILL
    if name in DRAW_NOTHING:
        assert not drawn.any()
    else:
        assert drawn.any()
    if name == "rect_degenerate":
        assert drawn[0].sum() == 1 and drawn[0][20, 20]      # on a pixel centre: that pixel; off one: nothing
        assert drawn[1].sum() == 14 and drawn[1][:, 10].sum() == 14      # a sliver around x = 5.25, column 10; y in [2.1, 9.1]: 14 centres
        assert drawn[2].sum() == 46 and (got[2][drawn[2]] == prims["color_z"][4]).all()      # the line y = 3.3 meets no centre; the sliver around y = 3.25 is row 41
    if name == "rect_huge":
        assert drawn[0].all() and drawn[1][38:42, 40:].all() and drawn[1].sum() == 4 * 40 and drawn[2][:, 16:18].all() and drawn[2].sum() == 2 * HGT
    if name == "marker_shapes":      # the squares of image 0 are (2 h + 1)^2 pixels where nothing covers them: h = 0 at column 8, row 39
        assert drawn[0][39, 8] and not drawn[0][38:41, 7:10].sum() > 1
    if name == "marker_corners":
        assert drawn[0][0, 0] and drawn[0][0, 79] and drawn[0][47, 0] and drawn[0][47, 79] and not drawn[0][10:30, 10:70].any()
        assert drawn[2][:4, :4].all() and drawn[2][:3, 77:].all() and drawn[2][45:, :3].all()      # squares of arm 3 around the corners and the pixels outside them
    if name == "image_ranges_new_kinds":      # per kind: [2, 1] red, empty; [-5, 99] green, every image; [3, 7] blue and [-9, -1] grey miss; [1, 1] red
        red, green, blue, grey = (int(prims["color_z"][k]) for k in range(4))
        assert [bool((got[i] == green).any()) for i in range(IMAGES)] == [True] * 3 and [bool((got[i] == red).any()) for i in range(IMAGES)] == [False, True, False]
        assert not (got == blue).any() and not (got == grey).any()
        rows_of = lambda word, i: set(np.argwhere(got[i] == word)[:, 0] // 10)      # the four kinds sit 10 rows apart
        assert len(rows_of(green, 0)) == 4 and len(rows_of(red, 1)) == 4
    if name == "equal_z":
        solo = []      # image 0: two rects, a marker and a glyph, all at z = 4 in four colours: every pixel keeps the largest word that reached it
        for k in range(4):
            a = np.full((IMAGES, HGT, W), FILL, dtype=np.uint32)
            twin_draw(a, VIEW, prims[k:k + 1], font)
            solo.append(a[0])
        assert np.array_equal(got[0], np.maximum.reduce(solo))
        both = (solo[0] != FILL) & (solo[1] != FILL)
        assert both.any() and (got[0][both] >= prims["color_z"][0]).all() and (got[0][both] == prims["color_z"][0]).any()      # red over green where only they meet
        z = got[1] >> 24
        assert (z == 2).any() and (z == 3).any() and (z == 4).any()      # the glyph over the rect over the sector: all three show


def test_new_kinds_in_any_order_on_the_host(host_program, tmp_path):
    cases = panel_cases()
    prims = np.concatenate([cases[k] for k in ("rect_corner_orders", "marker_shapes", "glyph_scales", "sector_angles", "equal_z")] + [H.prim_cases()["diagonal"]])
    a, _, _ = H.run_host(host_program, tmp_path, "fwd", W, HGT, VIEW, n_images=IMAGES, prims=prims, fill=FILL)
    b, _, _ = H.run_host(host_program, tmp_path, "rev", W, HGT, VIEW, n_images=IMAGES, prims=prims[::-1].copy(), fill=FILL)
    assert np.array_equal(a, b)


# ---- the font ---------------------------------------------------------------------------------------------------------------------------------------
def test_font_table(font):
    assert font.shape == (95, 7) and font.dtype == np.uint8 and (font < 32).all()
    empty = [k for k in range(95) if not font[k].any()]
    assert empty == [0]      # only the space
    assert len({bytes(row) for row in font}) == 95
    bits = lambda k: np.unpackbits(font[k][:, None], axis=1)[:, 3:]
    carriers = [ord(ch) - 32 for ch in "0123456789-."]
    for i, a in enumerate(carriers):
        for b in carriers[i + 1:]:
            d = int((bits(a) != bits(b)).sum())
            assert d >= 3, (chr(a + 32), chr(b + 32), d)
    for k in range(1, 95):      # every character reaches both sides or is a narrow one on purpose; none is a single pixel
        assert bits(k).sum() >= 3, chr(k + 32)


def test_symbols():
    import ctypes as C
    from distributional_rl_navigation_amd import _capi
    text = H._header()
    assert H._args(text, "mn_render_font") == ["uint8_t *out"]
    sig = {n: (r, a) for n, r, a in _capi.SIGNATURES}
    assert sig["mn_render_font"] == (C.c_int, [C.c_void_p])
    for name, value in (("MN_RENDER_RECT", _capi.RENDER_RECT), ("MN_RENDER_MARKER", _capi.RENDER_MARKER), ("MN_RENDER_GLYPH", _capi.RENDER_GLYPH),
                        ("MN_RENDER_SECTOR", _capi.RENDER_SECTOR)):
        import re
        m = re.search(name + r" = (\d+)", text)
        assert m and int(m.group(1)) == value, name
    assert (RECT, MARKER, GLYPH, SECTOR) == (_capi.RENDER_RECT, _capi.RENDER_MARKER, _capi.RENDER_GLYPH, _capi.RENDER_SECTOR)
    assert _capi.lib().mn_render_font(None) == -1


def test_kernels_keep_their_resources():
    """The two kernels of mn_render.hip with the four kinds in: no scratch, no spill, at most 256 registers (the figures are printed)."""
    H.test_render_kernels_resources()


# ---- numbers, text, choose_text ---------------------------------------------------------------------------------------------------------------------
def _strings(prims, width):
    from distributional_rl_navigation_amd import render
    p = render.prims_to_numpy(prims)
    assert (p["kind"] == GLYPH).all()
    codes = (p["half_width_px"] & 255).reshape(-1, width)
    return ["".join(chr(c) for c in row) for row in codes], p


@pytest.mark.parametrize("decimals", (0, 1, 2, 3))
def test_numbers_equal_python_formatting(decimals):
    from distributional_rl_navigation_amd import render
    rng = np.random.RandomState(40 + decimals)
    v = np.concatenate([rng.uniform(-1e6, 1e6, 300), rng.uniform(-100, 100, 100), rng.normal(0, 1, 90), [0.0, -0.0, 1.0, -1.0, 999999.0, -999999.0, 9.5 + 1e-3, 0.04, -0.96, 99.996]])
    scaled = np.abs(v) * 10 ** decimals
    off_tie = np.abs(scaled - np.floor(scaled) - 0.5) > 1e-6
    signed_zero = (np.signbit(v)) & (np.floor(scaled + 0.5) == 0)      # a negative that rounds to zero keeps no sign here: by the rule, below
    v = v[off_tie & ~signed_zero]
    width = 12
    got, p = _strings(render.numbers(torch.from_numpy(v), decimals, width, [3.0, 4.0], 7), width)
    want = [f"{x:.{decimals}f}".rjust(width) for x in v]
    assert len(p) == len(v) * width and len(v) >= 480
    assert got == want, [(g, w) for g, w in zip(got, want) if g != w][:5]


def test_numbers_by_the_rule():
    from distributional_rl_navigation_amd import render
    nan, inf = float("nan"), float("inf")
    one = lambda v, d, w: _strings(render.numbers(torch.tensor(v, dtype=torch.float64), d, w, [0.0, 0.0], 1), w)[0]
    assert one([0.125, -0.125, 0.375], 2, 6) == ["  0.13", " -0.13", "  0.38"]      # ties go up (Python: 0.12, -0.12, 0.38)
    assert one([2.5, 3.5, -2.5, 0.5, -0.5], 0, 3) == ["  3", "  4", " -3", "  1", " -1"]
    assert one([-0.001, -0.004, -0.005, 0.0, -0.0], 2, 5) == [" 0.00", " 0.00", "-0.01", " 0.00", " 0.00"]      # no minus sign on a zero
    assert one([123.0, 1234.0, -123.0, 12.34, 9.996], 1, 5) == ["123.0", "#####", "#####", " 12.3", " 10.0"]      # the text does not fit: all '#'
    assert one([nan, inf, -inf, 1e15, -1e15, 9.99e14], 0, 16) == ["#" * 16] * 5 + [" 999000000000000"]
    assert one([7.0, 7.4, 12.0, -3.0, 0.0], 0, 1) == ["7", "7", "#", "#", "0"]
    assert one([0.5], 1, 1) == ["#"] and one([0.5], 1, 3) == ["0.5"]
    for bad in (dict(decimals=4, width=8), dict(decimals=-1, width=8), dict(decimals=1, width=0)):
        with pytest.raises(ValueError):
            render.numbers(torch.zeros(1), anchor=[0.0, 0.0], color_z=1, **bad)
    # the record count is P * width whatever the values
    for vals in ([0.0] * 7, [nan] * 7, [1e9, -1e-9, 3.0, inf, 5.5, -7.25, 1e14]):
        assert render.numbers(torch.tensor(vals, dtype=torch.float64), 2, 9, torch.zeros(7, 2), 1).shape == (7 * 9, 48)


def test_number_records_positions():
    from distributional_rl_navigation_amd import render
    anchors = torch.tensor([[1.0, 2.0], [3.0, 4.0]], dtype=torch.float64)
    got, p = _strings(render.numbers(torch.tensor([1.5, -22.25]), 2, 6, anchors, [5, 6], scale=2, align="right", dx=-1, dy=3, image_first=[0, 1]), 6)
    assert got == ["  1.50", "-22.25"]
    p = p.reshape(2, 6)
    assert (p["x0"] == [[1.0], [3.0]]).all() and (p["y0"] == [[2.0], [4.0]]).all() and (p["y1"] == 3.0).all() and (p["half_width_px"] >> 8 == 2).all()
    assert p["x1"][0].tolist() == [-1 - (6 * 12 - 2) + 12 * i for i in range(6)]      # the last cell's 10 pixels end at the anchor's pixel + dx
    assert p["color_z"].tolist() == [[5] * 6, [6] * 6] and p["image_first"].tolist() == [[0] * 6, [1] * 6] == p["image_last"].tolist()


def test_text_records():
    from distributional_rl_navigation_amd import render
    p = render.prims_to_numpy(render.text("Hi there\nyou", [4.0, 5.0], render.word(0x102030, 9), scale=2, dx=3, dy=-1, image_first=1, image_last=4))
    assert len(p) == 8 + 3 and (p["kind"] == GLYPH).all() and "".join(chr(c & 255) for c in p["half_width_px"]) == "Hi thereyou"
    assert (p["half_width_px"] >> 8 == 2).all() and (p["x0"] == 4.0).all() and (p["y0"] == 5.0).all() and (p["color_z"] == 0x09102030).all()
    assert p["x1"].tolist() == [3 + 12 * i for i in range(8)] + [3 + 12 * i for i in range(3)] and p["y1"].tolist() == [-1] * 8 + [-1 + 18] * 3
    assert (p["image_first"] == 1).all() and (p["image_last"] == 4).all()
    r = render.prims_to_numpy(render.text("abc\nz", [0.0, 0.0], 1, align="right"))
    assert r["x1"].tolist() == [-17, -11, -5, -5] and r["y1"].tolist() == [0, 0, 0, 9]      # every line ends at the anchor: 3 * 6 - 1 = 17 pixels wide
    c = render.prims_to_numpy(render.text("abc", [0.0, 0.0], 1, scale=3, align="centre"))
    assert c["x1"].tolist() == [-25, -7, 11]      # 3 * 18 - 3 = 51 pixels, 25 left of the anchor
    assert render.text("", [0.0, 0.0], 1).shape == (0, 48) and render.text("\n\n", [0.0, 0.0], 1).shape == (0, 48)
    many = render.prims_to_numpy(render.text("ok", torch.tensor([[1.0, 1.0], [2.0, 2.0], [3.0, 3.0]]), [1, 2, 3], image_first=[0, 1, 2]))
    assert many["x0"].tolist() == [1, 1, 2, 2, 3, 3] and many["color_z"].tolist() == [1, 1, 2, 2, 3, 3] and many["image_last"].tolist() == [0, 0, 1, 1, 2, 2]
    assert chr(render.prims_to_numpy(render.text("\t", [0.0, 0.0], 1))["half_width_px"][0] & 255) == "?"
    with pytest.raises(ValueError):
        render.text("a", [0.0, 0.0], 1, scale=9)
    with pytest.raises(ValueError):
        render.text("a", [0.0, 0.0], 1, align="up")


def test_choose_text_records():
    from distributional_rl_navigation_amd import render
    got, p = _strings(render.choose_text(["a: -0.40", "w:  0.52", "x"], torch.tensor([1, 0, 2, 1, 7, -1]), torch.zeros(6, 2), 3, image_first=torch.arange(6)), 8)
    assert got == ["w:  0.52", "a: -0.40", "x       ", "w:  0.52", " " * 8, " " * 8]
    assert p["image_first"].reshape(6, 8)[:, 0].tolist() == list(range(6)) and p["x1"].reshape(6, 8)[3].tolist() == [6 * i for i in range(8)]
    with pytest.raises(ValueError):
        render.choose_text([], torch.tensor([0]), torch.zeros(1, 2), 1)


def test_other_builders_pack_records():
    from distributional_rl_navigation_amd import render
    p = render.prims_to_numpy(torch.cat((
        render.rects([[1.0, 2.0]], [[3.0, 0.5]], 9, 2, 3), render.markers([[1.0, 2.0], [3.0, 4.0]], "cross", 4, 1, [5, 6], [0, 1]),
        render.markers([[0.0, 0.0]], 1, 99, 2.5, 1), render.sectors([[0.0, 0.0]], [[0.0, 5.0]], 0.9 * math.pi / 2, 8),
        render.sectors([[0.0, 0.0]] * 3, [[1.0, 1.0]] * 3, 0.0, 8), render.sectors([[0.0, 0.0]], [[1.0, 1.0]], math.pi, 8))))
    assert p["kind"].tolist() == [RECT, MARKER, MARKER, MARKER, SECTOR, SECTOR, SECTOR, SECTOR, SECTOR]
    assert p[0].tolist()[:6] == (1.0, 2.0, 3.0, 0.5, 2, 3) and p[1].tolist()[:4] == (1.0, 2.0, 2.0, 1.0) and p["half_width_px"][1:4].tolist() == [4, 4, 99]
    assert p[3].tolist()[:4] == (0.0, 0.0, 1.0, 2.5) and p["color_z"][1:3].tolist() == [5, 6] and p["image_first"][1:3].tolist() == [0, 1]
    assert p["half_width_px"][4] == round((math.cos(0.9 * math.pi / 2) + 1) * 16384) and p["half_width_px"][5:8].tolist() == [32768] * 3 and p["half_width_px"][8] == 0
    view, size = (0.0, 0.0, 40.0, 20.0), (80, 20)      # half a unit per pixel across, one unit down
    a = render.prims_to_numpy(render.arrows([[10.0, 10.0], [5.0, 5.0]], [[20.0, 10.0], [5.0, 5.0]], 10, [1, 2], view, size, [0, 1], half_width=1))
    assert len(a) == 6 and (a["kind"] == 0).all() and (a["half_width_px"] == 1).all() and a["color_z"].tolist() == [1, 1, 1, 2, 2, 2] and a["image_first"].tolist() == [0] * 3 + [1] * 3
    assert a[0].tolist()[:4] == (10.0, 10.0, 20.0, 10.0) and (a["x0"][1:3] == 20.0).all() and (a["y0"][1:3] == 10.0).all()
    # the strokes go back along the shaft by 10 cos pixels = 0.5 units each and sideways by 10 sin pixels = 1 unit each
    c, s = 2 / math.sqrt(5), 1 / math.sqrt(5)
    assert np.allclose(a["x1"][1:3], 20.0 - 10 * c * 0.5, atol=1e-12) and np.allclose(sorted(a["y1"][1:3]), [10.0 - 10 * s, 10.0 + 10 * s], atol=1e-12)
    assert np.isnan(a["x1"][4:6]).all() and a[3].tolist()[:4] == (5.0, 5.0, 5.0, 5.0)      # no length: no head


# ---- the panels' bookkeeping, with stand-ins for the device calls ---------------------------------------------------------------------------------
class FakeCanvas:
    """What a panel asks of a canvas, recording instead of drawing."""

    def __init__(self, n_images):
        self.n_images, self.log = n_images, []

    def draw(self, prims):
        self.log.append(prims)
        return self


def _glyph_lines(p):
    """The GLYPH records of a buffer as {(image_first, image_last, pixel row offset): text}, the characters of a line in order of their offset."""
    g = p[p["kind"] == GLYPH]
    out = {}
    for rec in sorted(g, key=lambda r: (int(r["image_first"]), int(r["image_last"]), float(r["y0"]), float(r["y1"]), float(r["x0"]), float(r["x1"]))):
        out.setdefault((int(rec["image_first"]), int(rec["image_last"]), float(rec["y0"]), float(rec["y1"])), []).append(chr(int(rec["half_width_px"]) & 255))
    return {k: "".join(v) for k, v in out.items()}


def hand_made_quantiles():
    q = np.zeros((2, 32, 9))
    rng = np.random.RandomState(8)
    q[0] = rng.normal(0.0, 2.0, (32, 9)) + np.arange(9) * 1.5      # frame 0: the last action has the largest mean
    q[1] = rng.normal(0.0, 2.0, (32, 9)) - np.abs(np.arange(9) - 3) * 2.0      # frame 1: action 3
    q[0, 5, 2], q[0, 7, 6], q[1, 0, 0], q[1, 9, 8] = -21.5, 33.5, -40.5, 12.5      # the frames' extremes: exact in binary and at one decimal
    return q


def test_return_dist_panel_records():
    from distributional_rl_navigation_amd import _capi, render, render_panels
    q = hand_made_quantiles()
    params = _capi.default_params()
    canvas = FakeCanvas(2)
    width, height = 160, 120
    assert render_panels.return_dist_panel(torch.from_numpy(q), torch.tensor([0.37, 1.0]), "adaptive phi = ", width, height, params=params, canvas=canvas) is canvas
    (prims,) = canvas.log
    p = render.prims_to_numpy(prims)
    count = lambda k: int((p["kind"] == k).sum())
    # 9 baselines for all frames + 9 min-max lines per frame; 9 mean bars and 32 * 9 crosses per frame; no disc, ring or sector
    assert (count(0), count(1), count(2), count(RECT), count(MARKER), count(SECTOR)) == (9 + 2 * 9, 0, 0, 2 * 9, 2 * 288, 0)
    assert np.isfinite(np.stack([p[k] for k in ("x0", "y0", "x1", "y1")])).all()      # nothing is a break here
    base = p[(p["kind"] == 0) & (p["image_last"] - p["image_first"] == 1)]
    assert len(base) == 9 and (base["x0"] < base["x1"]).all() and len(set(base["y0"])) == 9 and (base["y0"] == base["y1"]).all()
    rows_y = np.sort(base["y0"])
    means = q.mean(axis=1)
    for f in range(2):
        marks = p[(p["kind"] == MARKER) & (p["image_first"] == f)]
        assert len(marks) == 288 and (marks["image_last"] == f).all() and (marks["x1"] == 2.0).all()      # crosses, into image f alone
        assert (marks["color_z"] & 0xFFFFFF == render_panels.GREEN).all()
        bars = p[(p["kind"] == RECT) & (p["image_first"] == f)]
        assert len(bars) == 9 and (bars["image_last"] == f).all()
        red = bars[bars["color_z"] & 0xFFFFFF == render_panels.RED]
        assert len(red) == 1 and ((bars["color_z"] & 0xFFFFFF == render_panels.BLUE).sum() == 8)
        best = int(means[f].argmax())
        assert best == (8, 3)[f]
        assert abs((red["y0"][0] + red["y1"][0]) / 2 - rows_y[best]) < 1e-9      # the red bar sits on the argmax row
        row_h = rows_y[1] - rows_y[0]
        assert abs((red["y1"][0] - red["y0"][0]) - 2 * 0.35 * row_h) < 1e-9      # +-0.35 rows
        blue_w = (bars["x1"] - bars["x0"])[bars["color_z"] & 0xFFFFFF == render_panels.BLUE]
        assert (red["x1"][0] - red["x0"][0]) > blue_w.max()      # ... and is wider
        # the crosses map the frame's own limits min - 5 .. max + 5 onto the baselines' extent
        lo, hi = q[f].min() - 5.0, q[f].max() + 5.0
        x = base["x0"][0] + (q[f] - lo) / (hi - lo) * (base["x1"][0] - base["x0"][0])
        assert np.allclose(np.sort(marks["x0"]), np.sort(x.ravel()), atol=1e-9) and (marks["x0"] > base["x0"][0]).all() and (marks["x0"] < base["x1"][0]).all()
    lines = _glyph_lines(p)
    texts = {k: v for k, v in lines.items()}
    per_frame = lambda f: sorted(t for k, v in texts.items() if k[0] == f and k[1] == f for t in v.split())
    assert per_frame(0) == sorted(["0.37", "-26.5", "38.5"]) and per_frame(1) == sorted(["1.00", "-45.5", "17.5"])      # the title's number, min - 5, max + 5
    both = [v for k, v in texts.items() if (k[0], k[1]) == (0, 1)]
    assert "adaptive phi = " in both and sum(v.count(",") for v in both) == 9      # the title's words and the nine compact action labels


def test_limit_label_of_a_tie_rounds_up_in_size():
    from distributional_rl_navigation_amd import render
    got = ["".join(chr(c) for c in row) for row in render.number_codes(torch.tensor([-26.25, 17.75]), 1, 8).tolist()]
    assert got == ["   -26.3", "    17.8"]


def test_panel_of_equal_quantiles_draws():
    from distributional_rl_navigation_amd import _capi, render, render_panels
    q = torch.full((1, 32, 9), 4.0, dtype=torch.float64)
    p = render.prims_to_numpy(render_panels.return_dist_prims(q, 1.0, width=160, height=120, params=_capi.default_params()))
    assert np.isfinite(np.stack([p[k] for k in ("x0", "y0", "x1", "y1")])).all()      # limits -1 .. 9: no division by zero
    marks = p[p["kind"] == MARKER]
    assert len(marks) == 288 and len(set(marks["x0"])) == 1
    assert (p[p["kind"] == RECT]["color_z"] & 0xFFFFFF == render_panels.RED).sum() == 1      # argmax of equal means: one row, the first
    lines = _glyph_lines(p)
    assert sorted(t for v in lines.values() for t in v.split() if t in ("-1.0", "9.0", "1.00")) == ["-1.0", "1.00", "9.0"]
    same = render.prims_to_numpy(render_panels.return_dist_prims(q, 1.0, width=160, height=120, xlim=(4.0, 4.0), labels=False))
    assert np.isfinite(np.stack([same[k] for k in ("x0", "y0", "x1", "y1")])).all()      # a degenerate axis given by hand: still no NaN


def test_shared_limits_and_q_values():
    from distributional_rl_navigation_amd import _capi, render, render_panels
    q = hand_made_quantiles()
    other = q * 2.0 + 30.0
    lo, hi = render_panels.shared_limits([torch.from_numpy(q), torch.from_numpy(other)])
    assert lo.tolist() == [min(q[f].min(), other[f].min()) - 5.0 for f in range(2)] and hi.tolist() == [max(q[f].max(), other[f].max()) + 5.0 for f in range(2)]
    a = render.prims_to_numpy(render_panels.return_dist_prims(torch.from_numpy(q), 1.0, width=160, height=120, xlim=(lo, hi), labels=False))
    b = render.prims_to_numpy(render_panels.return_dist_prims(torch.from_numpy(other), 0.5, width=160, height=120, xlim=(lo, hi), labels=False))
    la, lb = _glyph_lines(a), _glyph_lines(b)
    limits = lambda lines, f: sorted(t for k, v in lines.items() if (k[0], k[1]) == (f, f) for t in v.split() if t not in ("1.00", "0.50"))
    assert limits(la, 0) == limits(lb, 0) == sorted(["-26.5", "102.0"]) and limits(la, 1) == limits(lb, 1) == sorted(["-56.0", "60.0"]) and "1.00" in [v.strip() for v in la.values()] and "0.50" in [v.strip() for v in lb.values()]
    qv = torch.tensor([[1.0, 2.0, 9.0, 3.0, 4.0, 5.0, 6.0, 7.0, 8.0], [-1.0] * 9])
    p = render.prims_to_numpy(render_panels.q_values_prims(qv, width=160, height=300, params=_capi.default_params()))
    assert (p["kind"] == RECT).sum() == 18 and (p["kind"] == MARKER).sum() == 0 and (p["kind"] == 0).sum() == 9
    red = p[(p["kind"] == RECT) & (p["color_z"] & 0xFFFFFF == render_panels.RED)]
    assert red["image_first"].tolist() == [0, 1]
    lines = list(_glyph_lines(p).values())
    assert "Action Values" in lines and "a: -0.40" in lines and "w: 0.52" in lines and {"-4.0", "14.0", "-6.0", "4.0"} <= {t for v in lines for t in v.split()}


def test_sonar_velocity_goal_action_records():
    from distributional_rl_navigation_amd import _capi, render, render_panels
    params = _capi.default_params()
    obs = torch.zeros(3, 26, dtype=torch.float64)
    obs[:, 0], obs[:, 1], obs[:, 2], obs[:, 3] = torch.tensor([1.0, 0.0, -3.0]), torch.tensor([0.5, 0.0, 4.0]), torch.tensor([12.5, -3.25, 0.0]), torch.tensor([-7.0, 40.125, 0.0])
    obs[0, 4:6] = torch.tensor([5.0, 0.0])      # frame 0: beam 0 hits five units ahead
    obs[2, 4:8] = torch.tensor([0.0, 2.0, 3.0, -4.0])      # frame 2: one hit to the left, one ahead and to the right
    p = render.prims_to_numpy(render_panels.sonar_prims(obs, 10.0, math.pi / 3, 120, 120))
    wedge = p[p["kind"] == SECTOR]
    assert len(wedge) == 3 and wedge["image_first"].tolist() == [0, 1, 2] == wedge["image_last"].tolist() and (wedge["color_z"] >> 24 == render_panels.Z_TINT).all()
    assert len(set(wedge.tolist())) == 3 and len({r[:4] for r in wedge.tolist()}) == 1      # the same wedge, one record per frame
    assert wedge["x0"][0] == wedge["x1"][0] == 60.0 and wedge["half_width_px"][0] == render.sector_cosine(math.pi / 3) == 24576
    k = (wedge["y1"][0] - wedge["y0"][0]) / 10.0      # pixels per unit
    hits = p[p["kind"] == 1].reshape(3, 11)
    assert (hits["image_first"] == np.arange(3)[:, None]).all() and np.isfinite(hits["x0"]).sum() == 3      # every miss is a NaN record
    assert (hits["x0"][0, 0], hits["y0"][0, 0]) == (60.0, wedge["y0"][0] + 5.0 * k)      # (x, y) = (5, 0) -> (-y, x): straight up
    assert np.allclose([hits["x0"][2, 0], hits["y0"][2, 0], hits["x0"][2, 1], hits["y0"][2, 1]], [60.0 - 2.0 * k, wedge["y0"][0], 60.0 + 4.0 * k, wedge["y0"][0] + 3.0 * k])
    assert "LiDAR Reflections" in _glyph_lines(p).values()
    v = render.prims_to_numpy(render_panels.velocity_prims(obs, 120, 120))
    seg = v[v["kind"] == 0].reshape(2, 3, 3)      # [steer, velocity][frame][shaft, two head strokes]
    assert (seg["image_first"] == np.arange(3)[None, :, None]).all() and (seg["x0"][:, :, 0] == 60.0).all()
    scale = seg["y1"][0, :, 0] - seg["y0"][0, :, 0]      # the steer arrow is one unit long: pixels per unit of each frame
    assert scale[0] == scale[1] and scale[2] < scale[0]      # |v| <= 2: the fixed limits; frame 2 (v = (-3, 4)) zooms out
    assert np.allclose(seg["x1"][1, :, 0] - 60.0, -obs[:, 1].numpy() * scale) and np.allclose(seg["y1"][1, :, 0] - seg["y0"][1, :, 0], obs[:, 0].numpy() * scale)
    assert np.isnan(seg["x1"][1, 1, 1:]).all() and np.isfinite(seg["x1"][1, 0]).all()      # no velocity: no head
    assert abs(scale[2] * 8.0 - 120.0) < 1e-9      # xr = |v_y| = 4: 8 units across the 120 pixels
    lines = list(_glyph_lines(v).values())
    assert "Velocity Measurement" in lines and "- steer direction" in lines and "- velocity wrt seafloor" in lines
    g = _glyph_lines(render.prims_to_numpy(render_panels.goal_prims(obs, 200, 60)))
    assert "Goal Position (Relative)" in g.values()
    nums = lambda f: sorted(t for k, v in g.items() if k[0] == k[1] == f for t in v.split())
    assert nums(0) == ["-7.00", "12.50"] and nums(1) == ["-3.25", "40.13"] and nums(2) == ["0.00", "0.00"]
    a = _glyph_lines(render.prims_to_numpy(render_panels.action_prims(torch.tensor([0, 5, -1]), params, 100, 80)))
    texts = sorted((k[0], v) for k, v in a.items() if k[0] == k[1])
    assert texts == [(0, "a: -0.40"), (0, "w: -0.52"), (1, "a: 0.00 "), (1, "w: 0.52 "), (2, " " * 8), (2, " " * 8)] and "Action" in a.values()


def test_video_layouts():
    from distributional_rl_navigation_amd import render_panels
    for kind, n_dist, names in (("iqn", 2, ("title", "goal", "sonar", "velocity", "map", "dist0", "dist1")), ("dqn", 1, ("title", "goal", "sonar", "velocity", "map", "q")),
                                ("planner", 1, ("title", "goal", "sonar", "velocity", "map", "action"))):
        for size in ((1920, 1080), (240, 135), (97, 61)):
            slots = render_panels.video_layout(kind, size, n_dist)
            assert tuple(slots) == names
            taken = np.zeros((size[1], size[0]), int)
            for x, y, w, h in slots.values():
                assert w >= 1 and h >= 1 and x >= 0 and y >= 0 and x + w <= size[0] and y + h <= size[1]
                taken[y:y + h, x:x + w] += 1
            assert taken.max() == 1      # no two parts share a pixel
            assert slots["map"][2] == slots["map"][3]
    s = render_panels.video_layout("iqn", (1920, 1080), 2)
    assert s["title"] == (0, 0, 1920, 308) and s["dist1"] == (1536, 308, 384, 772) and s["map"] == (384 + (768 - 768) // 2, 308 + 2, 768, 768)
    with pytest.raises(ValueError):
        render_panels.video_layout("sheet", (10, 10))
