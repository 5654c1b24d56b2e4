"""Pictures (mn_render_worlds / mn_render_draw, csrc/mn_render_body.h, render.py) as far as they go without a GPU: the C-ABI declarations and their
ctypes bindings, the compiled resources of the two kernels (hipcc cross-compiles gfx950), the raster body itself -- it is __host__ __device__, so
tests/render_host.hip runs it on the CPU -- against an independent numpy restatement of the rules in include/marinenav_hip.h (written here from the
rules, not from the body: same operation order, cores summed in order of distance with ties by index), the PNG writer, and the bookkeeping of
episode_sheet / episode_frames with stand-ins for the device calls.
Bound: EQUAL pixel words.  np.sqrt and elementwise float64 operations are correctly rounded, so the twin and the body compute the same bits; the only
pixels the field comparison may leave out are threshold-fragile ones (the twin's t within 1e-9 of an integer, or |d^2 - r^2| < 1e-9 at an obstacle),
at most 4 per image, and their number is printed (it is 0 on these worlds and sizes).  The LIC images are compared in full."""
import ctypes as C
import json
import math
import os
import re
import struct
import subprocess
import zlib

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "distributional_rl_navigation_amd", "csrc")
G = os.path.join(ROOT, "tests", "golden")
HIPCC = "/opt/rocm/bin/hipcc"
WORLDS = (0, 10, 20, 29)
SIZES = ((96, 64), (67, 45), (128, 128))
WHOLE = (0.0, 0.0, 50.0, 50.0)


def _header():
    with open(os.path.join(ROOT, "include", "marinenav_hip.h")) as f:
        return f.read()


def _args(text, name):
    m = re.search(r"\bint " + name + r"\(([^;]*)\);", text)
    assert m, f"{name} is not declared in include/marinenav_hip.h"
    return [re.sub(r"\s+", " ", a).strip() for a in m.group(1).split(",")]


def _struct_bytes(text, name):
    """sizeof of a typedef struct of the header made of double / int32_t / uint32_t / uint16_t members (natural alignment, 8 at the end)."""
    m = re.search(r"typedef struct " + name + r" \{(.*?)\} " + name + ";", text, flags=re.S)
    assert m, name
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    consts = {k: int(v) for k, v in re.findall(r"#define (MN_RENDER_[A-Z_]+) (\d+)", text)}
    size = {"double": 8, "int32_t": 4, "uint32_t": 4, "uint16_t": 2}
    at = 0
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        ty, names = decl.split(None, 1)
        for nm in names.split(","):
            k = re.search(r"\[(\w+)\]", nm)
            count = (consts[k.group(1)] if not k.group(1).isdigit() else int(k.group(1))) if k else 1
            at = (at + size[ty] - 1) // size[ty] * size[ty] + size[ty] * count
    return (at + 7) // 8 * 8


def test_render_symbols_declared_and_bound():
    from distributional_rl_navigation_amd import _capi
    text = _header()
    assert _args(text, "mn_render_worlds") == ["mn_handle *h", "const int32_t *env_of_image_dev", "int32_t env0", "int32_t n_images", "int32_t width",
                                               "int32_t height", "const double view[4]", "const mn_render_style *style", "uint32_t *pixels_dev", "void *stream"]
    assert _args(text, "mn_render_draw") == ["uint32_t *pixels_dev", "int32_t n_images", "int32_t width", "int32_t height", "const double view[4]",
                                             "const mn_render_prim *prims_dev", "int64_t n_prims", "void *stream"]
    sig = {n: (r, a) for n, r, a in _capi.SIGNATURES}
    p, i32, i64, pd = C.c_void_p, C.c_int32, C.c_int64, C.POINTER(C.c_double)
    assert sig["mn_render_worlds"] == (C.c_int, [p, p, i32, i32, i32, i32, pd, C.POINTER(_capi.MnRenderStyle), p, p])
    assert sig["mn_render_draw"] == (C.c_int, [p, i32, i32, i32, pd, p, i64, p])
    assert C.sizeof(_capi.MnRenderPrim) == _struct_bytes(text, "mn_render_prim") == 48
    assert C.sizeof(_capi.MnRenderStyle) == _struct_bytes(text, "mn_render_style") == 192
    assert [f[0] for f in _capi.MnRenderPrim._fields_] == ["x0", "y0", "x1", "y1", "image_first", "image_last", "color_z", "kind", "half_width_px"]
    for name, value in (("MN_RENDER_SEGMENT", _capi.RENDER_SEGMENT), ("MN_RENDER_DISC", _capi.RENDER_DISC), ("MN_RENDER_RING", _capi.RENDER_RING)):
        m = re.search(name + r" = (\d+)", text)
        assert m and int(m.group(1)) == value, name
    for name, value in (("MN_RENDER_MAX_LEVELS", _capi.RENDER_MAX_LEVELS), ("MN_RENDER_MAX_LIC_STEPS", _capi.RENDER_MAX_LIC_STEPS),
                        ("MN_RENDER_MAX_HALF_WIDTH", _capi.RENDER_MAX_HALF_WIDTH)):
        m = re.search(r"#define " + name + r" (\d+)", text)
        assert m and int(m.group(1)) == value, name


def test_render_kernels_resources():
    """No scratch, no register spills (vector or scalar), at most 256 registers.  The message carries the figures DESIGN records."""
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-I../../include", "-I.", "--cuda-device-only", "-ffp-contract=off",
                        "-Rpass-analysis=kernel-resource-usage", "-c", "-o", "/dev/null", "mn_render.hip"], cwd=CSRC, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    usage, cur = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"remark: .*Function Name: (\S+)", line)
        if m:
            cur = usage.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:.*?\s([A-Za-z][A-Za-z ]*?)(?: \[[^\]]*\])?: (\d+)", line)
        if m and cur is not None:
            cur[m.group(1).strip()] = int(m.group(2))
    assert sorted(k.split("kernel")[0] for k in usage) == ["_Z21mn_render_draw_", "_Z23mn_render_worlds_"], list(usage)
    figures = "; ".join(f"{k}: VGPRs {v['VGPRs']}, SGPRs {v['TotalSGPRs']}, LDS {v['LDS Size']}, scratch {v['ScratchSize']}, spills "
                        f"{v['VGPRs Spill']} + {v['SGPRs Spill']}" for k, v in usage.items())
    print(figures)
    for v in usage.values():
        assert v["ScratchSize"] == 0 and v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0, figures
        assert v["VGPRs"] + v.get("AGPRs", 0) <= 256, figures


# ---- the host program -------------------------------------------------------------------------------------------------------------------------------
WORLD_REC = np.dtype([("nc", "<i4"), ("no", "<i4"), ("cores", "<f8", (8, 3)), ("obst", "<f8", (10, 3)), ("start", "<f8", (2,)), ("goal", "<f8", (2,))])
assert WORLD_REC.itemsize == 8 + 8 * (24 + 30 + 4)


def build_host(out_dir, extra=()):
    exe = os.path.join(str(out_dir), "render_host")
    r = subprocess.run([HIPCC, "--cuda-host-only", "-O2", "-std=c++17", "-ffp-contract=off", *extra, "-I" + os.path.join(ROOT, "include"), "-I" + CSRC,
                        "-o", exe, os.path.join(ROOT, "tests", "render_host.hip")], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    return build_host(tmp_path_factory.mktemp("render_host"))


def eval_worlds():
    """The 30 worlds of the evaluation config as dicts: cores [nc][3] = x, y, signed Gamma (+ if clockwise), obstacles [no][3], start, goal."""
    with open(os.path.join(G, "eval_config_seed3.json")) as f:
        cfg = json.load(f)
    out = []
    for k in range(len(cfg)):
        e = cfg[f"env_{k}"]["env"]
        pos, cw, gm = np.array(e["cores"]["positions"], dtype=np.float64).reshape(-1, 2), np.array(e["cores"]["clockwise"]), np.array(e["cores"]["Gamma"], dtype=np.float64)
        cores = np.concatenate([pos, np.where(cw > 0, gm, -gm)[:, None]], axis=1) if len(pos) else np.zeros((0, 3))
        ob = np.concatenate([np.array(e["obstacles"]["positions"], dtype=np.float64).reshape(-1, 2), np.array(e["obstacles"]["r"], dtype=np.float64)[:, None]], axis=1)
        out.append(dict(cores=cores, obstacles=ob, start=np.array(e["start"], dtype=np.float64), goal=np.array(e["goal"], dtype=np.float64)))
    return out


def world_records(worlds):
    """`worlds`: dicts as eval_worlds() gives them, or None for an index that is no world."""
    rec = np.zeros(len(worlds), dtype=WORLD_REC)
    for i, w in enumerate(worlds):
        if w is None:
            rec["nc"][i] = -1
            continue
        nc, no = len(w["cores"]), len(w["obstacles"])
        rec["nc"][i], rec["no"][i] = nc, no
        rec["cores"][i, :nc], rec["obst"][i, :no], rec["start"][i], rec["goal"][i] = w["cores"], w["obstacles"], w["start"], w["goal"]
    return rec


def cmp_style(lic, lic_steps=12, **kw):
    """The style of the comparisons: 16 levels, v_max 2.0, as the issue sets them."""
    from distributional_rl_navigation_amd import render
    return render.Style(v_max=2.0, lic=bool(lic), lic_steps=lic_steps, hpx=1.0, lic_floor=96, seed=7, **kw)



def run_host(exe, tmp_path, tag, width, height, view, style=None, worlds=None, n_images=None, prims=None, fill=0, spec=None):
    """The host program's (pixels [I][H][W] uint32, items, most items of one primitive in one image).  `worlds`: dicts / None per image -> the
    world layers are rendered; else `n_images` images start as `fill`.  `prims`: a record array (render.PRIM_DTYPE) or a [P][48] uint8 tensor."""
    from distributional_rl_navigation_amd import _capi, render
    p = _capi.default_params()
    for k, v in (spec or {}).items():
        setattr(p, k, v)
    style = style or cmp_style(False)
    n = len(worlds) if worlds is not None else int(n_images)
    rec = world_records(worlds) if worlds is not None else np.zeros(n, dtype=WORLD_REC)
    pb = b"" if prims is None else (prims.tobytes() if isinstance(prims, np.ndarray) else prims.cpu().numpy().tobytes())
    assert len(pb) % 48 == 0
    fin, fout = str(tmp_path / f"{tag}.in"), str(tmp_path / f"{tag}.out")
    with open(fin, "wb") as f:
        f.write(struct.pack("<5iI2i", n, width, height, len(pb) // 48, int(worlds is not None), fill, 0, 0))
        f.write(np.array(view, dtype="<f8").tobytes())
        f.write(bytes(p))
        f.write(bytes(style.to_c()))
        f.write(rec.tobytes())
        f.write(pb)
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    raw = open(fout, "rb").read()
    px = np.frombuffer(raw[:4 * n * width * height], dtype="<u4").reshape(n, height, width)
    items, most = struct.unpack("<2q", raw[4 * n * width * height:])
    return px, items, most


# ---- the twin: the rules of include/marinenav_hip.h in numpy ----------------------------------------------------------------------------------------
CORE_R, GOAL_DIS, MAP_W, MAP_H = 0.5, 2.0, 50.0, 50.0
TWO_PI = 2 * math.pi
TWO_PI_R_R = 2 * math.pi * CORE_R * CORE_R


def twin_velocity(cores, x, y):
    """get_velocity (marinenav_env.py:422-455) at the points (x, y): every core's contribution, added in order of distance (ties by index)."""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    if len(cores) == 0:
        return np.zeros_like(x), np.zeros_like(x)
    with np.errstate(all="ignore"):
        d, ux, uy = [], [], []
        for cx, cy, cg in cores:
            rx, ry = cx - x, cy - y
            dis = np.sqrt(rx * rx + ry * ry)
            rx, ry = rx / dis, ry / dis
            gamma = abs(cg)
            if cg > 0.0:      # clockwise: tangent = [[0, -1], [1, 0]] r
                tx, ty = 0. * rx + -1. * ry, 1. * rx + 0. * ry
            else:
                tx, ty = 0. * rx + 1. * ry, -1. * rx + 0. * ry
            speed = np.where(dis <= CORE_R, gamma / TWO_PI_R_R * dis, gamma / (TWO_PI * dis))
            d.append(dis); ux.append(tx * speed); uy.append(ty * speed)
        d, ux, uy = np.stack(d), np.stack(ux), np.stack(uy)
        order = np.argsort(d, axis=0, kind="stable")
        ux, uy = np.take_along_axis(ux, order, axis=0), np.take_along_axis(uy, order, axis=0)
        vx, vy = np.zeros_like(x), np.zeros_like(x)
        for q in range(len(cores)):
            vx = vx + ux[q]
            vy = vy + uy[q]
    return vx, vy


def twin_noise(c, r, seed):
    M = np.uint64(0xFFFFFFFF)
    c, r = np.asarray(c).astype(np.int64).astype(np.uint64) & M, np.asarray(r).astype(np.int64).astype(np.uint64) & M
    h = ((c * np.uint64(0x9E3779B1)) & M) ^ ((r * np.uint64(0x85EBCA77)) & M) ^ np.uint64((int(seed) * 0xC2B2AE3D) & 0xFFFFFFFF)
    h ^= h >> np.uint64(15); h = (h * np.uint64(0x2C1B3C6D)) & M
    h ^= h >> np.uint64(12); h = (h * np.uint64(0x297A2D39)) & M
    h ^= h >> np.uint64(15)
    return (h >> np.uint64(24)).astype(np.int64)


def twin_world(world, width, height, view, style):
    """(words [H][W] uint32, fragile [H][W] bool) of one world's image by the rules; `world` None: an image of `outside`."""
    W, H = int(width), int(height)
    if world is None:
        return np.full((H, W), style.outside, dtype=np.uint32), np.zeros((H, W), bool)
    x0, y0, x1, y1 = (float(a) for a in view)
    sx, sy = (x1 - x0) / W, (y1 - y0) / H
    c, r = np.meshgrid(np.arange(W), np.arange(H), indexing="xy")
    x, y = x0 + (c + 0.5) * sx, y1 - (r + 0.5) * sy
    inside = (x >= 0.0) & (x <= MAP_W) & (y >= 0.0) & (y <= MAP_H)
    n_levels, pal = len(style.palette), np.array(style.palette, dtype=np.int64)
    with np.errstate(all="ignore"):
        vx, vy = twin_velocity(world["cores"], x, y)
        speed = np.sqrt(vx * vx + vy * vy)
        t = speed / style.v_max * n_levels
        top = ~np.isfinite(t) | (t >= n_levels)
        level = np.where(top, n_levels - 1, np.floor(np.where(top, 0.0, t))).astype(np.int64)
        fragile = inside & np.isfinite(t) & (np.abs(t - np.rint(t)) < 1e-9)
        colour = pal[level]
        if style.lic:
            total, count = twin_noise(c, r, style.seed), np.ones((H, W), dtype=np.int64)
            for s in (1.0, -1.0):
                u, v, alive = c + 0.5, r + 0.5, inside.copy()
                for _ in range(int(style.lic_steps)):
                    wx, wy = twin_velocity(world["cores"], x0 + u * sx, y1 - v * sy)
                    sp = np.sqrt(wx * wx + wy * wy)
                    alive = alive & (sp > 0.0) & np.isfinite(sp)
                    u = np.where(alive, u + s * (style.hpx * wx / sp), u)
                    v = np.where(alive, v - s * (style.hpx * wy / sp), v)
                    fu, fv = np.floor(u), np.floor(v)
                    alive = alive & (fu >= 0.0) & (fu < W) & (fv >= 0.0) & (fv < H)
                    total = total + np.where(alive, twin_noise(np.where(alive, fu, 0.0), np.where(alive, fv, 0.0), style.seed), 0)
                    count = count + alive
            g = (2 * total + count) // (2 * count)
            f = style.lic_floor + (255 - style.lic_floor) * g // 255
            colour = ((colour >> 16 & 255) * f // 255) << 16 | ((colour >> 8 & 255) * f // 255) << 8 | ((colour & 255) * f // 255)
        words = np.where(inside, colour, style.outside).astype(np.int64)
        for ox, oy, orad in world["obstacles"]:
            dx, dy = x - ox, y - oy
            d2 = dx * dx + dy * dy
            words = np.where(d2 <= orad * orad, np.maximum(words, 1 << 24 | style.obstacle), words)
            fragile |= np.abs(d2 - orad * orad) < 1e-9
        if style.marker_r > 0.0:
            m2 = style.marker_r * style.marker_r
            sdx, sdy, gdx, gdy = x - world["start"][0], y - world["start"][1], x - world["goal"][0], y - world["goal"][1]
            gd2 = gdx * gdx + gdy * gdy
            rin = GOAL_DIS - max(sx, sy)
            ring = (gd2 <= GOAL_DIS * GOAL_DIS) & ((rin <= 0.0) | (gd2 >= rin * rin))
            words = np.where((sdx * sdx + sdy * sdy <= m2) | (gd2 <= m2) | ring, np.maximum(words, 2 << 24 | style.marker), words)
    return words.astype(np.uint32), fragile


def twin_draw(pixels, view, prims, max_half_width=8):
    """The primitives `prims` (records of render.PRIM_DTYPE) into `pixels` [I][H][W] uint32 by the rules, in plain Python floats.  Returns the
    largest number of samples any segment had."""
    I, H, W = pixels.shape
    x0, y0, x1, y1 = (float(a) for a in view)
    sx, sy = (x1 - x0) / W, (y1 - y0) / H
    fin = math.isfinite
    most = 0

    def put(i0, i1, c, r, word):
        assert 0 <= c < W and 0 <= r < H
        pixels[i0:i1 + 1, r, c] = np.maximum(pixels[i0:i1 + 1, r, c], np.uint32(word))

    def over(a, b):      # a / b as IEEE does it, also for b = 0 and overflow
        with np.errstate(all="ignore"):
            return float(np.float64(a) / np.float64(b))

    for p in prims:
        i0, i1 = max(int(p["image_first"]), 0), min(int(p["image_last"]), I - 1)
        if i0 > i1:
            continue
        kind, word = int(p["kind"]), int(p["color_z"])
        px0, py0, px1, py1 = float(p["x0"]), float(p["y0"]), float(p["x1"]), float(p["y1"])
        if kind == 0:
            hw = min(int(p["half_width_px"]), max_half_width)
            m = float(hw + 1)
            with np.errstate(all="ignore"):
                au, av, bu, bv = over(px0 - x0, sx), over(y1 - py0, sy), over(px1 - x0, sx), over(y1 - py1, sy)
                du, dv = float(np.float64(bu) - np.float64(au)), float(np.float64(bv) - np.float64(av))
            if not all(fin(q) for q in (au, av, bu, bv, du, dv)):
                continue
            ulo, uhi, vlo, vhi = -m, W + m, -m, H + m
            t0, t1, ok = 0.0, 1.0, True
            for pp, qq in ((-du, au - ulo), (du, uhi - au), (-dv, av - vlo), (dv, vhi - av)):
                if pp == 0.0:
                    if qq < 0.0:
                        ok = False
                        break
                    continue
                rr = qq / pp
                if pp < 0.0:
                    if rr > t1:
                        ok = False
                        break
                    t0 = max(t0, rr)
                else:
                    if rr < t0:
                        ok = False
                        break
                    t1 = min(t1, rr)
            if not ok:
                continue
            clamp = lambda a, lo, hi: lo if a < lo else (hi if a > hi else a)
            cau, cav = clamp(au + t0 * du, ulo, uhi), clamp(av + t0 * dv, vlo, vhi)
            cbu, cbv = clamp(au + t1 * du, ulo, uhi), clamp(av + t1 * dv, vlo, vhi)
            eu, ev = cbu - cau, cbv - cav
            n = int(math.ceil(max(abs(eu), abs(ev))))
            most = max(most, n + 1)
            for k in range(n + 1):
                pu, pv = (cau + eu * k / n, cav + ev * k / n) if n else (cau, cav)
                cc, cr = math.floor(pu), math.floor(pv)
                for r in range(max(cr - hw, 0), min(cr + hw, H - 1) + 1):
                    for c in range(max(cc - hw, 0), min(cc + hw, W - 1) + 1):
                        put(i0, i1, c, r, word)
        elif kind in (1, 2):
            rin, rout = (px1, py1) if kind == 2 else (0.0, px1)
            if not all(fin(q) for q in (px0, py0, rin, rout)) or rin < 0.0 or rout < rin:
                continue
            # every pixel of the image is tested: the body's bounding box is its own business, the rule is per pixel centre
            c, r = np.meshgrid(np.arange(W), np.arange(H), indexing="xy")
            with np.errstate(all="ignore"):
                dx, dy = (x0 + (c + 0.5) * sx) - px0, (y1 - (r + 0.5) * sy) - py0
                d2 = dx * dx + dy * dy
                hit = (d2 <= rout * rout) & (d2 >= rin * rin)
            pixels[i0:i1 + 1][:, hit] = np.maximum(pixels[i0:i1 + 1][:, hit], np.uint32(word))
    return most


# ---- worlds against the twin ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def worlds():
    w = eval_worlds()
    assert [len(w[k]["cores"]) for k in WORLDS] == [4, 6, 8, 8]
    return w


@pytest.mark.parametrize("lic", (False, True), ids=("plain", "lic"))
@pytest.mark.parametrize("size", SIZES, ids=[f"{w}x{h}" for w, h in SIZES])
def test_worlds_equal_the_twin(host_program, tmp_path, worlds, size, lic):
    width, height = size
    style = cmp_style(lic)
    got, _, _ = run_host(host_program, tmp_path, "w", width, height, WHOLE, style, [worlds[k] for k in WORLDS])
    for i, k in enumerate(WORLDS):
        want, fragile = twin_world(worlds[k], width, height, WHOLE, style)
        diff = got[i] != want
        print(f"[world {k} {width}x{height} lic={lic}] {int(diff.sum())} differing pixels, {int(fragile.sum())} threshold-fragile")
        if lic:
            assert not diff.any(), (k, np.argwhere(diff)[:5], got[i][diff][:5], want[diff][:5])
        else:
            assert fragile.sum() <= 4 and not (diff & ~fragile).any(), (k, np.argwhere(diff & ~fragile)[:5])
        z = got[i] >> 24
        assert (z == 1).any() and (z == 2).any() and (z == 0).any() and z.max() == 2      # obstacles, markers and water are all in the picture


def test_world_without_cores_is_level_zero_and_its_lic_is_flat(host_program, tmp_path, worlds):
    still = dict(cores=np.zeros((0, 3)), obstacles=np.zeros((0, 3)), start=worlds[0]["start"], goal=worlds[0]["goal"])
    view = (-5.0, -5.0, 55.0, 55.0)
    plain = cmp_style(False, marker_r=0.0)
    got, _, _ = run_host(host_program, tmp_path, "still", 60, 60, view, plain, [still])
    want = np.full((60, 60), plain.outside, dtype=np.uint32)
    want[5:55, 5:55] = plain.palette[0]      # pixel centres at -4.5 .. 54.5: columns and rows 5..54 lie inside [0, 50]
    assert np.array_equal(got[0], want)
    a, _, _ = run_host(host_program, tmp_path, "still12", 60, 60, view, cmp_style(True, 12, marker_r=0.0), [still])
    b, _, _ = run_host(host_program, tmp_path, "still0", 60, 60, view, cmp_style(True, 0, marker_r=0.0), [still])
    assert np.array_equal(a, b)      # no current: no streamline leaves its pixel
    # ... and with LIC on and no step, g is the pixel's own noise
    c, r = np.meshgrid(np.arange(60), np.arange(60), indexing="xy")
    g = twin_noise(c, r, 7)
    f = 96 + (255 - 96) * g // 255
    p0 = plain.palette[0]
    flat = ((p0 >> 16 & 255) * f // 255) << 16 | ((p0 >> 8 & 255) * f // 255) << 8 | ((p0 & 255) * f // 255)
    assert np.array_equal(b[0][5:55, 5:55], flat[5:55, 5:55].astype(np.uint32))


def test_pixel_centre_on_a_core_gets_the_top_level(host_program, tmp_path):
    # 10 x 10 pixels over [0, 10]^2: the centre of (row 6, column 3) is (3.5, 3.5)
    w = dict(cores=np.array([[3.5, 3.5, 20.0]]), obstacles=np.zeros((0, 3)), start=np.array([9.0, 9.0]), goal=np.array([9.0, 9.0]))
    style = cmp_style(False, marker_r=0.0)
    style.v_max = 1e6      # every other pixel is far below the top level
    got, _, _ = run_host(host_program, tmp_path, "core", 10, 10, (0.0, 0.0, 10.0, 10.0), style, [w])
    assert got[0][6, 3] == style.palette[-1]
    assert (got[0] == style.palette[-1]).sum() == 1 and (got[0] == style.palette[0]).sum() == 99


def test_view_outside_the_map_and_a_missing_world(host_program, tmp_path, worlds):
    style = cmp_style(True)
    got, _, _ = run_host(host_program, tmp_path, "out", 33, 17, (60.0, -30.0, 90.0, -1.0), style, [worlds[0], None])
    assert (got == style.outside).all()
    got, _, _ = run_host(host_program, tmp_path, "missing", 33, 17, WHOLE, style, [worlds[0], None])
    assert (got[1] == style.outside).all() and not (got[0] == style.outside).any()


# ---- primitives -------------------------------------------------------------------------------------------------------------------------------------
PRIM_W, PRIM_H, PRIM_VIEW, PRIM_IMAGES = 80, 48, (0.0, 0.0, 40.0, 24.0), 3      # half a world unit per pixel


def prim_cases():
    """name -> record array (render.PRIM_DTYPE): the cases of the issue, shared with the GPU test."""
    from distributional_rl_navigation_amd import render
    nan = float("nan")

    def rec(rows):
        a = np.zeros(len(rows), dtype=render.PRIM_DTYPE)
        for i, row in enumerate(rows):
            a[i] = row
        return a
    red, green, blue = render.word(0xFF0000, 4), render.word(0x00FF00, 4), render.word(0x0000FF, 5)
    return {
        "horizontal": rec([(3.2, 10.1, 30.7, 10.1, 0, 0, red, 0, 0)]),
        "vertical": rec([(17.3, 2.0, 17.3, 21.9, 0, 0, red, 0, 1)]),
        "diagonal": rec([(1.0, 1.0, 38.5, 22.25, 1, 1, red, 0, 0), (38.0, 2.0, 3.0, 23.0, 1, 2, green, 0, 2)]),
        "subpixel": rec([(20.1, 12.1, 20.3, 12.2, 0, 0, red, 0, 0), (5.0, 5.0, 5.0, 5.0, 0, 0, green, 0, 1)]),
        "crossing_other_z": rec([(2.0, 2.0, 38.0, 22.0, 0, 0, red, 0, 1), (2.0, 22.0, 38.0, 2.0, 0, 0, blue, 0, 1)]),
        "crossing_same_z": rec([(2.0, 2.0, 38.0, 22.0, 0, 0, red, 0, 1), (2.0, 22.0, 38.0, 2.0, 0, 0, green, 0, 1)]),
        "nan": rec([(nan, 2.0, 38.0, 22.0, 0, 2, red, 0, 1), (2.0, 2.0, 38.0, nan, 0, 2, red, 0, 1), (2.0, nan, 10.0, 4.0, 0, 2, red, 0, 0),
                    (4.0, 4.0, float("inf"), 4.0, 0, 2, red, 0, 0), (nan, 5.0, 1.0, 0.0, 0, 2, red, 1, 0), (5.0, 5.0, nan, 2.0, 0, 2, red, 2, 0)]),
        "huge": rec([(-1e300, 12.0, 1e300, 12.0, 0, 0, red, 0, 1), (20.0, -1e300, 20.0, 1e300, 1, 1, green, 0, 0), (-1e300, -1e300, 1e300, 1e300, 2, 2, blue, 0, 0),
                     (1e300, 1.0, 1e300, 20.0, 0, 2, red, 0, 3), (-1e308, 3.0, 1e308, 3.0, 0, 2, red, 0, 0)]),
        "outside": rec([(-30.0, -5.0, -2.0, 30.0, 0, 2, red, 0, 2), (41.5, 0.0, 60.0, 24.0, 0, 2, red, 0, 0), (0.0, 26.0, 40.0, 25.5, 0, 2, red, 0, 1),
                        (100.0, 100.0, 3.0, 0, 0, 2, green, 1, 0), (-50.0, 12.0, 5.0, 9.0, 0, 2, green, 2, 0)]),
        "image_ranges": rec([(2.0, 3.0, 30.0, 3.0, 2, 1, red, 0, 0), (2.0, 6.0, 30.0, 6.0, -5, 1, green, 0, 0), (2.0, 9.0, 30.0, 9.0, 1, 99, blue, 0, 0),
                             (2.0, 12.0, 30.0, 12.0, 3, 7, red, 0, 0), (2.0, 15.0, 30.0, 15.0, -9, -1, red, 0, 0), (10.0, 18.0, 2.0, 0.0, -1, 5, green, 1, 0)]),
        "disc_and_ring_on_the_edge": rec([(1.0, 23.0, 4.3, 0.0, 0, 0, red, 1, 0), (39.0, 12.0, 2.2, 5.1, 0, 1, green, 2, 0), (20.0, 12.0, 0.0, 0.0, 1, 1, blue, 1, 0),
                                          (20.0, 5.0, 1e300, 0.0, 2, 2, blue, 1, 0), (8.0, 8.0, 3.0, 2.0, 2, 2, red, 2, 0), (8.0, 8.0, -1.0, 0.0, 2, 2, red, 1, 0)]),
        "unknown_kind": rec([(2.0, 2.0, 38.0, 22.0, 0, 2, red, 3, 1), (2.0, 2.0, 38.0, 22.0, 0, 2, red, 65535, 1)]),
        "wide": rec([(3.0, 3.0, 37.0, 20.0, 0, 0, red, 0, 8), (3.0, 20.0, 37.0, 3.0, 1, 1, red, 0, 65535), (39.9, 23.9, 39.9, 23.9, 2, 2, green, 0, 4)]),
    }


CASE_NAMES = ("horizontal", "vertical", "diagonal", "subpixel", "crossing_other_z", "crossing_same_z", "nan", "huge", "outside", "image_ranges",
              "disc_and_ring_on_the_edge", "unknown_kind", "wide")
FILL = 0x01334455      # a background at z = 1, below every primitive of the cases


@pytest.mark.parametrize("name", CASE_NAMES)
def test_primitives_equal_the_twin(host_program, tmp_path, name):
    prims = prim_cases()[name]
    got, items, most = run_host(host_program, tmp_path, name, PRIM_W, PRIM_H, PRIM_VIEW, n_images=PRIM_IMAGES, prims=prims, fill=FILL)
    want = np.full((PRIM_IMAGES, PRIM_H, PRIM_W), FILL, dtype=np.uint32)
    samples = twin_draw(want, PRIM_VIEW, prims)
    drawn = got != FILL
    print(f"[{name}] {int(drawn.sum())} pixels drawn, {items} work items, at most {most} per primitive and image; twin: at most {samples} samples")
    assert np.array_equal(got, want), np.argwhere(got != want)[:5]
    # the sample count of a segment is bounded by the image, whatever its coordinates: max(W, H) + 2 (half_width + 1) + 1; a box by the image
    assert most <= max(PRIM_W * PRIM_H, max(PRIM_W, PRIM_H) + 2 * 9 + 1)
    if name in ("nan", "outside", "unknown_kind"):
        assert not drawn.any()
    if name == "huge":
        assert samples <= max(PRIM_W, PRIM_H) + 2 * 2 + 1
        assert drawn[0].any() and drawn[1].any() and drawn[2].any()
        assert not drawn[0][:, :][np.abs(np.arange(PRIM_H) - 23) > 2].any()      # y = 12 is row 23 / 24: nothing away from the line's rows
    if name == "image_ranges":      # y = 3, 6, 9, 12, 15 are rows 42, 36, 30, 24, 18; the disc covers rows 8 .. 16
        rows = lambda r: [bool(drawn[i, r].any()) for i in range(PRIM_IMAGES)]
        assert rows(42) == [False] * 3 and rows(36) == [True, True, False] and rows(30) == [False, True, True]      # [2, 1] is empty; [-5, 1]; [1, 99]
        assert rows(24) == [False] * 3 and rows(18) == [False] * 3 and rows(12) == [True] * 3      # [3, 7] and [-9, -1] miss every image; [-1, 5] has all
    if name.startswith("crossing"):
        a, b = (np.full((1, PRIM_H, PRIM_W), FILL, dtype=np.uint32) for _ in range(2))
        twin_draw(a, PRIM_VIEW, prims[:1]); twin_draw(b, PRIM_VIEW, prims[1:])
        assert np.array_equal(got[0], np.maximum(a[0], b[0])) and ((a[0] != FILL) & (b[0] != FILL)).any()      # the per-pixel max word either way


def test_draw_order_does_not_matter_on_the_host(host_program, tmp_path):
    cases = prim_cases()
    prims = np.concatenate([cases[k] for k in ("diagonal", "crossing_same_z", "crossing_other_z", "disc_and_ring_on_the_edge", "wide")])
    a, _, _ = run_host(host_program, tmp_path, "fwd", PRIM_W, PRIM_H, PRIM_VIEW, n_images=PRIM_IMAGES, prims=prims, fill=FILL)
    b, _, _ = run_host(host_program, tmp_path, "rev", PRIM_W, PRIM_H, PRIM_VIEW, n_images=PRIM_IMAGES, prims=prims[::-1].copy(), fill=FILL)
    assert np.array_equal(a, b)


# ---- PNG and sheets ---------------------------------------------------------------------------------------------------------------------------------
def decode_png(data):
    """An 8-bit RGB, filter-0 PNG by hand: (H, W, 3) uint8."""
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    at, chunks = 8, []
    while at < len(data):
        n, tag = struct.unpack(">I4s", data[at:at + 8])
        body = data[at + 8:at + 8 + n]
        assert struct.unpack(">I", data[at + 8 + n:at + 12 + n])[0] == zlib.crc32(tag + body) & 0xFFFFFFFF
        chunks.append((tag, body))
        at += 12 + n
    assert [t for t, _ in chunks][0] == b"IHDR" and chunks[-1] == (b"IEND", b"")
    w, h, depth, colour, comp, filt, lace = struct.unpack(">IIBBBBB", chunks[0][1])
    assert (depth, colour, comp, filt, lace) == (8, 2, 0, 0, 0)
    raw = np.frombuffer(zlib.decompress(b"".join(b for t, b in chunks if t == b"IDAT")), dtype=np.uint8).reshape(h, 1 + 3 * w)
    assert (raw[:, 0] == 0).all()
    return raw[:, 1:].reshape(h, w, 3)


def test_save_png_round_trip(tmp_path):
    from distributional_rl_navigation_amd import render
    rng = np.random.RandomState(5)
    for shape in ((1, 1, 3), (7, 13, 3), (45, 67, 3)):
        img = rng.randint(0, 256, size=shape).astype(np.uint8)
        path = str(tmp_path / "a.png")
        render.save_png(path, torch.from_numpy(img))
        assert np.array_equal(decode_png(open(path, "rb").read()), img)
    with pytest.raises(ValueError):
        render.save_png(str(tmp_path / "b.png"), np.zeros((4, 4), np.uint8))


def test_contact_sheet_shapes():
    from distributional_rl_navigation_amd import render
    rgb = torch.arange(5 * 4 * 6 * 3, dtype=torch.int64).reshape(5, 4, 6, 3).to(torch.uint8)
    s = render.contact_sheet(rgb, 3)
    assert s.shape == (8, 18, 3) and s.dtype == torch.uint8
    assert torch.equal(s[:4, 6:12], rgb[1]) and torch.equal(s[4:, :6], rgb[3]) and torch.equal(s[4:, 6:12], rgb[4]) and (s[4:, 12:] == 0).all()
    s = render.contact_sheet(rgb, 2, gap=1, fill=9)
    assert s.shape == (3 * 4 + 2, 2 * 6 + 1, 3) and torch.equal(s[5:9, 7:13], rgb[3]) and (s[4] == 9).all() and (s[:, 6] == 9).all()
    assert render.contact_sheet(rgb[:1], 4).shape == (4, 24, 3)


# ---- the builders' bookkeeping, with stand-ins for the device calls -------------------------------------------------------------------------------
class FakeCanvas:
    """What episode_sheet / episode_frames ask of a canvas, recording instead of drawing."""

    def __init__(self, n_images, log=None):
        self.n_images, self.view, self.log = n_images, WHOLE, [] if log is None else log
        self.pixels = torch.zeros(n_images, 1, 1)

    def repeat(self, n):
        return FakeCanvas(int(n), self.log)

    def draw(self, prims):
        self.log.append((self.n_images, prims))
        return self


def test_builders_pack_records():
    from distributional_rl_navigation_amd import render
    p = render.prims_to_numpy(torch.cat((
        render.segments([[0, 1], [2, 3]], [[4, 5], [6, float("nan")]], render.word(0xFF0000, 200), [0, 1], [5, 6], 2),
        render.polylines(torch.tensor([[[0.0, 0.0], [1.0, 0.0], [1.0, 1.0]], [[5.0, 5.0], [float("nan"), 0.0], [7.0, 7.0]]]), render.word(0x123456, 1), 3),
        render.discs([[1.5, 2.5]], 0.75, 7, 2, 4), render.rings([[1.5, 2.5], [0.0, 0.0]], 0.5, [1.5, 2.5], 8))))
    assert len(p) == 2 + 4 + 1 + 2
    assert p["kind"].tolist() == [0] * 6 + [1] + [2, 2] and p["half_width_px"].tolist() == [2, 2] + [0] * 7
    assert p["color_z"][0] == 0xC8FF0000 and p["color_z"][2] == 0x01123456
    assert p["image_first"].tolist() == [0, 1, 3, 3, 3, 3, 2, 0, 0] and p["image_last"].tolist() == [5, 6, 3, 3, 3, 3, 4, 0, 0]
    assert p[2].tolist()[:4] == (0.0, 0.0, 1.0, 0.0) and p[3].tolist()[:4] == (1.0, 0.0, 1.0, 1.0) and np.isnan(p["x1"][4]) and np.isnan(p["x0"][5])
    assert p[6].tolist()[:4] == (1.5, 2.5, 0.75, 0.0) and p[8].tolist()[:4] == (0.0, 0.0, 0.5, 2.5)


def test_episode_sheet_cuts_at_steps():
    from distributional_rl_navigation_amd import render
    T, n, N = 5, 3, 2
    traj = torch.arange(T * n * N * 2, dtype=torch.float64).reshape(T, n, N, 2)
    steps = torch.tensor([5, 2, 0])
    canvas = FakeCanvas(n)
    assert render.episode_sheet(None, traj, steps, color=0x00FF00, canvas=canvas, half_width=1) is canvas
    (images, prims), = canvas.log
    p = render.prims_to_numpy(prims)
    assert images == n and len(p) == n * (T * N - 1) and (p["kind"] == 0).all() and (p["color_z"] == render.word(0x00FF00, render.Z_TRAIL)).all()
    for e in range(n):
        mine = p[p["image_first"] == e]
        assert (mine["image_last"] == e).all() and len(mine) == T * N - 1
        whole = np.isfinite(mine["x0"]) & np.isfinite(mine["x1"])
        assert whole.sum() == max(int(steps[e]) * N - 1, 0)      # the points of steps 0 .. steps[e] - 1, joined; everything behind is NaN
        pts = traj[:, e].reshape(T * N, 2).numpy()
        assert np.array_equal(np.stack([mine["x0"], mine["y0"]], 1)[whole], pts[:-1][whole]) and np.array_equal(np.stack([mine["x1"], mine["y1"]], 1)[whole], pts[1:][whole])
    with pytest.raises(ValueError):
        render.episode_sheet(None, traj, steps, canvas=FakeCanvas(n + 1))


@pytest.mark.parametrize("every", (1, 3))
def test_episode_frames_ranges(every):
    from distributional_rl_navigation_amd import render
    T, N = 7, 2
    rng = np.random.RandomState(1)
    states = torch.from_numpy(rng.uniform(1.0, 9.0, size=(T, 1, 6)))
    traj = torch.from_numpy(rng.uniform(1.0, 9.0, size=(T, 1, N, 2)))
    seen = []

    def observe(st):
        seen.append(st.clone())
        obs = torch.zeros(st.shape[0], 26, dtype=torch.float64)
        obs[:, 4] = 1.0      # beam 0 hits one unit ahead; the others miss
        return obs
    back = FakeCanvas(1)
    out = render.episode_frames(None, 0, states, traj, beams=True, every=every, start=(0.5, 0.25), background=back, observe=observe, robot_r=0.5, half_width=2)
    F = (T + every - 1) // every
    (images, prims), = back.log
    assert images == F and out.n_images == F
    shown = [min(f * every, T - 1) for f in range(F)]
    assert len(seen) == 1 and torch.equal(seen[0], states[shown, 0])
    p = render.prims_to_numpy(prims)
    trail = p[(p["kind"] == 0) & (p["color_z"] >> 24 == render.Z_TRAIL)]
    assert len(trail) == T * N and (trail["image_last"] == F - 1).all() and (trail["half_width_px"] == 2).all()
    pts = np.concatenate([[[0.5, 0.25]], traj[:, 0].reshape(T * N, 2).numpy()])
    for j, seg in enumerate(trail):
        t = j // N
        assert seg["image_first"] == -(-t // every)      # the first frame f with f * every >= t
        assert (seg["x0"], seg["y0"], seg["x1"], seg["y1"]) == (pts[j, 0], pts[j, 1], pts[j + 1, 0], pts[j + 1, 1])
    # frame f holds exactly the trail segments of steps t <= f * every
    for f in range(F):
        inside = (trail["image_first"] <= f) & (trail["image_last"] >= f)
        assert inside.sum() == min(f * every + 1, T) * N
    robot = p[p["kind"] == 1]
    assert len(robot) == F and robot["image_first"].tolist() == list(range(F)) == robot["image_last"].tolist() and (robot["x1"] == 0.5).all()
    assert np.array_equal(np.stack([robot["x0"], robot["y0"]], 1), states[shown, 0, :2].numpy())
    top = p[(p["kind"] == 0) & (p["color_z"] >> 24 == render.Z_ROBOT)]
    beams = p[(p["kind"] == 0) & (p["color_z"] >> 24 == render.Z_BEAM)]
    assert len(top) == F and len(beams) == 11 * F and top["image_first"].tolist() == list(range(F)) == top["image_last"].tolist()
    st = states[shown, 0].numpy()
    assert np.allclose(top["x1"], st[:, 0] + np.cos(st[:, 2]), atol=1e-12) and np.allclose(top["y1"], st[:, 1] + np.sin(st[:, 2]), atol=1e-12)
    b = beams.reshape(F, 11)
    assert np.isnan(b["x1"][:, 1:]).all() and (b["image_first"] == np.arange(F)[:, None]).all() and (b["image_last"] == b["image_first"]).all()
    assert np.allclose(b["x1"][:, 0], st[:, 0] + np.cos(st[:, 2]), atol=1e-12) and np.allclose(b["y1"][:, 0], st[:, 1] + np.sin(st[:, 2]), atol=1e-12)
    assert np.array_equal(b["x0"][:, 0], st[:, 0])
    # no beams asked: no observation call, no beam records
    back2, seen[:] = FakeCanvas(1), []
    render.episode_frames(None, 0, states, traj, beams=False, every=every, background=back2, observe=observe, steps=4)
    p2 = render.prims_to_numpy(back2.log[0][1])
    assert not seen and not (p2["color_z"] >> 24 == render.Z_BEAM).any() and back2.log[0][0] == (4 + every - 1) // every
    assert np.isnan(p2["x0"][0]) and ((p2["kind"] == 0) & (p2["color_z"] >> 24 == render.Z_TRAIL)).sum() == 4 * N      # no start given: segment 0 is a break
