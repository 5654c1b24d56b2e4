"""Pictures of worlds and episodes, made where the data is: flow images (speed levels, optionally line integral convolution for the direction),
obstacles and start / goal markers by `mn_render_worlds`, trails, robots and sonar beams by `mn_render_draw` (include/marinenav_hip.h states the
raster rules; csrc/mn_render.hip holds the kernels).  A trajectory trace of an episode launch, `[T][n][N][2]` on the device, becomes a sheet of
one image per world (`episode_sheet`: the reference's `draw_trajectory` figure) or the frames of a video (`episode_frames`: the map of
`draw_video_plots`; render_panels.py draws its side panels and the whole frame from the plot primitives here: `rects`, `markers`, `sectors`,
`arrows`, `text`, `numbers`, `choose_text`) without leaving the device; only finished RGB images are copied to the host, by `save_png` (zlib and struct, no
plotting library).

A pixel is a uint32 word `z << 24 | r << 16 | g << 8 | b`; the larger word wins wherever two things meet, so the draw order `z` decides first and
the result never depends on the order in which primitives are drawn.  Colours here are ints `0xRRGGBB`; `word(rgb, z)` makes the pixel word."""
import ctypes as C
import dataclasses
import struct
import zlib

import numpy as np
import torch

from . import _capi

Z_FIELD, Z_OBSTACLE, Z_MARKER, Z_BEAM, Z_TRAIL, Z_ROBOT = 0, 1, 2, 3, 4, 5
PRIM_BYTES = 48
PRIM_DTYPE = np.dtype([("x0", "<f8"), ("y0", "<f8"), ("x1", "<f8"), ("y1", "<f8"), ("image_first", "<i4"), ("image_last", "<i4"), ("color_z", "<u4"),
                       ("kind", "<u2"), ("half_width_px", "<u2")])      # mn_render_prim, for reading a primitive buffer on the host
assert PRIM_DTYPE.itemsize == PRIM_BYTES == C.sizeof(_capi.MnRenderPrim)


def word(rgb, z=0):
    """The pixel word of colour `rgb` (0xRRGGBB) at draw order `z` (0..255)."""
    return (int(z) & 255) << 24 | (int(rgb) & 0xFFFFFF)


def blue_ramp(n_levels=16):
    """The default palette: level 0 (still water) light, the top level dark blue; integers by formula."""
    n = int(n_levels)
    d = max(n - 1, 1)
    return [(232 - 224 * i // d) << 16 | (241 - 193 * i // d) << 8 | (250 - 143 * i // d) for i in range(n)]


@dataclasses.dataclass
class Style:
    """How a world is coloured (mn_render_style).  `v_max`: the speed of the top level -- on the 30 worlds of the evaluation config the 99th
    percentile of the speed is 3.3-4.0 and the maximum below 10.  `lic`: line integral convolution over `lic_steps` Euler steps of `hpx` pixels each
    way; noise 0 darkens a colour to `lic_floor` / 255.  `marker_r` <= 0 leaves start and goal out."""
    v_max: float = 4.0
    palette: list = dataclasses.field(default_factory=blue_ramp)
    lic: bool = True
    lic_steps: int = 12
    hpx: float = 1.0
    lic_floor: int = 96
    seed: int = 0
    outside: int = 0x808080
    obstacle: int = 0xC0188C
    marker: int = 0xF2D21B
    marker_r: float = 0.6
    max_workgroups: int = 0

    def to_c(self):
        n = len(self.palette)
        if not 1 <= n <= _capi.RENDER_MAX_LEVELS:
            raise ValueError(f"a palette has 1 to {_capi.RENDER_MAX_LEVELS} levels, got {n}")
        s = _capi.MnRenderStyle(v_max=float(self.v_max), hpx=float(self.hpx), marker_r=float(self.marker_r), n_levels=n, lic=int(bool(self.lic)),
                                lic_steps=int(self.lic_steps), lic_floor=int(self.lic_floor), seed=int(self.seed) & 0xFFFFFFFF,
                                outside=int(self.outside) & 0xFFFFFF, obstacle=int(self.obstacle) & 0xFFFFFF, marker=int(self.marker) & 0xFFFFFF,
                                max_workgroups=int(self.max_workgroups), reserved=0)
        for i, c in enumerate(self.palette):
            s.palette[i] = int(c) & 0xFFFFFF
        return s


def _view4(view):
    return (C.c_double * 4)(*[float(a) for a in view])


def _ptr(t):
    return C.c_void_p(t.data_ptr())


class Canvas:
    """`pixels`: the packed [I][H][W] uint32 images on the device, `view` = (x0, y0, x1, y1) in world units.  `draw(prims)` draws a primitive buffer
    (`segments`, `polylines`, `discs`, `rings`, `rects`, `markers`, `sectors`, `arrows`, `text`, `numbers`; `torch.cat` joins buffers) into them in ONE launch and returns the canvas; `rgb()` drops the z byte."""

    def __init__(self, pixels, view):
        assert pixels.dim() == 3 and pixels.dtype == torch.uint32 and pixels.is_contiguous()
        self.pixels = pixels
        self.view = tuple(float(a) for a in view)

    n_images = property(lambda self: int(self.pixels.shape[0]))
    height = property(lambda self: int(self.pixels.shape[1]))
    width = property(lambda self: int(self.pixels.shape[2]))

    def draw(self, prims):
        prims = prims.contiguous()
        assert prims.dtype == torch.uint8 and prims.dim() == 2 and prims.shape[1] == PRIM_BYTES and prims.device == self.pixels.device
        rc = _capi.lib().mn_render_draw(_ptr(self.pixels), self.n_images, self.width, self.height, _view4(self.view), _ptr(prims), int(prims.shape[0]),
                                        _capi.stream_ptr(self.pixels.device))
        _capi.check(rc)
        return self

    def repeat(self, n):
        """A canvas of `n` copies of this canvas's FIRST image (a background rendered once, one copy per frame)."""
        return Canvas(self.pixels[:1].expand(int(n), -1, -1).contiguous(), self.view)

    def clone(self):
        return Canvas(self.pixels.clone(), self.view)

    def rgb(self):
        """uint8 [I][H][W][3] on the device."""
        p = self.pixels.view(torch.int32)
        return torch.stack(((p >> 16) & 255, (p >> 8) & 255, p & 255), dim=-1).to(torch.uint8)

    def z(self):
        """uint8 [I][H][W]: what lies on top at every pixel."""
        return ((self.pixels.view(torch.int32) >> 24) & 255).to(torch.uint8)


def whole_map(env):
    return (0.0, 0.0, float(env.params.width), float(env.params.height))


def image_height(width, view):
    """The height that keeps the aspect of `view` at `width` pixels."""
    return max(1, int(round(int(width) * (view[3] - view[1]) / (view[2] - view[0]))))


def world_images(env, envs=0, width=512, height=None, view=None, style=None):
    """Flow images of worlds `env` holds, in ONE launch (C-ABI mn_render_worlds): `envs` is one world index -- one image -- or an int tensor / array
    [I] -- image i shows world envs[i]; an index that is no world gives an image of `style.outside`.  `view=None` is the whole map, `height=None`
    keeps the view's aspect.  float64 on the master tables whatever the env's precision; nothing in the env changes.  Returns a Canvas."""
    view = whole_map(env) if view is None else tuple(float(a) for a in view)
    width = int(width)
    height = image_height(width, view) if height is None else int(height)
    style = Style() if style is None else style
    if isinstance(envs, (int, np.integer)):
        idx, env0, n = None, int(envs), 1
    else:
        idx = torch.as_tensor(envs).to(device=env.device, dtype=torch.int32).reshape(-1).contiguous()
        env0, n = 0, int(idx.shape[0])
    if n < 1 or width < 1 or height < 1 or n * width * height >= 1 << 31:
        raise ValueError(f"{n} images of {width} x {height}: every count must be at least 1 and their product below 2^31")
    px = torch.empty(n, height, width, dtype=torch.uint32, device=env.device)
    cs = style.to_c()
    env._check(env.L.mn_render_worlds(env.h, _ptr(idx) if idx is not None else None, env0, n, width, height, _view4(view), C.byref(cs), _ptr(px),
                                      env._stream()))
    return Canvas(px, view)


# ---- primitive builders: torch ops on whatever device the coordinates live on ---------------------------------------------------------------------
def _per_prim(v, n, dtype, device):
    t = torch.as_tensor(v, device=device).to(dtype).reshape(-1)
    if t.numel() == 1:
        t = t.expand(n)
    if t.numel() != n:
        raise ValueError(f"{t.numel()} values for {n} primitives")
    return t


def pack_prims(coords, kind, color_z, image_first=0, image_last=None, half_width=0):
    """[P][48] uint8: the records of mn_render_prim for `coords` [P][4] float64 (x0, y0, x1, y1 as `kind` reads them).  color_z (see `word`),
    image_first, image_last (default: image_first) and half_width are one value for all or one per primitive."""
    xy = torch.as_tensor(coords)
    xy = xy.to(torch.float64).reshape(-1, 4).contiguous()
    n, dev = xy.shape[0], xy.device
    first = _per_prim(image_first, n, torch.int32, dev)
    last = first if image_last is None else _per_prim(image_last, n, torch.int32, dev)
    cz = _per_prim(color_z, n, torch.int64, dev)
    cz = torch.where(cz >= 1 << 31, cz - (1 << 32), cz).to(torch.int32)      # the uint32 word in an int32's bits
    hw = _per_prim(half_width, n, torch.int32, dev).clamp(0, 0x7FFF)      # (the kernel counts anything above 8 as 8)
    tail = torch.stack((first, last, cz, hw << 16 | int(kind)), dim=1).contiguous()      # little endian: kind is the low half
    return torch.cat((xy.view(torch.uint8).reshape(n, 32), tail.view(torch.uint8).reshape(n, 16)), dim=1)


def segments(a, b, color_z, image_first=0, image_last=None, half_width=0):
    """Line segments from `a` [P][2] to `b` [P][2], world units; a NaN coordinate skips the segment."""
    a, b = torch.as_tensor(a).to(torch.float64).reshape(-1, 2), torch.as_tensor(b).to(torch.float64).reshape(-1, 2)
    return pack_prims(torch.cat((a, b.to(a.device)), dim=1), _capi.RENDER_SEGMENT, color_z, image_first, image_last, half_width)


def polylines(points, color_z, image_first=0, image_last=None, half_width=0):
    """`points` [..., M][2]: every leading index is one polyline of M points; a NaN row breaks the line.  Per-primitive values are [..., M - 1]."""
    p = torch.as_tensor(points).to(torch.float64)
    return segments(p[..., :-1, :].reshape(-1, 2), p[..., 1:, :].reshape(-1, 2), color_z, image_first, image_last, half_width)


def discs(centres, radius, color_z, image_first=0, image_last=None):
    c = torch.as_tensor(centres).to(torch.float64).reshape(-1, 2)
    r = _per_prim(radius, c.shape[0], torch.float64, c.device)
    return pack_prims(torch.stack((c[:, 0], c[:, 1], r, torch.zeros_like(r)), dim=1), _capi.RENDER_DISC, color_z, image_first, image_last)


def rings(centres, r_in, r_out, color_z, image_first=0, image_last=None):
    c = torch.as_tensor(centres).to(torch.float64).reshape(-1, 2)
    ri, ro = _per_prim(r_in, c.shape[0], torch.float64, c.device), _per_prim(r_out, c.shape[0], torch.float64, c.device)
    return pack_prims(torch.stack((c[:, 0], c[:, 1], ri, ro), dim=1), _capi.RENDER_RING, color_z, image_first, image_last)


# ---- the kinds a plot needs: rectangles, pixel-sized marks, sectors, arrows, text --------------------------------------------------------------------
MARKER_SHAPES = {"square": _capi.RENDER_MARKER_SQUARE, "plus": _capi.RENDER_MARKER_PLUS, "cross": _capi.RENDER_MARKER_CROSS}
GLYPH_ADVANCE, GLYPH_LINE = 6, 9      # pixels per character and per line at scale 1 (the cell is 5 x 7)
NUMBERS_MAX_DECIMALS = 3              # |v| < 1e15 times 10^3 stays an exact int64


def _pack16(coords, kind, color_z, image_first, image_last, param):
    """pack_prims with the record's 16-bit parameter as it is (0..65535): GLYPH's code | scale << 8, SECTOR's quantised cosine."""
    xy = torch.as_tensor(coords).to(torch.float64).reshape(-1, 4).contiguous()
    n, dev = xy.shape[0], xy.device
    first = _per_prim(image_first, n, torch.int32, dev)
    last = first if image_last is None else _per_prim(image_last, n, torch.int32, dev)
    cz = _per_prim(color_z, n, torch.int64, dev)
    cz = torch.where(cz >= 1 << 31, cz - (1 << 32), cz).to(torch.int32)
    w = _per_prim(param, n, torch.int64, dev).clamp(0, 0xFFFF) << 16 | int(kind)
    w = torch.where(w >= 1 << 31, w - (1 << 32), w).to(torch.int32)
    tail = torch.stack((first, last, cz, w), dim=1).contiguous()
    return torch.cat((xy.view(torch.uint8).reshape(n, 32), tail.view(torch.uint8).reshape(n, 16)), dim=1)


def rects(a, b, color_z, image_first=0, image_last=None):
    """Filled axis-aligned rectangles with corners `a` [P][2] and `b` [P][2] (any order), world units: every pixel whose centre lies inside, the
    edges included.  A NaN coordinate skips the rectangle."""
    a, b = torch.as_tensor(a).to(torch.float64).reshape(-1, 2), torch.as_tensor(b).to(torch.float64).reshape(-1, 2)
    return pack_prims(torch.cat((a, b.to(a.device)), dim=1), _capi.RENDER_RECT, color_z, image_first, image_last)


def markers(points, shape, arm, stroke, color_z, image_first=0, image_last=None):
    """Pixel-sized marks at `points` [P][2]: `shape` "square", "plus" or "cross" (or 0, 1, 2; one for all or [P]), `arm` pixels each way from the
    anchor pixel (at most 8), `stroke` the half thickness of a plus's or a cross's bars in pixels.  The size does not follow the view."""
    p = torch.as_tensor(points).to(torch.float64).reshape(-1, 2)
    n, dev = p.shape[0], p.device
    sh = MARKER_SHAPES[shape] if isinstance(shape, str) else shape
    return pack_prims(torch.stack((p[:, 0], p[:, 1], _per_prim(sh, n, torch.float64, dev), _per_prim(stroke, n, torch.float64, dev)), dim=1),
                      _capi.RENDER_MARKER, color_z, image_first, image_last, arm)


def sector_cosine(half_angle):
    """The 16-bit parameter of a SECTOR record for a half angle in radians (a host float): q with cos = q / 16384 - 1, quantised once."""
    import math
    return min(32768, max(0, int(round((math.cos(float(half_angle)) + 1.0) * 16384.0))))


def sectors(centres, mid_points, half_angle, color_z, image_first=0, image_last=None, device=None):
    """Wedges of discs: centre [P][2], `mid_points` [P][2] the point of the arc on the middle direction (so the radius is their distance), and the
    half angle in radians, one host float for all.  Built on the centres' device, or on `device`."""
    c, m = torch.as_tensor(centres, device=device).to(torch.float64).reshape(-1, 2), torch.as_tensor(mid_points).to(torch.float64).reshape(-1, 2)
    return _pack16(torch.cat((c, m.to(c.device)), dim=1), _capi.RENDER_SECTOR, color_z, image_first, image_last, sector_cosine(half_angle))


def arrows(a, b, head_px, color_z, view, size, image_first=0, image_last=None, half_width=0):
    """Arrows from `a` [P][2] to `b` [P][2]: the shaft and two head strokes of `head_px` pixels, 3 SEGMENT records each ([P][3] in this order).  The
    head is built in pixel units of `view` over `size` = (width, height), at atan(1 / 2) to the shaft; an arrow of no length has no head (its
    strokes are NaN)."""
    a, b = torch.as_tensor(a).to(torch.float64).reshape(-1, 2), torch.as_tensor(b).to(torch.float64).reshape(-1, 2)
    b = b.to(a.device)
    sx, sy = (float(view[2]) - float(view[0])) / int(size[0]), (float(view[3]) - float(view[1])) / int(size[1])
    du, dv = (b[:, 0] - a[:, 0]) / sx, -(b[:, 1] - a[:, 1]) / sy
    norm = torch.sqrt(du * du + dv * dv)
    uu, uv = du / norm, dv / norm      # (0 / 0 = NaN: no head)
    c, s = 2.0 / 5.0 ** 0.5, 1.0 / 5.0 ** 0.5
    tips = []
    for sign in (1.0, -1.0):
        pu, pv = -(c * uu) + sign * s * -uv, -(c * uv) + sign * s * uu
        tips.append(torch.stack((b[:, 0] + float(head_px) * pu * sx, b[:, 1] - float(head_px) * pv * sy), dim=1))
    n = a.shape[0]
    start = torch.stack((a, b, b), dim=1).reshape(3 * n, 2)
    end = torch.stack((b, tips[0], tips[1]), dim=1).reshape(3 * n, 2)
    def per_record(v, dtype):      # one value per arrow -> one per record
        return None if v is None else _per_prim(v, n, dtype, a.device)[:, None].expand(n, 3).reshape(-1)
    return segments(start, end, per_record(color_z, torch.int64), per_record(image_first, torch.int32), per_record(image_last, torch.int32), half_width)


def _align_shift(align, n_chars, scale):
    """Pixels from the anchor to the left edge of a line of `n_chars` characters."""
    width = max(GLYPH_ADVANCE * scale * n_chars - scale, 0)      # without the gap behind the last character
    if align == "left":
        return 0
    if align == "right":
        return -width
    if align == "centre" or align == "center":
        return -(width // 2)
    raise ValueError(f"align is 'left', 'right' or 'centre', got {align!r}")


def _glyphs(codes, anchor, cell_dx, cell_dy, color_z, scale, image_first, image_last):
    """GLYPH records of `codes` [P][L] (int tensor) at `anchor` [P][2] (or [2]): cell l of every row at pixel offset (cell_dx[l], cell_dy[l]) from the
    anchor's pixel, down positive.  Per-primitive values are one for all or [P]."""
    scale = int(scale)
    if not 1 <= scale <= 8:
        raise ValueError(f"a glyph's scale is 1..8, got {scale}")
    P, L = int(codes.shape[0]), int(codes.shape[1])
    dev = codes.device
    anchor = torch.as_tensor(anchor).to(device=dev, dtype=torch.float64).reshape(-1, 2)
    if anchor.shape[0] == 1:
        anchor = anchor.expand(P, 2)
    if anchor.shape[0] != P:
        raise ValueError(f"{anchor.shape[0]} anchors for {P} rows of text")
    off = torch.stack((torch.as_tensor(cell_dx, dtype=torch.float64, device=dev).reshape(L), torch.as_tensor(cell_dy, dtype=torch.float64, device=dev).reshape(L)), dim=1)
    coords = torch.cat((anchor[:, None, :].expand(P, L, 2), off[None].expand(P, L, 2)), dim=2).reshape(P * L, 4)

    def per_row(v, dtype):
        if v is None:
            return None
        return _per_prim(v, P, dtype, dev)[:, None].expand(P, L).reshape(-1)
    return _pack16(coords, _capi.RENDER_GLYPH, per_row(color_z, torch.int64), per_row(image_first, torch.int32), per_row(image_last, torch.int32),
                   (codes.to(torch.int64).clamp(0, 255) | scale << 8).reshape(-1))


def _text_cells(string, scale, align, dx, dy):
    """(codes [L], cell_dx [L], cell_dy [L]) of a string with "\\n": every character but the line breaks is one cell."""
    codes, xs, ys = [], [], []
    for k, line in enumerate(str(string).split("\n")):
        left = int(dx) + _align_shift(align, len(line), scale)
        for i, ch in enumerate(line):
            codes.append(ord(ch) if 32 <= ord(ch) <= 126 else ord("?"))
            xs.append(left + GLYPH_ADVANCE * scale * i)
            ys.append(int(dy) + GLYPH_LINE * scale * k)
    return codes, xs, ys


def text(string, anchor, color_z, scale=1, align="left", dx=0, dy=0, image_first=0, image_last=None, device=None):
    """`string` in the 5 x 7 font at `anchor` (world units; [2], or [P][2] for the same string at P anchors): one GLYPH record per character, the
    spaces included ([P][len]), each character `6 scale` pixels right of the one before, "\\n" `9 scale` pixels down.  (dx, dy) moves the text in
    pixels, dy down; the cell of the first line's first character has its top-left pixel at the anchor's pixel plus (dx, dy) for align "left";
    "right" ends every line there, "centre" centres it.  A character outside 32..126 becomes '?'.  An empty string gives 0 records.  The records
    are built on the anchor's device, or on `device` (a host anchor for a picture on the GPU)."""
    anchor = torch.as_tensor(anchor, device=device).to(torch.float64).reshape(-1, 2)
    codes, xs, ys = _text_cells(string, int(scale), align, dx, dy)
    P = anchor.shape[0]
    table = torch.tensor(codes, dtype=torch.int64, device=anchor.device).reshape(1, -1).expand(P, -1)
    return _glyphs(table, anchor, xs, ys, color_z, scale, image_first, image_last)


def number_codes(values, decimals, width, justify="right"):
    """[P][width] int64 character codes of `values` [P] in fixed notation on the device of `values`, the text at the right end of the cells or
    (`justify` "left") at their left end; see `numbers`."""
    if justify not in ("right", "left"):
        raise ValueError(f"justify is 'right' or 'left', got {justify!r}")
    d, width = int(decimals), int(width)
    if not 0 <= d <= NUMBERS_MAX_DECIMALS or width < 1:
        raise ValueError(f"numbers: decimals is 0..{NUMBERS_MAX_DECIMALS} and width at least 1, got {d} and {width}")
    v = torch.as_tensor(values).to(torch.float64).reshape(-1)
    dev = v.device
    bad = ~torch.isfinite(v) | (v.abs() >= 1e15)
    n = torch.floor(torch.where(bad, torch.zeros_like(v), v.abs()) * float(10 ** d) + 0.5).to(torch.int64)
    pow10 = torch.tensor([10 ** j for j in range(19)], dtype=torch.int64, device=dev)
    n_digits = (n[:, None] >= pow10[None, :]).sum(dim=1)                      # 0 for n = 0
    shown = torch.clamp(n_digits, min=d + 1)                                  # at least one digit before the point
    neg = (v < 0) & (n > 0)
    point = 1 if d > 0 else 0
    length = shown + point + neg.to(torch.int64)
    k = torch.arange(width - 1, -1, -1, device=dev, dtype=torch.int64)[None, :]      # cell -> its place counted from the right
    place = torch.where(k > d, k - point, k) if d > 0 else k                     # the decimal place of the digit in that cell
    digit = (n[:, None] // pow10[place.clamp(0, 18)]) % 10
    codes = torch.where(place < shown[:, None], 48 + digit, torch.full_like(digit, 32))
    if d > 0:
        codes = torch.where(k == d, torch.full_like(codes, 46), codes)
    codes = torch.where(neg[:, None] & (k == (shown + point)[:, None]), torch.full_like(codes, 45), codes)
    if justify == "left":      # cell i takes what stands (width - length) cells further right; the cells behind the text are spaces
        i = torch.arange(width, device=dev, dtype=torch.int64)[None, :]
        src = (i + (width - length)[:, None]).clamp(0, width - 1)
        codes = torch.where(i < length[:, None], torch.gather(codes, 1, src), torch.full_like(codes, 32))
    return torch.where((bad | (length > width))[:, None], torch.full_like(codes, 35), codes)


def numbers(values, decimals, width, anchor, color_z, scale=1, align="right", dx=0, dy=0, image_first=0, image_last=None, justify="right"):
    """`values` [P] (a device tensor, never read back) as text, value p at anchor p: exactly `width` GLYPH records per value ([P][width]), whatever
    the values.  n = floor(|v| 10^decimals + 0.5) as int64; its digits get a point before the last `decimals` digits and at least one digit before
    the point; '-' goes in front if v < 0 and n > 0; the text is right-justified in the `width` cells (`justify` "left": left-justified) and the unused cells hold a space.  A text
    longer than `width`, a non-finite v or |v| >= 1e15 fills every cell with '#'.  This is Python's f"{v:.{decimals}f}" except at ties, which that
    rounds to even on the exact decimal value and this rounds up on the float64 product, and except that a value that rounds to zero loses its
    sign.  `decimals` is 0..3.  The cells lie as a `text` of `width` characters does under `align`."""
    codes = number_codes(values, decimals, width, justify)
    _, xs, ys = _text_cells("0" * int(width), int(scale), align, dx, dy)
    return _glyphs(codes, anchor, xs, ys, color_z, scale, image_first, image_last)


def choose_text(strings, index, anchor, color_z, scale=1, align="left", dx=0, dy=0, image_first=0, image_last=None):
    """One of the host strings `strings` per anchor, chosen on the device: row index[p] (`index` [P], a device int tensor) of the code table goes at
    anchor p.  The strings are padded with spaces to the longest; every anchor gets that many GLYPH records.  An index outside the list writes
    spaces."""
    strings = [str(s) for s in strings]
    if not strings or any("\n" in s for s in strings):
        raise ValueError("choose_text takes a non-empty list of one-line strings")
    L = max(len(s) for s in strings)
    index = torch.as_tensor(index).reshape(-1)
    dev = index.device
    rows = [[ord(c) if 32 <= ord(c) <= 126 else ord("?") for c in s.ljust(L)] for s in strings] + [[32] * L]
    table = torch.tensor(rows, dtype=torch.int64, device=dev).reshape(len(rows), L)
    idx = index.to(torch.int64)
    idx = torch.where((idx >= 0) & (idx < len(strings)), idx, torch.full_like(idx, len(strings)))
    _, xs, ys = _text_cells("0" * L, int(scale), align, dx, dy)
    return _glyphs(table[idx], anchor, xs, ys, color_z, scale, image_first, image_last)


def font():
    """The 5 x 7 font as uint8 [95][7] (numpy): row byte j of code 32 + k, bit 4 the leftmost column (C-ABI mn_render_font)."""
    buf = (C.c_uint8 * (95 * 7))()
    _capi.check(_capi.lib().mn_render_font(C.cast(buf, C.c_void_p)))
    return np.frombuffer(bytes(buf), dtype=np.uint8).reshape(95, 7).copy()


def prims_to_numpy(prims):
    """A primitive buffer as a numpy record array (PRIM_DTYPE), on the host: for tests and for looking at what a builder made."""
    return np.frombuffer(prims.detach().cpu().contiguous().numpy().tobytes(), dtype=PRIM_DTYPE)


# ---- episodes -------------------------------------------------------------------------------------------------------------------------------------
def sheet_prims(traj, steps, color=0xE8590C, half_width=0, z=Z_TRAIL):
    """The trails of `episode_sheet`: env e's polyline over all sub-step positions of `traj` [T][n][N][2], into image e; the rows at or behind
    steps[e] are not drawn."""
    T, n, N = int(traj.shape[0]), int(traj.shape[1]), int(traj.shape[2])
    pts = traj.to(torch.float64).permute(1, 0, 2, 3)      # [n][T][N][2]
    alive = torch.arange(T, device=traj.device)[None, :] < torch.as_tensor(steps, device=traj.device).reshape(n, 1)
    pts = torch.where(alive[:, :, None, None], pts, torch.full_like(pts, float("nan"))).reshape(n, T * N, 2)
    image = torch.arange(n, device=traj.device, dtype=torch.int32)[:, None].expand(n, T * N - 1)
    return polylines(pts, word(color, z), image, None, half_width)


def episode_sheet(env, traj, steps, envs=None, color=0xE8590C, canvas=None, half_width=0, **world_kw):
    """Every env's whole trajectory of a trace `traj` [T][n][N][2] (an episode launch's, `set_trajectory_trace`) into that env's image: one image per
    world, ONE draw launch, the trace never leaves the device.  `steps` [n]: the steps env e ran (its rows t >= steps[e] are not drawn).  `canvas`:
    draw over it (the same worlds, another policy's trace, another colour: the reference's draw_trajectory figure); else `world_images` of
    `envs` (default: worlds 0 .. n - 1 of `env`) with `world_kw`.  Returns the canvas."""
    n = int(traj.shape[1])
    if canvas is None:
        canvas = world_images(env, torch.arange(n, dtype=torch.int32) if envs is None else envs, **world_kw)
    if canvas.n_images != n:
        raise ValueError(f"the canvas has {canvas.n_images} images for {n} envs")
    return canvas.draw(sheet_prims(traj, steps, color, half_width))


def frame_prims(states, traj, n_frames, every=1, start=None, robot_r=0.8, beams=None, trail_color=0xE8590C, robot_color=0x101010, beam_color=0x2F9E44,
                half_width=1):
    """The primitives of `episode_frames`, frame f showing the episode after step f * every: the trail segments of step t into frames
    [ceil(t / every), n_frames), the robot disc, its heading tick and the sonar beams of step f * every into frame f alone.  `states` [T][6],
    `traj` [T][N][2], `beams` None or [n_frames][11][2] in the robot frame ((0, 0): a miss), `start` None or the position before step 0."""
    T, N, dev = int(traj.shape[0]), int(traj.shape[1]), traj.device
    F, every = int(n_frames), int(every)
    pts = traj.to(torch.float64).reshape(T * N, 2)
    head = torch.full((1, 2), float("nan"), dtype=torch.float64, device=dev) if start is None else torch.as_tensor(start, dtype=torch.float64, device=dev).reshape(1, 2)
    pts = torch.cat((head, pts))      # segment j joins point j to point j + 1 = sub-step j % N of step j // N
    t_of = torch.arange(T * N, device=dev) // N
    first = ((t_of + every - 1) // every).to(torch.int32)
    parts = [polylines(pts, word(trail_color, Z_TRAIL), first, torch.full_like(first, F - 1), half_width)]
    frame = torch.arange(F, device=dev, dtype=torch.int32)
    st = states.to(torch.float64)[(frame.long() * every).clamp(max=T - 1)]
    x, y, c, s = st[:, 0], st[:, 1], torch.cos(st[:, 2]), torch.sin(st[:, 2])
    parts.append(discs(st[:, :2], robot_r, word(robot_color, Z_ROBOT), frame))
    tip = torch.stack((x + 2.0 * robot_r * c, y + 2.0 * robot_r * s), dim=1)
    parts.append(segments(st[:, :2], tip, word(robot_color, Z_ROBOT), frame, None, half_width))
    if beams is not None:
        b = torch.as_tensor(beams).to(device=dev, dtype=torch.float64).reshape(F, -1, 2)
        miss = (b[..., 0] == 0.0) & (b[..., 1] == 0.0)
        wx = x[:, None] + c[:, None] * b[..., 0] - s[:, None] * b[..., 1]      # out of the robot frame: p_world = R(theta) p + (x, y)
        wy = y[:, None] + s[:, None] * b[..., 0] + c[:, None] * b[..., 1]
        nan = torch.full_like(wx, float("nan"))
        hit = torch.stack((torch.where(miss, nan, wx), torch.where(miss, nan, wy)), dim=-1)
        parts.append(segments(st[:, None, :2].expand(-1, b.shape[1], -1), hit, word(beam_color, Z_BEAM), frame[:, None].expand(-1, b.shape[1])))
    return torch.cat(parts)


def episode_frames(env, env_index, states, traj, beams=True, every=1, steps=None, start=None, background=None, observe=None, width=512, height=None,
                   view=None, style=None, **prim_kw):
    """The frames of ONE episode in world `env_index`: `states` [T][6] (or [T][1][6]) and `traj` [T][N][2] (or [T][1][N][2]) as
    `rollout_at(..., trace=("state", "traj"))` returns them (`state_trace`, `traj_trace`) -- a stored action list becomes a video without a handle
    row -- or one env's column of an episode launch's traces.  `steps`: how many steps ran (default T).  Frame f shows the episode after step
    f * every.  The background is rendered once (`world_images`, or `background`: a one-image Canvas) and copied per frame; everything else is ONE
    draw launch.  The beams are `observation_at(states, dtype=float64)` of the frames' states (`observe` replaces that call), turned into the world
    frame with torch.  Returns a Canvas of F = ceil(steps / every) images."""
    states, traj = torch.as_tensor(states), torch.as_tensor(traj)
    if states.dim() == 3:
        states = states[:, 0]
    if traj.dim() == 4:
        traj = traj[:, 0]
    T = int(traj.shape[0]) if steps is None else min(int(steps), int(traj.shape[0]))
    if T < 1 or states.shape[0] < T:
        raise ValueError(f"{T} steps to draw from {tuple(states.shape)} states and {tuple(traj.shape)} positions")
    states, traj = states[:T], traj[:T]
    every = max(1, int(every))
    F = (T + every - 1) // every
    if background is None:
        background = world_images(env, int(env_index), width=width, height=height, view=view, style=style)
    if "robot_r" not in prim_kw and env is not None:
        prim_kw["robot_r"] = float(env.params.robot_r)
    obs = None
    if beams:
        shown = states[(torch.arange(F, device=states.device) * every).clamp(max=T - 1)]
        if observe is None:
            observe = lambda st: env.observation_at(st, env=int(env_index), velocity="given", dtype=torch.float64)
        obs = observe(shown)[:, 4:].reshape(F, -1, 2)
    return background.repeat(F).draw(frame_prims(states.to(background.pixels.device), traj.to(background.pixels.device), F, every, start, beams=obs,
                                                 **prim_kw))


# ---- leaving the device ---------------------------------------------------------------------------------------------------------------------------
def contact_sheet(rgb, cols, gap=0, fill=0):
    """[I][H][W][3] images as one [rows * H + (rows - 1) gap][cols * W + (cols - 1) gap][3] image, row by row; missing tiles and gaps are `fill`."""
    I, H, W, ch = rgb.shape
    cols = max(1, int(cols))
    rows = (I + cols - 1) // cols
    out = rgb.new_full((rows * H + (rows - 1) * gap, cols * W + (cols - 1) * gap, ch), fill)
    for i in range(I):
        r, c = divmod(i, cols)
        out[r * (H + gap):r * (H + gap) + H, c * (W + gap):c * (W + gap) + W] = rgb[i]
    return out


def png_bytes(rgb):
    """An 8-bit RGB PNG of `rgb` [H][W][3] uint8 (tensor or array): filter 0 on every row, one zlib stream."""
    a = rgb.detach().cpu().numpy() if torch.is_tensor(rgb) else np.asarray(rgb)
    if a.ndim != 3 or a.shape[2] != 3 or a.dtype != np.uint8:
        raise ValueError(f"save_png takes uint8 [H][W][3], got {a.dtype} {a.shape}")
    h, w = a.shape[:2]
    raw = np.concatenate((np.zeros((h, 1), np.uint8), a.reshape(h, w * 3)), axis=1).tobytes()

    def chunk(tag, data):
        return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)
    return b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 0)) + chunk(b"IDAT", zlib.compress(raw, 6)) + chunk(b"IEND", b"")


def save_png(path, rgb):
    with open(path, "wb") as f:
        f.write(png_bytes(rgb))
