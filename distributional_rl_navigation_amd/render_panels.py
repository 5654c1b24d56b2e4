"""The side panels of the reference's episode video (env_visualizer.draw_video_plots) and the whole frame, drawn where the data is: the return
distributions an IQN action was chosen from (`plot_return_dist`), the Q-values of a DQN action (`plot_action_qvalues`), the sonar reflections and the
measured velocity in the robot frame (`plot_measurements`), the goal and action text -- built from render.py's primitives (rects, markers, sectors,
arrows, text, numbers) as torch ops on the device of their inputs, drawn by ONE mn_render_draw launch per panel.  No value is read back.

A panel is a Canvas of F images whose view is its own pixel grid, (0, 0, width, height) with y up: a panel coordinate is a pixel coordinate.  What
the reference does per frame with set_xlim happens in the builder, on the device: x' = (x - lo_f) / (hi_f - lo_f) across the plot box, and the limit
labels are `numbers` of lo_f and hi_f.  Every `*_prims` function returns the primitive buffer of its panel (on the CPU too); `*_panel` draws it
into a blank canvas (or into `canvas`).  Text is the one 5 x 7 font: phi is spelled out, nothing is bold, nothing is anti-aliased."""
import torch

from . import render
from .render import word

Z_TINT, Z_AXIS, Z_LINE, Z_MARK, Z_BAR, Z_TOP, Z_TEXT = 1, 2, 3, 4, 5, 6, 7
WHITE, BLACK, RED, BLUE, GREEN, LINE_BLUE, WEDGE = 0xFFFFFF, 0x000000, 0xFF0000, 0x0000FF, 0x008000, 0x1F77B4, 0xFFCCCC      # (red at alpha 0.2 on white)
MEAN_BAR = 0.35      # the mean bar reaches this many rows up and down


def blank(n_images, width, height, device, color=WHITE):
    """A canvas of `n_images` images of one colour at z = 0 whose view is its pixel grid."""
    px = torch.full((int(n_images), int(height), int(width)), int(color) & 0xFFFFFF, dtype=torch.int32, device=device).view(torch.uint32)
    return render.Canvas(px, (0.0, 0.0, float(width), float(height)))


def text_scale(width, height=None):
    """The glyph scale of a panel: 1 up to 400 pixels of width, then one more per 400 (3 in a 1920-wide frame's panels)."""
    return max(1, min(8, int(width) // 400 + 1))


def _frames(F, device):
    return torch.arange(int(F), dtype=torch.int32, device=device)


def _limits(values, xlim, F):
    """(lo [F], hi [F]) float64: "frame": min - 5 and max + 5 of every frame's values; else the pair given (floats or [F] tensors)."""
    if isinstance(xlim, str):
        if xlim != "frame":
            raise ValueError(f"xlim is 'frame' or (lo, hi), got {xlim!r}")
        flat = values.reshape(F, -1)
        return flat.amin(dim=1) - 5.0, flat.amax(dim=1) + 5.0
    lo, hi = (render._per_prim(v, F, torch.float64, values.device) for v in xlim)
    return lo, hi


def shared_limits(blocks):
    """The reference's one xlim for all distribution panels of a frame: (min - 5, max + 5) over every block [F][...] of `blocks`, per frame."""
    F = int(blocks[0].shape[0])
    lo = torch.stack([b.to(torch.float64).reshape(F, -1).amin(dim=1) for b in blocks]).amin(dim=0) - 5.0
    hi = torch.stack([b.to(torch.float64).reshape(F, -1).amax(dim=1) for b in blocks]).amax(dim=0) + 5.0
    return lo, hi


def action_labels(params, compact=False):
    """The nine (a, w) label pairs of the action table of `params` (robot.compute_actions: a outer, w inner): ["a: -0.40", ...], ["w: -0.52", ...]."""
    table = [(float(a), float(w)) for a in params.a for w in params.w]
    if compact:
        return [f"{a:.1f},{w:.2f}" for a, w in table], None
    return [f"a: {a:.2f}" for a, _ in table], [f"w: {w:.2f}" for _, w in table]


def _title(parts, string, value, decimals, value_width, width, height, scale, F, device):
    """A centred title line at the top: `string`, followed by `value` [F] as a number where given."""
    n = len(string) + (value_width if value is not None else 0)
    left = (int(width) - (render.GLYPH_ADVANCE * scale * n - scale)) // 2
    anchor = (0.5, float(height) - 0.5)      # the top-left pixel of the panel
    parts.append(render.text(string, anchor, word(BLACK, Z_TEXT), scale, "left", left, 1, 0, F - 1, device))
    if value is not None:
        parts.append(render.numbers(value, decimals, value_width, anchor, word(BLACK, Z_TEXT), scale, "left", left + render.GLYPH_ADVANCE * scale * len(string), 1,
                                    _frames(F, device), justify="left"))


def _bars_prims(means, quantiles, lo, hi, title, title_value, width, height, labels, params):
    """What return_dist_prims and q_values_prims share: `means` [F][A] as bars on A rows, `quantiles` None or [F][K][A] as marks on them."""
    F, A = int(means.shape[0]), int(means.shape[1])
    dev = means.device
    W, H, s = int(width), int(height), text_scale(width)
    strip = render.GLYPH_LINE * s + 2
    compact = (H - 2 * strip) / (A + 1) < 2 * render.GLYPH_LINE      # two label lines of scale 1 do not fit a row: one short line
    la, lw = action_labels(params, compact) if labels and params is not None else (None, None)
    right = (render.GLYPH_ADVANCE * max(len(t) for t in la) + 4) if la else 2
    X0, X1, Y0, Y1 = 2.5, W - right - 0.5, float(strip), float(H - strip)
    span = torch.where(hi > lo, hi - lo, torch.ones_like(hi))      # (never zero: the frame's limits are 10 apart or more)
    to_x = lambda v: X0 + (v - lo.reshape((F,) + (1,) * (v.dim() - 1))) / span.reshape((F,) + (1,) * (v.dim() - 1)) * (X1 - X0)
    row_h = (Y1 - Y0) / (A + 1)      # ylim [-1, A]
    y = Y0 + (torch.arange(A, dtype=torch.float64, device=dev) + 1.0) * row_h      # [A]
    frame = _frames(F, dev)
    parts = []
    ends = torch.stack((torch.full_like(y, X0), y, torch.full_like(y, X1), y), dim=1)
    parts.append(render.segments(ends[:, :2], ends[:, 2:], word(BLACK, Z_AXIS), 0, F - 1))      # the baselines: A records for all frames
    yf = y[None, :].expand(F, A)
    if quantiles is not None:
        K = int(quantiles.shape[1])
        qx = to_x(quantiles)      # [F][K][A]
        arm = max(1, min(render._capi.RENDER_MAX_HALF_WIDTH, int(row_h * 0.3)))
        parts.append(render.markers(torch.stack((qx, y[None, None, :].expand(F, K, A)), dim=-1), "cross", arm, 0 if s == 1 else s - 1, word(GREEN, Z_MARK),
                                    frame[:, None, None].expand(F, K, A)))
        x_min, x_max = to_x(quantiles.amin(dim=1)), to_x(quantiles.amax(dim=1))      # [F][A]
        parts.append(render.segments(torch.stack((x_min, yf), dim=-1), torch.stack((x_max, yf), dim=-1), word(LINE_BLUE, Z_LINE), frame[:, None].expand(F, A), None,
                                     0 if s == 1 else 1))
    best = means.argmax(dim=1, keepdim=True) == torch.arange(A, device=dev)[None, :]      # [F][A]; a NaN row has no finite bar to draw anyway
    mx = to_x(means)
    half = torch.where(best, torch.full_like(mx, 1.5 * s), torch.full_like(mx, 1.0 * s))
    colour = torch.where(best, torch.full_like(mx, word(RED, Z_TOP)), torch.full_like(mx, word(BLUE, Z_BAR))).to(torch.int64)
    parts.append(render.rects(torch.stack((mx - half, yf - MEAN_BAR * row_h), dim=-1), torch.stack((mx + half, yf + MEAN_BAR * row_h), dim=-1), colour,
                              frame[:, None].expand(F, A)))
    _title(parts, title, title_value, 2, 4, W, H, s, F, dev)
    bottom = (0.5, Y0 - 0.5)      # the pixel row under the plot box
    parts.append(render.numbers(lo, 1, 8, bottom, word(BLACK, Z_TEXT), s, "left", 2, 2, frame, justify="left"))
    parts.append(render.numbers(hi, 1, 8, (X1, Y0 - 0.5), word(BLACK, Z_TEXT), s, "right", 0, 2, frame))
    if la:
        anchors = torch.stack((torch.full_like(y, X1 + 3.0), y), dim=1)
        for k in range(A):      # host strings: one text per row, for all frames
            if lw is None:
                parts.append(render.text(la[k], anchors[k], word(BLACK, Z_TEXT), 1, "left", 0, -3, 0, F - 1))
            else:
                parts.append(render.text(la[k] + "\n" + lw[k], anchors[k], word(BLACK, Z_TEXT), 1, "left", 0, -render.GLYPH_LINE + 1, 0, F - 1))
    return torch.cat(parts)


def return_dist_prims(quantiles, cvar, title=None, width=480, height=360, xlim="frame", labels=True, params=None):
    """The primitives of `return_dist_panel`: per frame and action row a baseline, the K quantile values as green crosses, a line from the row's
    least to its largest, and the mean as a bar of +-0.35 rows -- red and wider on the row whose mean is largest, blue elsewhere."""
    q = torch.as_tensor(quantiles).to(torch.float64)
    if q.dim() != 3:
        raise ValueError(f"quantiles is [F][K][A], got {tuple(q.shape)}")
    F = int(q.shape[0])
    cv = render._per_prim(cvar, F, torch.float64, q.device)
    lo, hi = _limits(q, xlim, F)
    return _bars_prims(q.mean(dim=1), q, lo, hi, "phi = " if title is None else str(title), cv, width, height, labels, params)


def _draw(prims, F, width, height, canvas):
    canvas = blank(F, width, height, prims.device) if canvas is None else canvas
    if canvas.n_images != F:
        raise ValueError(f"the canvas has {canvas.n_images} images for {F} frames")
    return canvas.draw(prims)


def return_dist_panel(quantiles, cvar, title=None, width=480, height=360, xlim="frame", labels=True, params=None, canvas=None):
    """The reference's plot_return_dist for F frames at once: `quantiles` [F][K][9] (a step's row of rollout_iqn(..., want_quantiles=True)["quantiles"]
    or of maps.iqn_policy(..., quantiles=True)), `cvar` [F] or a float -- the title reads `title` (default "phi = ", the reference's first panel
    says "adaptive phi = ") followed by cvar to two decimals, taken from the device.  `xlim` "frame": min - 5 .. max + 5 of every frame's own
    quantiles; or (lo, hi), floats or [F] tensors (`shared_limits` of all panels shown together gives the reference's common axis).  `labels`: the
    a / w labels of `params`' action table on the right (needs `params`).  Returns a Canvas of F images; ONE draw launch."""
    prims = return_dist_prims(quantiles, cvar, title, width, height, xlim, labels, params)
    return _draw(prims, int(torch.as_tensor(quantiles).shape[0]), width, height, canvas)


def q_values_prims(q, title="Action Values", width=480, height=360, xlim="frame", labels=True, params=None):
    v = torch.as_tensor(q).to(torch.float64)
    if v.dim() != 2:
        raise ValueError(f"q is [F][A], got {tuple(v.shape)}")
    lo, hi = _limits(v, xlim, int(v.shape[0]))
    return _bars_prims(v, None, lo, hi, str(title), None, width, height, labels, params)


def q_values_panel(q, title="Action Values", width=480, height=360, xlim="frame", labels=True, params=None, canvas=None):
    """The reference's plot_action_qvalues: `q` [F][9] (DQNPolicy.rollout(trace=("q", ...))) as bars, red on the largest."""
    return _draw(q_values_prims(q, title, width, height, xlim, labels, params), int(torch.as_tensor(q).shape[0]), width, height, canvas)


def _reflections(obs):
    return obs[:, 4:].reshape(obs.shape[0], -1, 2)


def sonar_prims(obs, sonar_range, half_angle, width=320, height=320, title="LiDAR Reflections"):
    """The robot-frame part of plot_measurements: the field of view as a SECTOR in a light tint at low z, every
    reflection of `obs` [F][26] with a non-zero point as a blue disc at (-y, x) -- the robot looks up --, over x in [-R - 1, R + 1] and y in
    [-1, R + 1] with equal scales.  A missed beam is the row's (0, 0) pair."""
    obs = torch.as_tensor(obs).to(torch.float64)
    F, dev = int(obs.shape[0]), obs.device
    W, H, s, R = int(width), int(height), text_scale(width), float(sonar_range)
    top = render.GLYPH_LINE * s + 2
    k = min(W / (2.0 * R + 2.0), (H - top) / (R + 2.0))      # pixels per unit
    ox, oy = W / 2.0, (H - top) / 2.0 - (R / 2.0) * k      # the robot: the box [-1, R + 1] is centred under the title
    # one record per frame, not one for all: a wavefront serves a primitive, and the wedge is most of the panel
    parts = [render.sectors([[ox, oy]] * F, [[ox, oy + R * k]] * F, half_angle, word(WEDGE, Z_TINT), _frames(F, dev), None, dev)]
    b = _reflections(obs)
    miss = (b[..., 0] == 0.0) & (b[..., 1] == 0.0)
    nan = torch.full_like(b[..., 0], float("nan"))
    centres = torch.stack((torch.where(miss, nan, ox - b[..., 1] * k), torch.where(miss, nan, oy + b[..., 0] * k)), dim=-1)
    parts.append(render.discs(centres, max(1.5, 0.012 * W), word(BLUE, Z_MARK), _frames(F, dev)[:, None].expand(F, b.shape[1])))
    _title(parts, title, None, 0, 0, W, H, s, F, dev)
    return torch.cat(parts)


def sonar_panel(obs, sonar_range, half_angle, width=320, height=320, title="LiDAR Reflections", canvas=None):
    return _draw(sonar_prims(obs, sonar_range, half_angle, width, height, title), int(torch.as_tensor(obs).shape[0]), width, height, canvas)


def velocity_prims(obs, width=320, height=320, title="Velocity Measurement"):
    """The velocity part of plot_measurements: the steer direction (0, 0) -> (0, 1) in black and the measured velocity (-v_y, v_x) of `obs` [F][26]
    (its first two entries, robot frame) as a red arrow, over x in [-xr, xr], y in [-1, yr] with xr = max(2, |v_y|), yr = max(2, |v_x|) and equal
    scales -- the reference's rule, applied per frame on the device; then the two legend lines."""
    obs = torch.as_tensor(obs).to(torch.float64)
    F, dev = int(obs.shape[0]), obs.device
    W, H, s = int(width), int(height), text_scale(width)
    top, legend = render.GLYPH_LINE * s + 2, 2 * render.GLYPH_LINE * s + 2
    vx, vy = obs[:, 0], obs[:, 1]
    xr, yr = vy.abs().clamp(min=2.0), vx.abs().clamp(min=2.0)
    box_h = float(H - top - legend)
    k = torch.minimum(W / (2.0 * xr), box_h / (yr + 1.0))      # [F] pixels per unit
    ox, oy = torch.full_like(k, W / 2.0), legend + box_h / 2.0 - (yr - 1.0) / 2.0 * k
    o = torch.stack((ox, oy), dim=1)
    frame = _frames(F, dev)
    view, size, head, hw = (0.0, 0.0, float(W), float(H)), (W, H), max(3.0, 0.03 * W), 0 if s == 1 else 1
    parts = [render.arrows(o, torch.stack((ox, oy + k), dim=1), head, word(BLACK, Z_LINE), view, size, frame, None, hw),
             render.arrows(o, torch.stack((ox - vy * k, oy + vx * k), dim=1), head, word(RED, Z_MARK), view, size, frame, None, hw)]
    _title(parts, title, None, 0, 0, W, H, s, F, dev)
    parts.append(render.text("- steer direction", (0.5, legend - 0.5), word(BLACK, Z_TEXT), s, "left", 2, 1, 0, F - 1, dev))
    parts.append(render.text("- velocity wrt seafloor", (0.5, legend - 0.5), word(RED, Z_TEXT), s, "left", 2, 1 + render.GLYPH_LINE * s, 0, F - 1, dev))
    return torch.cat(parts)


def velocity_panel(obs, width=320, height=320, title="Velocity Measurement", canvas=None):
    return _draw(velocity_prims(obs, width, height, title), int(torch.as_tensor(obs).shape[0]), width, height, canvas)


def goal_prims(obs, width=320, height=120):
    """The reference's two goal lines: "Goal Position (Relative)" and "(x, y)" of `obs` [F][26] (entries 2 and 3, robot frame) to two decimals."""
    obs = torch.as_tensor(obs).to(torch.float64)
    F, dev = int(obs.shape[0]), obs.device
    W, H, s = int(width), int(height), text_scale(width)
    frame = _frames(F, dev)
    line = render.GLYPH_LINE * s
    y0 = max(1, (H - 2 * line) // 2)
    anchor, adv = (0.5, H - 0.5), render.GLYPH_ADVANCE * s
    parts = [render.text("Goal Position (Relative)", anchor, word(BLACK, Z_TEXT), s, "left", 2, y0, 0, F - 1, dev),
             render.text("(", anchor, word(BLACK, Z_TEXT), s, "left", 2, y0 + line, 0, F - 1, dev),
             render.numbers(obs[:, 2], 2, 7, anchor, word(BLACK, Z_TEXT), s, "left", 2 + adv, y0 + line, frame),
             render.text(",", anchor, word(BLACK, Z_TEXT), s, "left", 2 + 8 * adv, y0 + line, 0, F - 1, dev),
             render.numbers(obs[:, 3], 2, 7, anchor, word(BLACK, Z_TEXT), s, "left", 2 + 9 * adv, y0 + line, frame),
             render.text(")", anchor, word(BLACK, Z_TEXT), s, "left", 2 + 16 * adv, y0 + line, 0, F - 1, dev)]
    return torch.cat(parts)


def goal_panel(obs, width=320, height=120, canvas=None):
    return _draw(goal_prims(obs, width, height), int(torch.as_tensor(obs).shape[0]), width, height, canvas)


def action_prims(actions, params, width=240, height=320):
    """The reference's plot_action_and_steer_state of a video: "Action", "a: -0.40", "w:  0.52" by the action index `actions` [F] (a device int
    tensor; -1, a finished env's entry, writes blanks) from the action table of `params`, chosen on the device."""
    actions = torch.as_tensor(actions).reshape(-1)
    F, dev = int(actions.shape[0]), actions.device
    W, H, s = int(width), int(height), text_scale(width)
    la, lw = action_labels(params)
    frame, line = _frames(F, dev), render.GLYPH_LINE * s + s
    y0 = max(1, (H - 3 * line) // 2)
    anchor = torch.tensor([[0.5, H - 0.5]], dtype=torch.float64, device=dev).expand(F, 2)
    return torch.cat((render.text("Action", anchor[0], word(BLACK, Z_TEXT), s, "left", 2, y0, 0, F - 1),
                      render.choose_text(la, actions, anchor, word(BLACK, Z_TEXT), s, "left", 2, y0 + line, frame),
                      render.choose_text(lw, actions, anchor, word(BLACK, Z_TEXT), s, "left", 2, y0 + 2 * line, frame)))


def action_panel(actions, params, width=240, height=320, canvas=None):
    return _draw(action_prims(actions, params, width, height), int(torch.as_tensor(actions).reshape(-1).shape[0]), width, height, canvas)


def title_prims(title, subtitle, width, height, F, device=None):
    """The title strip: `title` large, the lines of `subtitle` under it; a record per character and FRAME (the large glyphs of one record for all
    frames would be one wavefront's work)."""
    W, H, F = int(width), int(height), int(F)
    big = max(1, min(8, H // 40 + 1))
    small = max(1, big // 2)
    anchor, left = torch.tensor([[0.5, H - 0.5]], dtype=torch.float64, device=device).expand(F, 2), max(2, W // 40)
    frame = _frames(F, anchor.device)
    lines = [str(t) for t in subtitle]
    total = render.GLYPH_LINE * big + render.GLYPH_LINE * small * len(lines)
    y0 = max(1, (H - total) // 2)
    parts = [render.text(str(title), anchor, word(BLACK, Z_TEXT), big, "left", left, y0, frame)]
    for k, t in enumerate(lines):
        parts.append(render.text(t, anchor, word(BLACK, Z_TEXT), small, "left", left, y0 + render.GLYPH_LINE * big + render.GLYPH_LINE * small * k, frame))
    return torch.cat(parts)


# ---- the whole frame ----------------------------------------------------------------------------------------------------------------------------------
def video_layout(kind, size, n_dist=1):
    """name -> (x, y, w, h), pixels from the top-left, of the reference's three draw_video_plots grids scaled to `size` = (width, height): "iqn"
    (7 rows x (3 + n_dist) columns: title 2 rows; goal 1, sonar 2, velocity 2 rows in column 0; the map in columns 1-2; one distribution panel per
    further column), "dqn" (13 x 4: title 3 rows; goal 2, sonar 4, velocity 4; map columns 1-2; Q-values column 3) and "planner" (13 x 8: a margin
    column; goal / sonar / velocity in columns 1-2; map columns 3-6; the action text in column 7, rows 5-8).  The map slot is the largest square
    that fits its columns, centred."""
    W, H = int(size[0]), int(size[1])
    if kind == "iqn":
        rows, cols, head, left, maps, goal, sonar = 7, 3 + int(n_dist), 2, (0, 1), (1, 3), (2, 3), (3, 5)
    elif kind == "dqn":
        rows, cols, head, left, maps, goal, sonar = 13, 4, 3, (0, 1), (1, 3), (3, 5), (5, 9)
    elif kind == "planner":
        rows, cols, head, left, maps, goal, sonar = 13, 8, 3, (1, 3), (3, 7), (3, 5), (5, 9)
    else:
        raise ValueError(f"video_layout: kind is 'iqn', 'dqn' or 'planner', got {kind!r}")
    cx = lambda c: c * W // cols
    ry = lambda r: r * H // rows

    def cell(r0, r1, c0, c1):
        return (cx(c0), ry(r0), cx(c1) - cx(c0), ry(r1) - ry(r0))
    out = {"title": cell(0, head, 0, cols), "goal": cell(goal[0], goal[1], *left), "sonar": cell(sonar[0], sonar[1], *left), "velocity": cell(sonar[1], rows, *left)}
    x, y, w, h = cell(head, rows, *maps)
    m = max(1, min(w, h))
    out["map"] = (x + (w - m) // 2, y + (h - m) // 2, m, m)
    if kind == "iqn":
        for i in range(int(n_dist)):
            out[f"dist{i}"] = cell(head, rows, 3 + i, 4 + i)
    elif kind == "dqn":
        out["q"] = cell(head, rows, 3, 4)
    else:
        out["action"] = cell(5, 9, 7, 8)
    return out


def _pick(t, rows):
    return None if t is None else torch.as_tensor(t)[rows.to(torch.as_tensor(t).device)]


def video_frames(env, env_index, states, traj, obs, actions=None, dist=None, q=None, title=None, subtitle=(), every=1, size=(1920, 1080), steps=None,
                 start=None, beams=True, style=None, return_parts=False, **frame_kw):
    """The frames of the reference's episode video, uint8 [F][H][W][3] on the device: a title strip, the left column of goal / sonar / velocity
    panels, the map (`render.episode_frames` of `states` [T][6] and `traj` [T][N][2] in world `env_index` of `env`) and, on the right, the IQN
    layout's distribution panels (`dist`: a list of (title, cvar [T] or float, quantiles [T][K][9]), all on one axis per frame as in the
    reference), the DQN layout's Q-values (`q` [T][9]) or the planner layout's action text (`actions` [T]).  `obs` [T][26] float64 are the
    observations of the steps' states (`env.observation_at`), `every` shows every that many steps: frame f is step f * every, as in
    `episode_frames`.  Every part is a Canvas of its own -- ONE mn_render_worlds launch for the map's background, ONE mn_render_draw launch per
    canvas -- and the parts are joined by slicing; nothing is copied to the host.  `return_parts`: also name -> (canvas, (x, y, w, h))."""
    states, traj = torch.as_tensor(states), torch.as_tensor(traj)
    if states.dim() == 3:
        states = states[:, 0]
    if traj.dim() == 4:
        traj = traj[:, 0]
    T = int(traj.shape[0]) if steps is None else min(int(steps), int(traj.shape[0]))
    every = max(1, int(every))
    F = (T + every - 1) // every
    dev = env.device
    rows = (torch.arange(F, device=dev) * every).clamp(max=T - 1)
    kind = "iqn" if dist is not None else ("dqn" if q is not None else "planner")
    if kind == "planner" and actions is None:
        raise ValueError("video_frames: one of dist, q or actions says which layout to draw")
    W, H = int(size[0]), int(size[1])
    slots = video_layout(kind, (W, H), len(dist) if dist is not None else 1)
    params = env.params
    obs_f = _pick(obs, rows).to(device=dev, dtype=torch.float64)
    parts = {}
    x, y, w, h = slots["title"]
    default_title = {"iqn": "Adaptive IQN performance", "dqn": "DQN performance", "planner": "Planner performance"}[kind]
    parts["title"] = blank(F, w, h, dev).draw(title_prims(default_title if title is None else title, subtitle, w, h, F, dev))
    x, y, w, h = slots["goal"]
    parts["goal"] = goal_panel(obs_f, w, h)
    x, y, w, h = slots["sonar"]
    parts["sonar"] = sonar_panel(obs_f, float(params.sonar_range), float(params.sonar_angle) / 2.0, w, h)
    x, y, w, h = slots["velocity"]
    parts["velocity"] = velocity_panel(obs_f, w, h)
    x, y, w, h = slots["map"]
    parts["map"] = render.episode_frames(env, env_index, states, traj, beams=beams, every=every, steps=T, start=start, width=w, height=h, style=style,
                                         observe=(lambda st: obs_f) if beams else None, **frame_kw)
    if kind == "iqn":
        blocks = [_pick(qt, rows).to(device=dev, dtype=torch.float64) for _, _, qt in dist]
        lim = shared_limits(blocks)
        for i, (name, cvar, _) in enumerate(dist):
            x, y, w, h = slots[f"dist{i}"]
            cv = _pick(cvar, rows) if torch.is_tensor(cvar) else cvar
            parts[f"dist{i}"] = return_dist_panel(blocks[i], cv, name, w, h, lim, labels=i == len(dist) - 1, params=params)
    elif kind == "dqn":
        x, y, w, h = slots["q"]
        parts["q"] = q_values_panel(_pick(q, rows).to(dev), "Action Values", w, h, "frame", True, params)
    else:
        x, y, w, h = slots["action"]
        parts["action"] = action_panel(_pick(actions, rows).to(dev), params, w, h)
    out = torch.full((F, H, W, 3), 255, dtype=torch.uint8, device=dev)
    for name, canvas in parts.items():
        x, y, w, h = slots[name]
        out[:, y:y + h, x:x + w] = canvas.rgb()
    if return_parts:
        return out, {name: (canvas, slots[name]) for name, canvas in parts.items()}
    return out
