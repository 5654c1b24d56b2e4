"""Times the picture launches on one MI355X and writes profiles/render_bench.txt.

    python scripts/render_bench.py [--out FILE] [--reps 5] [--inner 3]

Medians of `--reps` timed windows of `--inner` calls after a warm-up window, all cases alternating in one process; wall time per call, synchronised,
with the range.  Cases: world_images for the 30 worlds of tests/golden/eval_config_seed3.json at 512 x 512 with LIC off, 12 and 32 steps; 4 000
thumbnails of 128 x 128; as the yardstick of the LIC-off field layer what the package offered before for the same pixels -- velocity_at on the pixel
grid plus torch palette indexing (the grid itself is built once, outside the window); mn_render_draw for one 1 000-step episode (a synthetic smooth
walk, N = 10 sub-steps) into 250 frames of 512 x 512 (the primitive buffer is built once, outside); episode_sheet for 500 worlds x 8 traces of 1 000
steps at 128 x 128 (building the primitives from the traces included).  Nothing is asserted.

    python scripts/render_bench.py --panels [--out profiles/render_panels_bench.txt]

--panels: the side panels and the whole video frame instead (render_panels.py): one 1 000-step episode as 250 frames of 1920 x 1080 in the IQN layout
with two distribution panels (synthetic quantiles and observations) -- the record building of every panel (torch), the draw launch of every canvas
(records built once, outside the window), launches of the distribution panel's MARKER records and GLYPH records alone, and the whole `video_frames`
call; for scale the mn_render_draw frame case above in the same run.  Each draw case also reports the pixels it covered (counted once, outside)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
G = os.path.join(ROOT, "tests", "golden")


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=None, help="default: profiles/render_bench.txt, with --panels profiles/render_panels_bench.txt")
    ap.add_argument("--panels", action="store_true")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--inner", type=int, default=3)
    ap.add_argument("--device", default="cuda:0")
    args = ap.parse_args(argv)
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "render_panels_bench.txt" if args.panels else "render_bench.txt")
    import numpy as np
    import torch
    from distributional_rl_navigation_amd import render
    from distributional_rl_navigation_amd.marinenav_env.vec_env import VecMarineNavEnv
    with open(os.path.join(G, "eval_config_seed3.json")) as f:
        cfg = json.load(f)
    worlds = [VecMarineNavEnv.world_from_eval_config(cfg[f"env_{k}"]) for k in range(len(cfg))]
    env = VecMarineNavEnv(len(worlds), device=args.device, precision="f64")
    env.load_worlds(worlds)
    dev, nw = env.device, len(worlds)
    all30 = torch.arange(nw, dtype=torch.int32, device=dev)
    thumbs = torch.arange(4000, dtype=torch.int32, device=dev) % nw
    styles = {s: render.Style(lic=s > 0, lic_steps=s) for s in (0, 12, 32)}

    # the yardstick: the same pixel centres through velocity_at, the same levels and palette through torch
    W = H = 512
    c = (torch.arange(W, dtype=torch.float64, device=dev) + 0.5) * (50.0 / W)
    r = 50.0 - (torch.arange(H, dtype=torch.float64, device=dev) + 0.5) * (50.0 / H)
    grid = torch.stack(torch.meshgrid(r, c, indexing="ij")[::-1], dim=-1).reshape(1, H * W, 2).expand(nw, -1, -1).reshape(-1, 2).contiguous()
    grid_env = all30.repeat_interleave(H * W)
    pal = torch.tensor(styles[0].palette, dtype=torch.int32, device=dev)

    def torch_field():
        v = env.velocity_at(grid, env=grid_env)
        t = torch.linalg.vector_norm(v, dim=1) / styles[0].v_max * len(styles[0].palette)
        level = torch.where(torch.isfinite(t) & (t < len(styles[0].palette)), t.floor(), torch.full_like(t, len(styles[0].palette) - 1)).long()
        return pal[level].reshape(nw, H, W)

    # one 1 000-step episode as 250 frames
    T, N, F = 1000, 10, 250
    a = torch.linspace(0, 6 * np.pi, T * N, dtype=torch.float64, device=dev)
    walk = torch.stack((5.0 + 40.0 * torch.arange(T * N, device=dev) / (T * N) + 1.5 * torch.sin(a), 25.0 + 18.0 * torch.sin(a / 3)), dim=1)
    traj1 = walk.reshape(T, N, 2)
    st1 = torch.cat((traj1[:, -1], torch.zeros(T, 4, dtype=torch.float64, device=dev)), dim=1)
    frame_buf = render.frame_prims(st1, traj1, F, every=T // F, robot_r=0.8)
    frames = render.world_images(env, 0, width=512, style=styles[12]).repeat(F)

    if args.panels:
        return panels_bench(args, env, st1, traj1, frame_buf, frames)

    # 500 worlds x 8 traces
    n_sheet = 500
    sheet_worlds = torch.arange(n_sheet, dtype=torch.int32, device=dev) % nw
    phase = torch.arange(n_sheet, dtype=torch.float64, device=dev)[None, :, None]
    tt = torch.arange(T * N, dtype=torch.float64, device=dev).reshape(T, 1, N) / (T * N)
    traces = [torch.stack((5.0 + 40.0 * tt + torch.sin(6.0 * tt + phase + k), 5.0 + 40.0 * tt + 2.0 * torch.cos(9.0 * tt + 0.37 * phase * k)), dim=-1).contiguous()
              for k in range(8)]
    steps = torch.full((n_sheet,), T, dtype=torch.int64, device=dev)
    sheet = render.world_images(env, sheet_worlds, width=128, style=styles[12])

    def sheets():
        for k, tr in enumerate(traces):
            render.episode_sheet(env, tr, steps, color=0x102030 * (k + 1), canvas=sheet)

    cases = [("world_images 30 x 512 x 512, LIC off", lambda: render.world_images(env, all30, width=512, style=styles[0]), 30 * 512 * 512, "pixel"),
             ("world_images 30 x 512 x 512, LIC 12", lambda: render.world_images(env, all30, width=512, style=styles[12]), 30 * 512 * 512, "pixel"),
             ("world_images 30 x 512 x 512, LIC 32", lambda: render.world_images(env, all30, width=512, style=styles[32]), 30 * 512 * 512, "pixel"),
             ("velocity_at + torch palette, 30 x 512 x 512", torch_field, 30 * 512 * 512, "pixel"),
             ("world_images 4 000 x 128 x 128, LIC 12", lambda: render.world_images(env, thumbs, width=128, style=styles[12]), 4000 * 128 * 128, "pixel"),
             (f"mn_render_draw, {frame_buf.shape[0]} primitives of a 1 000-step episode, 250 x 512 x 512", lambda: frames.draw(frame_buf), int(frame_buf.shape[0]), "primitive"),
             ("episode_sheet, 500 worlds x 8 traces of 1 000 steps, 128 x 128", sheets, 8 * n_sheet * (T * N - 1), "segment")]
    report(args, env, cases)


def report(args, env, cases):
    import torch
    times = [[] for _ in cases]
    for rep in range(args.reps + 1):      # the first round warms up
        for i, (_, fn, _, _) in enumerate(cases):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.inner):
                fn()
            torch.cuda.synchronize()
            if rep:
                times[i].append((time.perf_counter() - t0) / args.inner)
    lines = [f"device: {torch.cuda.get_device_name(0)}; medians of {args.reps} windows of {args.inner} calls after a warm-up window, the cases alternating in one "
             "process; wall time per call, synchronised",
             f"{'case':<84}{'median ms':>12}{'min':>10}{'max':>10}{'ns per unit':>14}  unit"]
    for (name, _, count, unit), t in zip(cases, times):
        med = sorted(t)[len(t) // 2]
        lines.append(f"{name:<84}{med * 1e3:>12.3f}{min(t) * 1e3:>10.3f}{max(t) * 1e3:>10.3f}{med / max(count, 1) * 1e9:>14.3f}  {unit}")
    text = "\n".join(lines)
    print(text, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    env.close()


def panels_bench(args, env, states, traj, frame_buf, frames):
    """The --panels cases: see the module's docstring."""
    import numpy as np
    import torch
    from distributional_rl_navigation_amd import render, render_panels as rp
    dev, T, F, every, size = env.device, int(traj.shape[0]), 250, 4, (1920, 1080)
    g = torch.Generator(device="cpu").manual_seed(3)
    drift = torch.cumsum(torch.randn(T, 1, 9, generator=g) * 0.3, dim=0)
    quant = [(drift * s + torch.sort(torch.randn(T, 32, 9, generator=g) * 4.0, dim=1).values - 20.0).to(dev) for s in (1.0, 0.6)]
    cvar = torch.rand(T, generator=g).to(dev)
    obs = torch.zeros(T, 26, dtype=torch.float64)
    obs[:, :4] = torch.randn(T, 4, generator=g, dtype=torch.float64) * torch.tensor([1.0, 0.5, 15.0, 15.0], dtype=torch.float64)
    ang = torch.linspace(-np.pi / 3, np.pi / 3, 11, dtype=torch.float64)
    rng_ = 3.0 + 6.0 * torch.rand(T, 11, generator=g, dtype=torch.float64)
    hit = torch.rand(T, 11, generator=g) < 0.5
    obs[:, 4:] = torch.where(hit[..., None], torch.stack((rng_ * torch.cos(ang), rng_ * torch.sin(ang)), dim=-1), torch.zeros(T, 11, 2, dtype=torch.float64)).reshape(T, 22)
    obs = obs.to(dev)
    rows = (torch.arange(F, device=dev) * every).clamp(max=T - 1)
    slots = rp.video_layout("iqn", size, 2)
    dist = [("adaptive phi = ", cvar, quant[0]), ("phi = ", 1.0, quant[1])]
    params, R, half = env.params, float(env.params.sonar_range), float(env.params.sonar_angle) / 2
    qf, cf, of = quant[0][rows], cvar[rows], obs[rows]
    _, _, dw, dh = slots["dist1"]
    _, _, sw, sh = slots["sonar"]
    _, _, vw, vh = slots["velocity"]
    _, _, gw, gh = slots["goal"]
    _, _, tw, th = slots["title"]
    build = {"return_dist": lambda: rp.return_dist_prims(qf, cf, "phi = ", dw, dh, params=params), "sonar": lambda: rp.sonar_prims(of, R, half, sw, sh),
             "velocity": lambda: rp.velocity_prims(of, vw, vh), "goal": lambda: rp.goal_prims(of, gw, gh),
             "title": lambda: rp.title_prims("Adaptive IQN performance", ("1. a line of text", "2. another line of text"), tw, th, F, dev)}
    bufs = {k: fn() for k, fn in build.items()}
    shapes = {"return_dist": (dw, dh), "sonar": (sw, sh), "velocity": (vw, vh), "goal": (gw, gh), "title": (tw, th)}
    kinds = render.prims_to_numpy(bufs["return_dist"])["kind"]
    only = {name: bufs["return_dist"][torch.from_numpy(np.flatnonzero(kinds == k)).to(dev)].contiguous() for name, k in (("MARKER", 5), ("GLYPH", 6), ("RECT", 4))}
    cases, canvases = [], {}

    def covered(buf, w, h, background=None):      # counted once, outside every window
        c = rp.blank(F, w, h, dev) if background is None else background.clone()
        before = c.pixels.clone().view(torch.int32)
        return int((c.draw(buf).pixels.view(torch.int32) != before).sum())
    n_frame = covered(frame_buf, 512, 512, frames)
    cases.append((f"mn_render_draw, the frame case: {frame_buf.shape[0]} segments and discs, 250 x 512 x 512, {n_frame} pixels covered", lambda: frames.draw(frame_buf), n_frame, "covered pixel"))
    for k, fn in build.items():
        cases.append((f"build {k} records ({bufs[k].shape[0]}), torch", fn, int(bufs[k].shape[0]), "record"))
    for k, buf in bufs.items():
        w, h = shapes[k]
        canvases[k] = rp.blank(F, w, h, dev)
        n = covered(buf, w, h)
        cases.append((f"draw {k}: {buf.shape[0]} records, 250 x {w} x {h}, {n} pixels covered", lambda k=k, buf=buf: canvases[k].draw(buf), n, "covered pixel"))
    for name, buf in only.items():
        canvases[name] = rp.blank(F, dw, dh, dev)
        n = covered(buf, dw, dh)
        cases.append((f"draw the return_dist panel's {name} records alone: {buf.shape[0]}, {n} pixels covered", lambda name=name, buf=buf: canvases[name].draw(buf), n, "covered pixel"))
    whole = lambda: rp.video_frames(env, 0, states, traj, obs, dist=dist, subtitle=("1. a line of text", "2. another line of text"), every=every, size=size)
    cases.append(("video_frames, 250 frames of 1920 x 1080, IQN layout, two distribution panels", whole, F * size[0] * size[1], "pixel"))
    report(args, env, cases)


if __name__ == "__main__":
    main()
