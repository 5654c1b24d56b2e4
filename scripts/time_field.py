"""Minimum-time-to-goal fields of evaluation worlds: what travel time was achievable in a world, and how close a policy's episodes come to it.

    python scripts/time_field.py --eval-config tests/golden/eval_config_seed3.json --worlds 0:30 --out fields.npz
    python scripts/time_field.py --eval-config tests/golden/eval_config_seed3.json --worlds 0:6 --out fields.npz --png fields.png
    python scripts/time_field.py --eval-config tests/golden/eval_config_seed3.json --worlds 0:30 --out fields.npz --compare APF BA \\
        --iqn tests/golden/pretrained_IQN_seed3 --adaptive --dqn tests/golden/pretrained_DQN_seed3/q_net.npz

--out FILE.npz: `T` [worlds][ny][nx] float64 (seconds to the goal from every cell of the --nx x --ny grid for a vehicle of constant --speed, default
the robot's max_speed, kept --clearance beyond r + robot_r away from every obstacle; +inf: the goal cannot be reached), `dir` (the stencil direction
of the first move, 255: none), `status`, `sweeps`, `worlds`, and `T_start` (T at each world's start: the yardstick).  One launch, one workgroup per
world (VecMarineNavEnv.time_field -> mn_time_field).
--png FILE.png: one tile per world: the flow image (render.world_images) with T as isochrone bands of --band seconds laid over the water by palette
indexing, cells the goal cannot be reached from in grey, and the field's own route from the world's start (maps.time_path) drawn over it.
--compare: the named policies' episodes on the same worlds through the existing one-launch functions; per policy the success count, and the median
and range of time / T(start) over its successful episodes from starts the grid reaches the goal from.  T is the time of a vehicle that turns and
accelerates at once and always runs at --speed, over-estimated by the 16-direction stencil (up to 2.75 % in still water) and by averaging the
current per edge: a ratio slightly below 1 is possible.  PILOT among --compare is the upper baseline: it knows the whole map and follows the field
under the real dynamics, so a policy's ratio divided by the pilot's median is its time against what the real robot can do.
    python scripts/time_field.py --eval-config tests/golden/eval_config_seed3.json --compare APF BA PILOT --pilot-horizon 2"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BANDS = (0xFFF3BF, 0xFFD8A8, 0xFFC9C9, 0xEEBEFA, 0xD0BFFF, 0xA5D8FF, 0x99E9F2, 0xB2F2BB)
UNREACHABLE = 0x868E96
ROUTE = 0xE8590C


def _policies(args):
    """[(label, run)]: run(env, T, fields) -> the traces "done" and "info" of every env's episode, by the policy's one-launch function (`fields`: the
    worlds' time fields, which only the field pilot reads)."""
    trace = ("reward", "done", "info", "action")
    out = []
    for name in args.compare or ():
        if name == "PILOT":
            out.append((f"PILOT horizon {args.pilot_horizon}", lambda env, T, fields: env.rollout_pilot(T, fields, horizon=args.pilot_horizon, trace=trace)))
        else:
            out.append((name, lambda env, T, fields, name=name: env.rollout_policy(T, name, trace=trace)))
    for path in args.iqn or ():
        from distributional_rl_navigation_amd.iqn.agent import IQNAgent
        from distributional_rl_navigation_amd.iqn.fused_act import ActRng, rollout_iqn
        agent = IQNAgent(26, 9, device=args.device, seed=args.seed, BUFFER_SIZE=1024)
        agent.load_model(path, args.device)

        def run(env, T, fields, agent=agent):
            tr = rollout_iqn(agent.qnetwork_local, env, T, ActRng(args.seed, env.device), cvar=args.cvar, adaptive=args.adaptive, trace=trace)
            if tr is None:
                raise SystemExit("the IQN episode launch refused this form")
            return tr
        out.append(("IQN adaptive" if args.adaptive else f"IQN cvar {args.cvar:g}", run))
    for path in args.dqn or ():
        from distributional_rl_navigation_amd.dqn import DQNPolicy
        pol = DQNPolicy.load(path, device=args.device)

        def run(env, T, fields, pol=pol):
            tr = pol.rollout(env, T, trace=trace)
            if tr is None:
                raise SystemExit("the DQN episode launch does not run this network")
            return tr
        out.append(("DQN", run))
    return out


def banded(canvas, T, band_s, torch):
    """`canvas` (flow images [I][H][W]) with field i's isochrone bands laid over the water pixels (z = 0) of image i: the pixel's centre picks its
    cell, floor(T / band_s) mod the palette its colour; a cell with T = +inf is grey.  Obstacles and markers stay.  All on the device."""
    from distributional_rl_navigation_amd import render
    n, H, W = canvas.pixels.shape
    _, ny, nx = T.shape
    x0, y0, x1, y1 = canvas.view
    dev = T.device
    x = x0 + (torch.arange(W, dtype=torch.float64, device=dev) + 0.5) * ((x1 - x0) / W)
    y = y1 - (torch.arange(H, dtype=torch.float64, device=dev) + 0.5) * ((y1 - y0) / H)
    i = torch.floor(x / ((x1 - x0) / nx)).long().clamp(0, nx - 1)
    j = torch.floor(y / ((y1 - y0) / ny)).long().clamp(0, ny - 1)
    t = T[:, j][:, :, i]      # [I][H][W]
    reach = torch.isfinite(t)
    pal = torch.tensor(BANDS, dtype=torch.int32, device=dev)
    band = torch.floor(torch.where(reach, t, torch.zeros_like(t)) / float(band_s)).long() % len(BANDS)
    p = canvas.pixels.view(torch.int32)
    water = ((p >> 24) & 255) == render.Z_FIELD
    lic = (p & 255).float() / 250.0      # the flow image's own shading (its blue channel runs 107..250) keeps the streamlines visible under the bands
    col = pal[band]
    shaded = torch.zeros_like(col)
    for shift in (16, 8, 0):
        shaded |= (((col >> shift) & 255).float() * lic.clamp(0.45, 1.0)).to(torch.int32).clamp(0, 255) << shift
    new = torch.where(water, torch.where(reach, shaded, torch.full_like(p, UNREACHABLE)), p)
    return render.Canvas(new.view(torch.uint32).contiguous(), canvas.view)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--eval-config", required=True, help="eval_config.json (the episode_data schema)")
    ap.add_argument("--worlds", metavar="A:B", help="worlds A .. B - 1 (default: all)")
    ap.add_argument("--nx", type=int, default=128)
    ap.add_argument("--ny", type=int, default=128)
    ap.add_argument("--speed", type=float, default=None, help="vehicle speed through the water (default: max_speed)")
    ap.add_argument("--clearance", type=float, default=0.0)
    ap.add_argument("--max-sweeps", type=int, default=None)
    ap.add_argument("--out", metavar="FILE.npz")
    ap.add_argument("--png", metavar="FILE.png")
    ap.add_argument("--width", type=int, default=256, help="pixels per tile of --png")
    ap.add_argument("--band", type=float, default=2.0, help="seconds per isochrone band of --png")
    ap.add_argument("--cols", type=int, default=0)
    ap.add_argument("--v-max", type=float, default=4.0)
    ap.add_argument("--compare", nargs="*", choices=("APF", "BA", "PILOT"), metavar="POLICY",
                    help="APF, BA and / or PILOT (the field pilot on these very fields: VecMarineNavEnv.rollout_pilot); --iqn / --dqn add learned policies")
    ap.add_argument("--pilot-horizon", type=int, default=2, help="the look-ahead of PILOT in steps (1..16)")
    ap.add_argument("--iqn", action="append", metavar="DIR")
    ap.add_argument("--adaptive", action="store_true")
    ap.add_argument("--cvar", type=float, default=1.0)
    ap.add_argument("--dqn", action="append", metavar="FILE")
    ap.add_argument("--max-steps", type=int, default=1000)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--device", default="cuda:0")
    args = ap.parse_args(argv)
    if not (args.out or args.png or args.compare is not None or args.iqn or args.dqn):
        ap.error("one or more of --out, --png, --compare")

    import numpy as np
    import torch
    from distributional_rl_navigation_amd import _capi, maps, render
    from distributional_rl_navigation_amd.marinenav_env.vec_env import VecMarineNavEnv
    with open(args.eval_config) as f:
        cfg = json.load(f)
    a, b = (int(v) for v in args.worlds.split(":")) if args.worlds else (0, len(cfg))
    which = list(range(a, b))
    worlds = [VecMarineNavEnv.world_from_eval_config(cfg[f"env_{k}"]) for k in which]
    env = VecMarineNavEnv(len(worlds), device=args.device, precision="f64")
    env.load_worlds(worlds)
    idx = torch.arange(len(worlds), dtype=torch.int32)
    T, d, status, sweeps = env.time_field(idx, args.nx, args.ny, speed=args.speed, clearance=args.clearance, max_sweeps=args.max_sweeps)
    late = [which[i] for i in torch.nonzero(status == _capi.TIME_FIELD_NOT_CONVERGED).view(-1).tolist()]
    if late:
        raise SystemExit(f"worlds {late} did not converge in {args.max_sweeps or 4 * (args.nx + args.ny)} sweeps: raise --max-sweeps")
    W, Hm = float(env.params.width), float(env.params.height)
    fields = [maps.field_dict(T[i], d[i], W, Hm, int(status[i]), int(sweeps[i])) for i in range(len(worlds))]
    starts = torch.tensor(np.array([w["start"] for w in worlds], dtype=np.float64), device=env.device)
    t_start = torch.stack([maps.time_at(fields[i], starts[i:i + 1])[0] for i in range(len(worlds))])
    unreachable = [which[i] for i in torch.nonzero(~torch.isfinite(t_start)).view(-1).tolist()]
    finite = t_start[torch.isfinite(t_start)]
    print(f"{len(worlds)} fields of {args.nx} x {args.ny}: sweeps {int(sweeps.min())}..{int(sweeps.max())}; T(start) "
          + (f"{float(finite.min()):.2f}..{float(finite.max()):.2f} s" if finite.numel() else "-")
          + f"; worlds whose start cannot reach the goal on this grid: {unreachable if unreachable else 'none'}")
    if args.out:
        np.savez(args.out, T=T.cpu().numpy(), dir=d.cpu().numpy(), status=status.cpu().numpy(), sweeps=sweeps.cpu().numpy(), worlds=np.array(which),
                 T_start=t_start.cpu().numpy())
        print(f"{args.out}: T, dir [{len(worlds)}][{args.ny}][{args.nx}], status, sweeps, worlds, T_start")
    if args.png:
        canvas = banded(render.world_images(env, idx, width=args.width, style=render.Style(v_max=args.v_max)), T, args.band, torch)
        prims = []
        for i in range(len(worlds)):
            path, lengths = maps.time_path(fields[i], starts[i:i + 1])
            if int(lengths[0]) >= 2:
                prims.append(render.polylines(path, render.word(ROUTE, render.Z_TRAIL), image_first=i, half_width=1 if args.width >= 192 else 0))
        if prims:
            canvas.draw(torch.cat(prims))
        rgb = canvas.rgb()
        cols = args.cols or int(np.ceil(np.sqrt(rgb.shape[0])))
        render.save_png(args.png, render.contact_sheet(rgb, cols, gap=2, fill=255))
        print(f"{args.png}: {rgb.shape[0]} tiles of {rgb.shape[2]} x {rgb.shape[1]}, {cols} per row; bands of {args.band:g} s, {len(prims)} routes")
    for label, run in _policies(args):
        env.load_worlds(worlds)
        tr = run(env, args.max_steps, T)
        done = tr["done"].bool()
        last = done.to(torch.uint8).argmax(dim=0)
        success = done.any(dim=0) & (tr["info"][last, torch.arange(len(worlds), device=env.device)] == 4)
        time = (last + 1).double() * (env.params.dt * env.params.N)
        ok = success & torch.isfinite(t_start)
        ratio = (time / t_start)[ok]
        line = f"{label}: {int(success.sum())} of {len(worlds)} succeed"
        if ratio.numel():
            line += f"; time / T(start) over {ratio.numel()}: median {float(ratio.median()):.3f}, range {float(ratio.min()):.3f}..{float(ratio.max()):.3f}"
        print(line)
    env.close()


if __name__ == "__main__":
    main()
