"""Episodes as pictures, made on the device: a sheet of worlds with one trail per policy, or the frames of one episode.

    python scripts/render_episodes.py --eval-config tests/golden/eval_config_seed3.json --worlds 0:6 --planner APF --planner BA \\
        --iqn tests/golden/pretrained_IQN_seed3 --adaptive --dqn tests/golden/pretrained_DQN_seed3/q_net.npz --sheet sheet.png
    python scripts/render_episodes.py --eval-config tests/golden/eval_config_seed3.json --world 3 --planner APF --frames frames/
    python scripts/render_episodes.py --eval-config tests/golden/eval_config_seed3.json --replay tests/golden/g6_pretrained_replay.npz \\
        --subset greedy --episode 0 --max-steps 60 --frames frames/
    python scripts/render_episodes.py --eval-config tests/golden/eval_config_seed3.json --world 3 --iqn tests/golden/pretrained_IQN_seed3 --adaptive \\
        --panels --dist-cvars 1.0,0.5 --width 1920 --every 4 --frames video/

--sheet FILE.png: one tile per world (`--worlds a:b` or `--world k`), every policy's trail in its own colour over the world's flow image
(the reference's draw_trajectory figure).  With --frames, --panels draws the reference's whole video frame around the map (render_panels.video_frames:
title, goal / sonar / velocity panels, and the return distributions of an --iqn run -- the one the actions were chosen from plus one panel per
level of --dist-cvars 1.0,0.5 --, the Q-values of a --dqn run, or the action text of a --planner run or a --replay); --width is then the width of
the whole 16:9 frame.  --frames DIR: `frame_%04d.png` of ONE episode (the first policy named, or the stored action list
`--replay NPZ` of an `*_evaluations.npz` in the layout of tests/golden/g6_pretrained_replay.npz, replayed through `rollout_at` without a handle
row): trail, robot, heading and sonar beams per frame (draw_video_plots without its side panels); a policy's episode is run by its launch and
the actions it chose are replayed the same way, which gives the headings the launch does not trace.  Policies run through the existing episode
launches (`rollout_policy`, `rollout_iqn`, `DQNPolicy.rollout`) with a trajectory trace attached; the trace never leaves the device, only the
finished RGB images do."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COLORS = (0xE8590C, 0x2F9E44, 0x7048E8, 0xF03E3E, 0x0C8599, 0xE64980, 0x5C940D, 0x495057)


def _steps(done):
    """[n] int64 on the device: the steps each env ran on the `done` trace [T][n] (through the step that ended it, or all T)."""
    import torch
    d = done.bool()
    T = d.shape[0]
    return torch.where(d.any(dim=0), d.to(torch.uint8).argmax(dim=0) + 1, torch.full_like(d[0], T, dtype=torch.int64))


def _policies(args):
    """[(label, run)]: run(env, T) -> traces with "traj" and "done" of every env's current episode.  With --panels the traces also hold what the
    policy's panel shows (IQN: "quantiles", "cvar" and "obs" of the batched act_eval form; DQN: "q"); `run.kind` and `run.agent` say whose they are."""
    out = []
    panels = bool(getattr(args, "panels", False))
    for name in args.planner or ():
        run = lambda env, T, name=name: env.rollout_policy(T, name, trace=("done", "action", "traj"))
        run.kind, run.agent = "planner", None
        out.append((name, run))
    for path in args.iqn or ():
        from distributional_rl_navigation_amd.iqn.agent import IQNAgent
        from distributional_rl_navigation_amd.iqn.fused_act import ActRng, rollout_iqn
        agent = IQNAgent(26, 9, device=args.device, seed=args.seed, BUFFER_SIZE=1024)
        agent.load_model(path, args.device)

        def run(env, T, agent=agent):
            tr = rollout_iqn(agent.qnetwork_local, env, T, ActRng(args.seed, env.device), cvar=args.cvar, adaptive=args.adaptive,
                             trace=("done", "action", "traj") + (("cvar", "obs") if panels else ()), want_quantiles=panels)
            if tr is None:
                raise SystemExit("the IQN episode launch refused this form")
            return tr
        run.kind, run.agent = "iqn", agent
        out.append(("IQN adaptive" if args.adaptive else f"IQN cvar {args.cvar:g}", run))
    for path in args.dqn or ():
        from distributional_rl_navigation_amd.dqn import DQNPolicy
        pol = DQNPolicy.load(path, device=args.device)

        def run(env, T, pol=pol):
            tr = pol.rollout(env, T, trace=("done", "action", "traj") + (("q",) if panels else ()))
            if tr is None:
                raise SystemExit("the DQN episode launch does not run this network")
            return tr
        run.kind, run.agent = "dqn", None
        out.append(("DQN", run))
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--eval-config", required=True, help="eval_config.json (the episode_data schema)")
    ap.add_argument("--world", type=int, help="one world")
    ap.add_argument("--worlds", metavar="A:B", help="worlds A .. B - 1")
    ap.add_argument("--iqn", action="append", metavar="DIR")
    ap.add_argument("--adaptive", action="store_true")
    ap.add_argument("--cvar", type=float, default=1.0)
    ap.add_argument("--dqn", action="append", metavar="FILE")
    ap.add_argument("--planner", action="append", choices=("APF", "BA"))
    ap.add_argument("--replay", metavar="NPZ", help="stored action lists (<subset>_ids, <subset>_actions, <subset>_len)")
    ap.add_argument("--subset", default="greedy")
    ap.add_argument("--episode", type=int, default=0, help="row of the subset to replay")
    ap.add_argument("--sheet", metavar="FILE.png")
    ap.add_argument("--frames", metavar="DIR")
    ap.add_argument("--cols", type=int, default=0, help="tiles per row of the sheet (default: about square)")
    ap.add_argument("--width", type=int, default=256, help="pixels per image")
    ap.add_argument("--max-steps", type=int, default=1000)
    ap.add_argument("--every", type=int, default=1, help="a frame every that many steps")
    ap.add_argument("--panels", action="store_true", help="with --frames: the whole video frame, --width wide and 9/16 of that high")
    ap.add_argument("--dist-cvars", default="", metavar="C,C", help="with --iqn --panels: further distribution panels at these CVaR levels")
    ap.add_argument("--no-lic", action="store_true")
    ap.add_argument("--no-beams", action="store_true")
    ap.add_argument("--v-max", type=float, default=4.0)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--device", default="cuda:0")
    args = ap.parse_args(argv)
    if bool(args.sheet) == bool(args.frames):
        ap.error("one of --sheet FILE.png or --frames DIR")
    if args.panels and not args.frames:
        ap.error("--panels draws around --frames")
    dist_cvars = [float(c) for c in args.dist_cvars.split(",") if c.strip()]

    import numpy as np
    import torch
    from distributional_rl_navigation_amd import render, render_panels
    from distributional_rl_navigation_amd.marinenav_env.vec_env import VecMarineNavEnv
    with open(args.eval_config) as f:
        cfg = json.load(f)
    style = render.Style(v_max=args.v_max, lic=not args.no_lic)
    size = (args.width, max(1, args.width * 9 // 16))

    def full_frames(env, out, steps, start, title, **shown):
        """The whole video frame around the map: the observations of the shown states, then render_panels.video_frames."""
        obs = env.observation_at(out["state_trace"][:steps, 0], env=0, velocity="given", dtype=torch.float64)
        return render_panels.video_frames(env, 0, out["state_trace"], out["traj_trace"], obs, title=title, every=args.every, size=size, steps=steps,
                                          start=start, beams=not args.no_beams, style=style, **shown)

    if args.replay:
        if not args.frames:
            ap.error("--replay makes --frames")
        z = np.load(args.replay)
        k = int(z[f"{args.subset}_ids"][args.episode][1])
        n = min(int(z[f"{args.subset}_len"][args.episode]), args.max_steps)
        actions = z[f"{args.subset}_actions"][args.episode][:n].astype(np.int32)
        world = VecMarineNavEnv.world_from_eval_config(cfg[f"env_{k}"])
        env = VecMarineNavEnv(1, device=args.device, precision="f64")
        env.load_worlds([world])
        start = np.array([[world["start"][0], world["start"][1], world["init_theta"], world["init_speed"]]])
        out = env.rollout_at(start, actions, env=0, trace=("state", "traj"), dtype=torch.float64)
        steps = int(out["steps"][0])
        if args.panels:
            rgb = full_frames(env, out, steps, world["start"], f"Stored {args.subset} episode {args.episode}", actions=torch.from_numpy(actions[:steps]).to(env.device))
        else:
            canvas = render.episode_frames(env, 0, out["state_trace"], out["traj_trace"], beams=not args.no_beams, every=args.every, steps=steps,
                                           start=world["start"], width=args.width, style=style)
        what = f"world {k}, {args.subset} episode {args.episode}: {steps} stored steps"
    else:
        if args.worlds:
            a, b = (int(v) for v in args.worlds.split(":"))
            which = list(range(a, b))
        else:
            which = [args.world if args.world is not None else 0]
        policies = _policies(args)
        if not policies:
            ap.error("one or more of --iqn, --dqn, --planner (or --replay)")
        worlds = [VecMarineNavEnv.world_from_eval_config(cfg[f"env_{k}"]) for k in which]
        env = VecMarineNavEnv(len(worlds), device=args.device, precision="f64")      # (the trajectory trace is float64)
        if args.frames:
            label, run = policies[0]
            env.load_worlds(worlds[:1] * len(worlds))
            tr = run(env, args.max_steps)
            steps = int(_steps(tr["done"])[0])
            # the episode launches trace positions, not headings: the actions the policy chose are replayed through rollout_at (the same world, the
            # reference's own float64 arithmetic), which returns the states and the sub-step positions the frames are drawn from
            w0 = worlds[0]
            start = np.array([[w0["start"][0], w0["start"][1], w0["init_theta"], w0["init_speed"]]])
            out = env.rollout_at(start, tr["action"][:steps, 0].clamp(min=0), env=0, trace=("state", "traj"), dtype=torch.float64)
            steps = int(out["steps"][0])
            if args.panels:
                shown = {}
                if run.kind == "iqn":
                    from distributional_rl_navigation_amd import maps
                    shown["dist"] = [("adaptive phi = " if args.adaptive else "phi = ", tr["cvar"][:steps, 0], tr["quantiles"][:steps, 0])]
                    for cv in dist_cvars:      # the same observation rows at a fixed level: the agent's own batched act_eval
                        shown["dist"].append(("phi = ", cv, maps.iqn_policy(run.agent, cv, quantiles=True)(tr["obs"][:steps, 0].contiguous())["quantiles"]))
                elif run.kind == "dqn":
                    shown["q"] = tr["q"][:steps, 0]
                else:
                    shown["actions"] = tr["action"][:steps, 0]
                names = {"APF": "Artificial Potential Field", "BA": "Bug Algorithm"}
                rgb = full_frames(env, out, steps, w0["start"], f"{names.get(label, label)} performance", **shown)
            else:
                canvas = render.episode_frames(env, 0, out["state_trace"], out["traj_trace"], beams=not args.no_beams, every=args.every, steps=steps,
                                               start=w0["start"], width=args.width, style=style)
            what = f"world {which[0]}, {label}: {steps} steps"
        else:
            canvas = render.world_images(env, torch.arange(len(worlds), dtype=torch.int32), width=args.width, style=style)
            notes = []
            for i, (label, run) in enumerate(policies):
                env.load_worlds(worlds)
                tr = run(env, args.max_steps)
                steps = _steps(tr["done"])
                render.episode_sheet(env, tr["traj"], steps, color=COLORS[i % len(COLORS)], canvas=canvas, half_width=1 if args.width >= 192 else 0)
                notes.append(f"{label} #{COLORS[i % len(COLORS)]:06x} (steps {int(steps.min())}..{int(steps.max())})")
            what = f"worlds {which[0]}..{which[-1]}: " + ", ".join(notes)

    if not args.panels:
        rgb = canvas.rgb()
    if args.sheet:
        cols = args.cols or int(np.ceil(np.sqrt(rgb.shape[0])))
        render.save_png(args.sheet, render.contact_sheet(rgb, cols, gap=2, fill=255))
        print(f"{args.sheet}: {rgb.shape[0]} tiles of {rgb.shape[2]} x {rgb.shape[1]}, {cols} per row; {what}")
    else:
        os.makedirs(args.frames, exist_ok=True)
        host = rgb.cpu()
        for f in range(host.shape[0]):
            render.save_png(os.path.join(args.frames, f"frame_{f:04d}.png"), host[f])
        print(f"{args.frames}: {host.shape[0]} frames of {host.shape[2]} x {host.shape[1]}; {what}")
    env.close()


if __name__ == "__main__":
    main()
