"""The plot primitives, the panels and the full video frame on the device (mn_render_draw's RECT, MARKER, GLYPH and SECTOR; render_panels.py;
scripts/render_episodes.py --panels): the kernel against the host build of the same raster body, pixel word for pixel word -- EQUAL, nothing left
out --, the order independence of the atomic-max drawing over all seven kinds, and a real short IQN episode drawn as panels and as whole frames
without a copy to the host on the way.  The cases and the numpy twin are tests/test_render_panels_cpu.py's."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import test_render_cpu as H      # noqa: E402
import test_render_panels_cpu as P      # noqa: E402

pytestmark = pytest.mark.gpu

G = os.path.join(os.path.dirname(__file__), "golden")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def torch():
    import torch as t
    if not t.cuda.is_available():
        pytest.skip("no GPU")
    return t


@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    if not os.path.exists(H.HIPCC):
        pytest.skip("no hipcc")
    return H.build_host(tmp_path_factory.mktemp("render_host_panels_gpu"))


def _words(canvas):
    return canvas.pixels.cpu().numpy()


def _canvas(torch, n_images, width, height, view, fill):
    from distributional_rl_navigation_amd import render
    px = torch.full((n_images, height, width), fill, dtype=torch.int32, device="cuda:0").view(torch.uint32)
    return render.Canvas(px, view)


def _prims_tensor(torch, rec):
    return torch.from_numpy(np.frombuffer(rec.tobytes(), dtype=np.uint8).reshape(len(rec), 48).copy()).to("cuda:0")


@pytest.mark.parametrize("name", P.CASE_NAMES)
def test_new_kind_cases_equal_the_host_program(torch, host_program, tmp_path, name):
    prims = P.panel_cases()[name]
    want, _, _ = H.run_host(host_program, tmp_path, name, P.W, P.HGT, P.VIEW, n_images=P.IMAGES, prims=prims, fill=P.FILL)
    canvas = _canvas(torch, P.IMAGES, P.W, P.HGT, P.VIEW, P.FILL)
    got = _words(canvas.draw(_prims_tensor(torch, prims)))
    assert np.array_equal(got, want), np.argwhere(got != want)[:5]


def random_records(n, seed):
    """About `n` records of all seven kinds over 3 images of 80 x 48, most of them inside the picture, some across its edges."""
    from distributional_rl_navigation_amd import render
    rng = np.random.RandomState(seed)
    rec = np.zeros(n, dtype=render.PRIM_DTYPE)
    kind = rng.choice([0, 1, 2, 4, 5, 6, 7], size=n)
    rec["kind"] = kind
    rec["x0"], rec["y0"] = rng.uniform(-3.0, 43.0, n), rng.uniform(-3.0, 27.0, n)
    rec["x1"], rec["y1"] = rec["x0"] + rng.normal(0.0, 3.0, n), rec["y0"] + rng.normal(0.0, 3.0, n)      # SEGMENT, RECT, SECTOR: a second point
    disc, ring, marker, glyph = kind == 1, kind == 2, kind == 5, kind == 6
    rec["x1"][disc] = rng.uniform(0.0, 2.5, disc.sum())
    rec["x1"][ring], rec["y1"][ring] = rng.uniform(0.0, 1.5, ring.sum()), rng.uniform(1.5, 3.0, ring.sum())
    rec["x1"][marker], rec["y1"][marker] = rng.randint(0, 3, marker.sum()), rng.randint(0, 4, marker.sum())
    rec["x1"][glyph], rec["y1"][glyph] = rng.randint(-6, 7, glyph.sum()), rng.randint(-8, 9, glyph.sum())
    hw = rng.randint(0, 3, n)
    hw[marker] = rng.randint(0, 10, marker.sum())
    hw[glyph] = rng.randint(33, 127, glyph.sum()) | rng.randint(1, 4, glyph.sum()) << 8
    hw[kind == 7] = rng.randint(0, 32769, (kind == 7).sum())
    rec["half_width_px"] = hw
    rec["image_first"] = rng.randint(-1, 3, n)
    rec["image_last"] = rec["image_first"] + rng.randint(0, 3, n)
    rec["color_z"] = (rng.randint(1, 6, n).astype(np.int64) << 24 | rng.randint(0, 1 << 24, n)).astype(np.uint32)
    return rec


def test_random_records_of_all_kinds_in_any_order(torch, host_program, tmp_path):
    rec = random_records(2000, 23)
    assert all((rec["kind"] == k).sum() > 200 for k in (0, 1, 2, 4, 5, 6, 7))
    want, _, _ = H.run_host(host_program, tmp_path, "random", P.W, P.HGT, P.VIEW, n_images=P.IMAGES, prims=rec, fill=0)
    prims = _prims_tensor(torch, rec)
    rng = np.random.RandomState(5)
    out = []
    for perm in (np.arange(len(rec)), rng.permutation(len(rec)), rng.permutation(len(rec))):
        canvas = _canvas(torch, P.IMAGES, P.W, P.HGT, P.VIEW, 0)
        out.append(_words(canvas.draw(prims[torch.from_numpy(perm).to("cuda:0")].contiguous())))
    canvas = _canvas(torch, P.IMAGES, P.W, P.HGT, P.VIEW, 0)
    canvas.draw(prims[1100:].contiguous())
    out.append(_words(canvas.draw(prims[:1100].contiguous())))      # split over two launches, the second half first
    for k, got in enumerate(out):
        assert np.array_equal(got, want), (k, np.argwhere(got != want)[:5])
    assert (want != 0).mean() > 0.5      # a crowded canvas: most pixels were contested


# ---- a real short episode -----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def episode(torch):
    """World 0 of the evaluation config under the shipped IQN checkpoint, adaptive, for at most 12 steps: the traces of the launch, the replayed
    states, the observations of those states and the agent."""
    from distributional_rl_navigation_amd.iqn.agent import IQNAgent
    from distributional_rl_navigation_amd.iqn.fused_act import ActRng, rollout_iqn
    from distributional_rl_navigation_amd.marinenav_env.vec_env import VecMarineNavEnv
    with open(os.path.join(G, "eval_config_seed3.json")) as f:
        world = VecMarineNavEnv.world_from_eval_config(json.load(f)["env_0"])
    env = VecMarineNavEnv(1, device="cuda:0", precision="f64")
    env.load_worlds([world])
    agent = IQNAgent(26, 9, device="cuda:0", seed=0, BUFFER_SIZE=1024)
    agent.load_model(os.path.join(G, "pretrained_IQN_seed3"), "cuda:0")
    tr = rollout_iqn(agent.qnetwork_local, env, 12, ActRng(0, env.device), adaptive=True, trace=("done", "action", "traj", "cvar", "obs"), want_quantiles=True)
    assert tr is not None
    done = tr["done"][:, 0].bool()
    steps = int(done.to(torch.uint8).argmax()) + 1 if bool(done.any()) else 12
    start = np.array([[world["start"][0], world["start"][1], world["init_theta"], world["init_speed"]]])
    out = env.rollout_at(start, tr["action"][:steps, 0].clamp(min=0), env=0, trace=("state", "traj"), dtype=torch.float64)
    assert int(out["steps"][0]) == steps
    obs = env.observation_at(out["state_trace"][:steps, 0], env=0, velocity="given", dtype=torch.float64)
    yield dict(env=env, agent=agent, tr=tr, steps=steps, out=out, obs=obs, world=world)
    env.close()


def _twin_panel(prims_cpu, n_images, width, height, font):
    from distributional_rl_navigation_amd import render
    want = np.full((n_images, height, width), 0xFFFFFF, dtype=np.uint32)
    fragile = P.twin_draw(want, (0.0, 0.0, float(width), float(height)), render.prims_to_numpy(prims_cpu), font)
    return want, fragile


def test_return_dist_panel_equals_the_twin(torch, episode):
    """The device builder and the kernel against the builder on the host (torch on the CPU, fed with the copied-back quantiles) and the numpy twin of
    the raster rules.  Equal words; the twin's threshold-fragile RECT pixels (none expected) may be left out."""
    from distributional_rl_navigation_amd import render, render_panels
    T, env = episode["steps"], episode["env"]
    q, cv = episode["tr"]["quantiles"][:T, 0], episode["tr"]["cvar"][:T, 0]
    assert q.shape == (T, 32, 9) and bool(torch.isfinite(q).all())
    canvas = render_panels.return_dist_panel(q, cv, "adaptive phi = ", 160, 120, params=env.params)
    assert canvas.pixels.shape == (T, 120, 160) and canvas.pixels.is_cuda
    got = _words(canvas)
    want, fragile = _twin_panel(render_panels.return_dist_prims(q.cpu(), cv.cpu(), "adaptive phi = ", 160, 120, params=env.params), T, 160, 120, render.font())
    diff = got != want
    print(f"[return_dist {T} frames] {int(diff.sum())} words differ, {int(fragile.sum())} threshold-fragile; z seen {sorted(set((got >> 24).ravel().tolist()))}")
    assert fragile.reshape(T, -1).sum(axis=1).max() <= 4 and not (diff & ~fragile).any(), np.argwhere(diff & ~fragile)[:5]
    for z in (render_panels.Z_AXIS, render_panels.Z_MARK, render_panels.Z_TOP, render_panels.Z_TEXT):
        assert ((got >> 24) == z).any(axis=(1, 2)).all(), z      # baselines, crosses, the red bar and text in every frame
    assert ((got & 0xFFFFFF) == render_panels.RED).any(axis=(1, 2)).all()


def test_sonar_panel_equals_the_twin(torch, episode):
    from distributional_rl_navigation_amd import render, render_panels
    T, env, obs = episode["steps"], episode["env"], episode["obs"]
    half = float(env.params.sonar_angle) / 2
    got = _words(render_panels.sonar_panel(obs, float(env.params.sonar_range), half, 96, 80))
    want, fragile = _twin_panel(render_panels.sonar_prims(obs.cpu(), float(env.params.sonar_range), half, 96, 80), T, 96, 80, render.font())
    diff = got != want
    print(f"[sonar {T} frames] {int(diff.sum())} words differ, {int(fragile.sum())} threshold-fragile, {int(((got >> 24) == render_panels.Z_MARK).sum())} reflection pixels")
    assert fragile.reshape(T, -1).sum(axis=1).max() <= 4 and not (diff & ~fragile).any(), np.argwhere(diff & ~fragile)[:5]
    assert ((got >> 24) == render_panels.Z_TINT).any(axis=(1, 2)).all()      # the wedge is in every frame


class HostCopies:
    """Counts the ways a CUDA tensor reaches the host while it is active: .cpu(), .numpy(), .item(), .tolist(), .to(<cpu>), int() / float() / bool()."""
    NAMES = ("cpu", "numpy", "item", "tolist", "__int__", "__float__", "__bool__", "__index__")

    def __init__(self, torch):
        self.torch, self.count, self.saved = torch, 0, {}

    def __enter__(self):
        T = self.torch.Tensor
        for name in self.NAMES:
            orig = getattr(T, name)
            self.saved[name] = orig

            def stand_in(t, *a, _orig=orig, **kw):
                self.count += int(t.is_cuda)
                return _orig(t, *a, **kw)
            setattr(T, name, stand_in)
        orig_to = T.to
        self.saved["to"] = orig_to

        def to(t, *a, **kw):
            out = orig_to(t, *a, **kw)
            self.count += int(t.is_cuda and not out.is_cuda)
            return out
        T.to = to
        return self

    def __exit__(self, *exc):
        for name, orig in self.saved.items():
            setattr(self.torch.Tensor, name, orig)


def test_video_frames_of_the_episode(torch, episode):
    from distributional_rl_navigation_amd import maps, render, render_panels
    env, tr, T, out, obs = episode["env"], episode["tr"], episode["steps"], episode["out"], episode["obs"]
    fixed = maps.iqn_policy(episode["agent"], 1.0, quantiles=True)(tr["obs"][:T, 0].contiguous())["quantiles"]
    dist = [("adaptive phi = ", tr["cvar"][:T, 0], tr["quantiles"][:T, 0]), ("phi = ", 1.0, fixed)]
    before = env.save_state().clone()
    with HostCopies(torch) as copies:
        rgb, parts = render_panels.video_frames(env, 0, out["state_trace"], out["traj_trace"], obs, dist=dist, subtitle=("a short episode",), every=2, size=(240, 135),
                                                steps=T, start=episode["world"]["start"], return_parts=True)
        probe = torch.zeros(1, device="cuda:0")
    assert copies.count == 0, copies.count      # from the traces to the finished RGB tensor nothing went to the host
    with HostCopies(torch) as check:
        probe.cpu()
    assert check.count == 1      # ... and the stand-in does count
    assert torch.equal(before, env.save_state())      # byte for byte
    F = (T + 1) // 2
    assert rgb.shape == (F, 135, 240, 3) and rgb.dtype == torch.uint8 and rgb.is_cuda
    slots = render_panels.video_layout("iqn", (240, 135), 2)
    assert set(parts) == set(slots) == {"title", "goal", "sonar", "velocity", "map", "dist0", "dist1"}
    covered = torch.zeros(135, 240, dtype=torch.bool, device="cuda:0")
    for name, (canvas, slot) in parts.items():
        x, y, w, h = slot
        assert slot == slots[name] and canvas.pixels.shape == (F, h, w), name
        assert torch.equal(rgb[:, y:y + h, x:x + w], canvas.rgb()), name
        covered[y:y + h, x:x + w] = True
    assert bool((rgb[:, ~covered] == 255).all())      # what no part covers stays white
    # the parts are what the panel calls give on their own: the map is episode_frames, the panels are on the frames' rows with one shared axis
    rows = (torch.arange(F, device="cuda:0") * 2).clamp(max=T - 1)
    x, y, w, h = slots["map"]
    alone = render.episode_frames(env, 0, out["state_trace"], out["traj_trace"], every=2, steps=T, start=episode["world"]["start"], width=w)
    assert torch.equal(parts["map"][0].pixels.view(torch.int32), alone.pixels.view(torch.int32))
    lim = render_panels.shared_limits([tr["quantiles"][:T, 0][rows], fixed[rows]])
    x, y, w, h = slots["dist0"]
    alone = render_panels.return_dist_panel(tr["quantiles"][:T, 0][rows], tr["cvar"][:T, 0][rows], "adaptive phi = ", w, h, lim, labels=False, params=env.params)
    assert torch.equal(parts["dist0"][0].pixels.view(torch.int32), alone.pixels.view(torch.int32))
    x, y, w, h = slots["sonar"]
    alone = render_panels.sonar_panel(obs[rows], float(env.params.sonar_range), float(env.params.sonar_angle) / 2, w, h)
    assert torch.equal(parts["sonar"][0].pixels.view(torch.int32), alone.pixels.view(torch.int32))
    for name in parts:
        assert bool((parts[name][0].z() > 0).any()), name      # every part drew something


# ---- the script, in fresh processes -----------------------------------------------------------------------------------------------------------------
def _script(args, tmp_path):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "render_episodes.py"), "--eval-config", os.path.join(G, "eval_config_seed3.json")] + args,
                       capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-3000:]
    print(r.stdout)
    return r.stdout


def _frames_of(d):
    files = sorted(os.listdir(d))
    return files, [H.decode_png(open(os.path.join(d, f), "rb").read()) for f in files]


def test_script_panels_of_an_iqn_episode(torch, tmp_path):
    from distributional_rl_navigation_amd import render_panels
    common = ["--iqn", os.path.join(G, "pretrained_IQN_seed3"), "--adaptive", "--max-steps", "6", "--every", "2"]
    full, bare = str(tmp_path / "full"), str(tmp_path / "bare")
    text = _script(common + ["--panels", "--dist-cvars", "1.0", "--frames", full, "--width", "240"], tmp_path)
    x, y, w, h = render_panels.video_layout("iqn", (240, 135), 2)["map"]
    _script(common + ["--frames", bare, "--width", str(w)], tmp_path)
    files, imgs = _frames_of(full)
    assert files == [f"frame_{f:04d}.png" for f in range(3)] and "3 frames of 240 x 135" in text
    assert all(i.shape == (135, 240, 3) for i in imgs)
    files_bare, maps_alone = _frames_of(bare)
    assert files_bare == files and all(m.shape == (h, w, 3) for m in maps_alone)
    for i, m in zip(imgs, maps_alone):
        assert np.array_equal(i[y:y + h, x:x + w], m)      # the map of the full frame is the frame the script wrote without --panels
    slots = render_panels.video_layout("iqn", (240, 135), 2)
    for name in ("title", "goal", "sonar", "velocity", "dist0", "dist1"):
        sx, sy, sw, sh = slots[name]
        assert (imgs[0][sy:sy + sh, sx:sx + sw] != 255).any(), name
    assert not np.array_equal(imgs[0], imgs[2])


def test_script_panels_of_a_planner_episode(torch, tmp_path):
    from distributional_rl_navigation_amd import render_panels
    d = str(tmp_path / "apf")
    text = _script(["--planner", "APF", "--panels", "--max-steps", "6", "--every", "2", "--frames", d, "--width", "240"], tmp_path)
    files, imgs = _frames_of(d)
    assert len(files) == 3 and all(i.shape == (135, 240, 3) for i in imgs) and "3 frames of 240 x 135" in text
    sx, sy, sw, sh = render_panels.video_layout("planner", (240, 135))["action"]
    assert (imgs[0][sy:sy + sh, sx:sx + sw] == 0).all(axis=-1).any()      # black text in the action slot
