"""Pictures on the device (mn_render_worlds / mn_render_draw, render.py, scripts/render_episodes.py): the kernels against the host build of the same
raster body (tests/render_host.hip), pixel word for pixel word -- EQUAL, nothing left out: both are the same IEEE float64 and integer operations
with contraction off --, the mapping (ragged tiles, the stride loop, one world for all against an index per image, f64 and mixed handles), the order
independence of the atomic-max drawing, the refusals, the promise that nothing in the handle is written, and episode sheets / frames from real
traces.  The helpers (host program, worlds, styles, primitive cases) are tests/test_render_cpu.py's."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import test_render_cpu as H      # noqa: E402

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
    return H.build_host(tmp_path_factory.mktemp("render_host_gpu"))


def _device_worlds():
    from distributional_rl_navigation_amd.marinenav_env.vec_env import VecMarineNavEnv
    with open(os.path.join(G, "eval_config_seed3.json")) as f:
        cfg = json.load(f)
    return [VecMarineNavEnv.world_from_eval_config(cfg[f"env_{k}"]) for k in range(len(cfg))]


@pytest.fixture(scope="module")
def envs(torch):
    """The 30 evaluation worlds on an f64 and on a mixed handle."""
    from distributional_rl_navigation_amd.marinenav_env.vec_env import VecMarineNavEnv
    out = {}
    for precision in ("f64", "mixed"):
        env = VecMarineNavEnv(30, precision=precision)
        env.load_worlds(_device_worlds())
        out[precision] = env
    yield out
    for env in out.values():
        env.close()


@pytest.fixture(scope="module")
def worlds():
    return H.eval_worlds()


def _words(canvas):
    return canvas.pixels.cpu().numpy()


# ---- mn_render_worlds -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lic", (False, True), ids=("plain", "lic"))
@pytest.mark.parametrize("size", ((67, 45), (96, 64)), ids=("67x45", "96x64"))
def test_world_images_equal_the_host_program(torch, envs, worlds, host_program, tmp_path, size, lic):
    from distributional_rl_navigation_amd import render
    width, height = size
    style = H.cmp_style(lic)
    which = (0, 10, 29)
    want, _, _ = H.run_host(host_program, tmp_path, "w", width, height, H.WHOLE, style, [worlds[k] for k in which])
    idx = torch.tensor(which, dtype=torch.int32)
    got = _words(render.world_images(envs["f64"], idx, width=width, height=height, style=style))
    diff = got != want
    print(f"[{width}x{height} lic={lic}] {int(diff.sum())} of {diff.size} pixel words differ from the host program")
    assert got.shape == (3, height, width) and got.dtype == np.uint32
    assert not diff.any(), (np.argwhere(diff)[:5], got[diff][:5], want[diff][:5])
    # one world for all (env0) against an index per image, and the mixed handle: the same float64 master tables
    for i, k in enumerate(which):
        one = render.world_images(envs["f64"], k, width=width, height=height, style=style)
        assert one.pixels.shape == (1, height, width) and np.array_equal(_words(one)[0], want[i]), k
    assert np.array_equal(_words(render.world_images(envs["mixed"], idx, width=width, height=height, style=style)), want)
    assert np.array_equal(_words(render.world_images(envs["mixed"], 10, width=width, height=height, style=style))[0], want[1])


def test_default_view_and_height(torch, envs):
    from distributional_rl_navigation_amd import render
    c = render.world_images(envs["f64"], 3, width=40)
    assert c.view == (0.0, 0.0, 50.0, 50.0) and c.pixels.shape == (1, 40, 40)
    c = render.world_images(envs["f64"], 3, width=40, view=(10.0, 20.0, 30.0, 30.0))
    assert c.pixels.shape == (1, 20, 40)
    rgb, z = c.rgb(), c.z()
    assert rgb.shape == (1, 20, 40, 3) and rgb.dtype == torch.uint8 and rgb.is_cuda and z.shape == (1, 20, 40)
    w = c.pixels.view(torch.int32)
    assert torch.equal(rgb[..., 0].int() << 16 | rgb[..., 1].int() << 8 | rgb[..., 2].int() | z.int() << 24, w)


def test_stride_loop_equals_single_calls(torch, envs):
    """70 images of 16 x 16 are 280 tiles; a grid of 3 workgroups takes them in 94 rounds, each workgroup changing image on the way."""
    from distributional_rl_navigation_amd import render
    idx = torch.arange(70, dtype=torch.int32) % 30
    few = H.cmp_style(True, max_workgroups=3)
    got = _words(render.world_images(envs["f64"], idx, width=16, height=16, style=few))
    assert np.array_equal(got, _words(render.world_images(envs["f64"], idx, width=16, height=16, style=H.cmp_style(True))))
    for i in range(70):
        assert np.array_equal(got[i], _words(render.world_images(envs["f64"], int(idx[i]), width=16, height=16, style=H.cmp_style(True)))[0]), i


def test_bad_world_index_gives_an_outside_image(torch, envs, worlds, host_program, tmp_path):
    from distributional_rl_navigation_amd import render
    style = H.cmp_style(True)
    idx = torch.tensor([5, 30, -1, 7, 1 << 30], dtype=torch.int32)
    got = _words(render.world_images(envs["f64"], idx, width=67, height=45, style=style))      # returns: the call is MN_OK
    want, _, _ = H.run_host(host_program, tmp_path, "bad", 67, 45, H.WHOLE, style, [worlds[5], None, None, worlds[7], None])
    assert np.array_equal(got, want) and (got[1] == style.outside).all() and (got[2] == style.outside).all() and (got[4] == style.outside).all()


# ---- mn_render_draw -------------------------------------------------------------------------------------------------------------------------------
def _canvas(torch, n_images, width, height, view, fill):
    from distributional_rl_navigation_amd import render
    px = torch.full((n_images, height, width), fill, dtype=torch.int32, device="cuda:0").view(torch.uint32)
    return render.Canvas(px, view)


def _prims_tensor(torch, rec):
    return torch.from_numpy(np.frombuffer(rec.tobytes(), dtype=np.uint8).reshape(len(rec), 48).copy()).to("cuda:0")


@pytest.mark.parametrize("name", H.CASE_NAMES)
def test_primitive_cases_equal_the_host_program(torch, host_program, tmp_path, name):
    prims = H.prim_cases()[name]
    want, _, _ = H.run_host(host_program, tmp_path, name, H.PRIM_W, H.PRIM_H, H.PRIM_VIEW, n_images=H.PRIM_IMAGES, prims=prims, fill=H.FILL)
    canvas = _canvas(torch, H.PRIM_IMAGES, H.PRIM_W, H.PRIM_H, H.PRIM_VIEW, H.FILL)
    assert canvas.draw(_prims_tensor(torch, prims)) is canvas
    got = _words(canvas)
    assert np.array_equal(got, want), np.argwhere(got != want)[:5]


def test_random_segments_in_any_order(torch, host_program, tmp_path):
    from distributional_rl_navigation_amd import render
    rng = np.random.RandomState(11)
    n, images, width, height, view = 3000, 5, 96, 64, (0.0, 0.0, 48.0, 32.0)
    a = rng.uniform(-2.0, 50.0, size=(n, 2)) * [1.0, 32.0 / 48.0]
    b = a + rng.normal(0.0, 1.5, size=(n, 2))
    z, rgb = rng.randint(1, 6, size=n), rng.randint(0, 1 << 24, size=n)
    first = rng.randint(-1, images, size=n)
    last = first + rng.randint(0, 3, size=n)
    prims = render.segments(a, b, torch.from_numpy((z.astype(np.int64) << 24) | rgb), first, last, rng.randint(0, 3, size=n)).to("cuda:0")
    out = []
    for perm in (torch.arange(n), torch.from_numpy(rng.permutation(n)), torch.from_numpy(rng.permutation(n))):
        canvas = _canvas(torch, images, width, height, view, 0)
        out.append(_words(canvas.draw(prims[perm.to("cuda:0")].contiguous())))
    assert np.array_equal(out[0], out[1]) and np.array_equal(out[0], out[2])
    want, _, _ = H.run_host(host_program, tmp_path, "random", width, height, view, n_images=images, prims=prims, fill=0)
    assert np.array_equal(out[0], want) and (out[0] != 0).mean() > 0.2      # a crowded canvas: most drawn pixels were contested


def test_trail_frames_hold_their_segments(torch):
    """A trail of T segments, segment t into frames [t, F): frame f must equal an image that got exactly the segments t <= f."""
    from distributional_rl_navigation_amd import render
    T, F, width, height, view = 40, 40, 67, 45, (0.0, 0.0, 50.0, 50.0)
    s = np.linspace(0.0, 1.0, T + 1)
    pts = np.stack([5.0 + 40.0 * s, 25.0 + 15.0 * np.sin(7.0 * s)], axis=1)
    t = torch.arange(T, dtype=torch.int32)
    frames = _canvas(torch, F, width, height, view, 7).draw(render.polylines(pts, render.word(0xFF0000, 4), t, torch.full_like(t, F - 1), 1).to("cuda:0"))
    got = _words(frames)
    single = render.polylines(pts, render.word(0xFF0000, 4), 0, 0, 1)
    for f in (0, 1, 17, F - 1):
        want = _words(_canvas(torch, 1, width, height, view, 7).draw(single[:f + 1].to("cuda:0")))[0]
        assert np.array_equal(got[f], want), f
    drawn = (got != 7).sum(axis=(1, 2))
    assert (np.diff(drawn) >= 0).all() and drawn[0] > 0 and drawn[-1] > drawn[0]


def test_render_calls_write_nothing_into_the_handle(torch):
    from distributional_rl_navigation_amd import render
    from distributional_rl_navigation_amd.marinenav_env.vec_env import VecMarineNavEnv
    env = VecMarineNavEnv(96, precision="f64", seed=21)
    env.set_attrs(num_cores=6, num_obs=8, min_start_goal_dis=35.0)
    env.reset()
    for t in range(3):
        env.step(env.random_actions(2, t))
    before = env.save_state().clone()
    obs = env.obs.clone()
    rng = np.random.RandomState(3)
    for lic in (False, True):
        c = render.world_images(env, torch.from_numpy(rng.randint(-2, 98, size=9).astype(np.int32)), width=50, style=H.cmp_style(lic))
        c.draw(render.discs(rng.uniform(0, 50, size=(20, 2)), 2.0, render.word(0xFFFFFF, 9), 0, 8).to(env.device))
        render.world_images(env, 95, width=33, height=21, style=H.cmp_style(lic))
    assert torch.equal(before, env.save_state()) and torch.equal(obs, env.obs)      # byte for byte: pose, counters, tables, RNG rows, done queue
    env.close()


def test_host_visible_refusals(torch, envs):
    from distributional_rl_navigation_amd import _capi, render
    env = envs["f64"]
    L, h, s = env.L, env.h, env._stream()
    px = torch.zeros(2, 8, 8, dtype=torch.int32, device=env.device)
    p = lambda t: C.c_void_p(t.data_ptr())
    view = lambda *v: (C.c_double * 4)(*v)
    good_view = view(0.0, 0.0, 50.0, 50.0)
    idx = torch.zeros(2, dtype=torch.int32, device=env.device)

    def worlds(handle=h, index=None, env0=0, n=2, w=8, hh=8, v=good_view, pixels=p(px)):
        st = render.Style().to_c()
        return L.mn_render_worlds(handle, index, env0, n, w, hh, v, C.byref(st), pixels, s)

    def raw(**fields):
        st = render.Style().to_c()
        for k, val in fields.items():
            setattr(st, k, val)
        return L.mn_render_worlds(h, None, 0, 2, 8, 8, good_view, C.byref(st), p(px), s)

    assert worlds() == 0 and worlds(index=p(idx), env0=99) == 0
    assert worlds(handle=None) == -1
    assert L.mn_render_worlds(h, None, 0, 2, 8, 8, good_view, None, p(px), s) == -1      # style NULL
    assert worlds(pixels=None) == -1 and worlds(v=None) == -1
    assert worlds(n=0) == -1 and worlds(w=0) == -1 and worlds(hh=-3) == -1 and worlds(n=1 << 15, w=1 << 8, hh=1 << 8) == -1
    assert worlds(v=view(50.0, 0.0, 50.0, 50.0)) == -1 and worlds(v=view(0.0, 9.0, 50.0, 2.0)) == -1
    assert worlds(v=view(0.0, 0.0, float("inf"), 50.0)) == -1 and worlds(v=view(float("nan"), 0.0, 50.0, 50.0)) == -1
    assert raw(n_levels=0) == -1 and raw(n_levels=33) == -1 and raw(n_levels=32) == 0 and raw(n_levels=1) == 0
    assert raw(lic_steps=-1) == -1 and raw(lic_steps=65) == -1 and raw(lic_steps=64) == 0
    assert raw(lic_floor=256) == -1 and raw(max_workgroups=-1) == -1
    assert raw(v_max=0.0) == -1 and raw(v_max=-1.0) == -1 and raw(v_max=float("nan")) == -1
    assert worlds(env0=30) == -1 and worlds(env0=-1) == -1
    assert len(L.mn_last_error(h)) > 0
    prims = render.discs([[1.0, 1.0]], 1.0, 5).to(env.device)

    def draw(pixels=p(px), n=2, w=8, hh=8, v=good_view, pr=p(prims), count=1):
        return L.mn_render_draw(pixels, n, w, hh, v, pr, count, s)
    assert draw() == 0 and draw(pr=None, count=0) == 0
    assert draw(pixels=None) == -1 and draw(v=None) == -1 and draw(pr=None) == -1 and draw(count=-1) == -1
    assert draw(n=0) == -1 and draw(w=0) == -1 and draw(hh=0) == -1 and draw(n=1 << 15, w=1 << 8, hh=1 << 8) == -1
    assert draw(v=view(0.0, 0.0, 0.0, 50.0)) == -1 and draw(v=view(0.0, 0.0, 50.0, float("nan"))) == -1
    torch.cuda.synchronize()
    with pytest.raises(ValueError):
        render.world_images(env, 0, width=0)
    with pytest.raises(_capi.MarineNavHipError):
        render.world_images(env, 30, width=8)


# ---- episodes -------------------------------------------------------------------------------------------------------------------------------------
def _pixel_of(view, width, height, xy):
    """floor of the pixel coordinates of world points [.., 2]."""
    x0, y0, x1, y1 = view
    return np.floor((xy[..., 0] - x0) / ((x1 - x0) / width)).astype(np.int64), np.floor((y1 - xy[..., 1]) / ((y1 - y0) / height)).astype(np.int64)


def _near(mask_points, width, height, reach):
    """Pixels within `reach` (Chebyshev) of any of the pixel positions (c [m], r [m])."""
    c, r = mask_points
    out = np.zeros((height, width), bool)
    for cc, rr in zip(c, r):
        out[max(rr - reach, 0):rr + reach + 1, max(cc - reach, 0):cc + reach + 1] = True
    return out


def test_episode_sheet_from_a_planner_trace(torch):
    from distributional_rl_navigation_amd import render
    from distributional_rl_navigation_amd.marinenav_env.vec_env import VecMarineNavEnv
    env = VecMarineNavEnv(3, precision="f64")
    env.load_worlds(_device_worlds()[:3])
    tr = env.rollout_policy(60, "APF", trace=("done", "traj"))
    done = tr["done"].cpu().numpy().astype(bool)
    ran = np.where(done.any(axis=0), done.argmax(axis=0) + 1, 60)
    steps = np.minimum(ran, [60, 25, 0])      # env 1 is cut short by hand, env 2 draws nothing
    width, hw = 128, 1
    back = render.world_images(env, torch.arange(3, dtype=torch.int32), width=width, style=H.cmp_style(False))
    canvas = render.episode_sheet(env, tr["traj"], torch.from_numpy(steps), color=0xE8590C, canvas=back.clone(), half_width=hw)
    got, base = _words(canvas), _words(back)
    traj = tr["traj"].cpu().numpy()      # [T][n][N][2]
    trail = (got >> 24) == render.Z_TRAIL
    assert np.array_equal(got[~trail], base[~trail]) and (got[trail] == render.word(0xE8590C, render.Z_TRAIL)).all()
    for e in range(3):
        pts = traj[:steps[e], e].reshape(-1, 2)
        assert np.isfinite(pts).all()
        c, r = _pixel_of(canvas.view, width, width, pts)
        inside = (c >= 0) & (c < width) & (r >= 0) & (r < width)
        print(f"[sheet env {e}] {steps[e]} of {ran[e]} steps, {len(pts)} points, {int(trail[e].sum())} trail pixels")
        assert not (trail[e] & ~_near((c, r), width, width, hw + 1)).any()      # every drawn pixel lies within half_width + 1 pixels of a trace point
        assert trail[e][r[inside], c[inside]].all()                             # every trace point in front of steps[e] has its pixel
    assert trail[0].any() and trail[1].any() and not trail[2].any()
    # another trace over the same canvas: the per-pixel max decides, the first trail stays where the second does not cover it
    again = render.episode_sheet(env, tr["traj"], torch.from_numpy(np.array([0, 0, 10])), color=0xFFFFFF, canvas=canvas)
    assert again is canvas and np.array_equal(_words(canvas)[:2], got[:2]) and ((_words(canvas)[2] >> 24) == render.Z_TRAIL).any()
    env.close()


def test_episode_frames_from_a_stored_action_list(torch, envs):
    from distributional_rl_navigation_amd import render
    z = np.load(os.path.join(G, "g6_pretrained_replay.npz"))
    ep, T = 2, 12      # a short successful episode: the robot stays on the map
    k = int(z["greedy_ids"][ep][1])
    assert z["greedy_len"][ep] >= T
    env = envs["f64"]
    world = _device_worlds()[k]
    start = np.array([[world["start"][0], world["start"][1], world["init_theta"], world["init_speed"]]])
    out = env.rollout_at(start, z["greedy_actions"][ep][:T].astype(np.int32), env=k, trace=("state", "traj"), dtype=torch.float64)
    assert int(out["steps"][0]) == T
    width, hw = 128, 1
    style = H.cmp_style(False)
    view = (-10.0, -10.0, 60.0, 60.0)      # the map with a margin of 10: these episodes brush the map's edge
    back = render.world_images(env, k, width=width, view=view, style=style)
    frames = render.episode_frames(env, k, out["state_trace"], out["traj_trace"], beams=True, background=back, half_width=hw)
    got, base = _words(frames), _words(back)[0]
    assert got.shape == (T, width, width)
    states, traj = out["state_trace"][:, 0].cpu().numpy(), out["traj_trace"][:, 0].cpu().numpy()
    zz = got >> 24
    px = (view[2] - view[0]) / width
    assert frames.view == view and (states[:, :2] > -8.0).all() and (states[:, :2] < 58.0).all()      # every robot, with its heading tick, is inside the picture
    robot_r, sonar = float(env.params.robot_r), float(env.params.sonar_range)
    for t in range(T):
        c, r = _pixel_of(frames.view, width, width, states[t, :2])
        body = (zz[t] == render.Z_ROBOT)
        assert body[r, c]
        assert not (body & ~_near(([c], [r]), width, width, int(np.ceil(2 * robot_r / px)) + hw + 1)).any()      # disc and heading tick: around states[t]
        cc, rr = np.meshgrid(np.arange(width), np.arange(width), indexing="xy")
        dx, dy = (view[0] + (cc + 0.5) * px) - states[t, 0], (view[3] - (rr + 0.5) * px) - states[t, 1]
        assert body[dx * dx + dy * dy <= robot_r * robot_r].all()      # the disc rule, centred on states[t]
        beam = zz[t] == render.Z_BEAM
        assert not (beam & ~_near(([c], [r]), width, width, int(np.ceil(sonar / px)) + 2)).any()
        changed = got[t] != base
        assert np.array_equal(changed, zz[t] >= render.Z_BEAM)      # everything the frame adds lies above the background's layers
    # frame 0: one step of trail, the robot and its beams: away from the beams everything new is near the start
    c0, r0 = _pixel_of(frames.view, width, width, np.array(world["start"], dtype=np.float64))
    new0 = (got[0] != base) & (zz[0] != render.Z_BEAM)
    first_step = np.abs(traj[0] - np.array(world["start"])).max()      # how far the first step's sub-steps get from the start
    assert new0.any() and not (new0 & ~_near(([c0], [r0]), width, width, int(np.ceil((2 * robot_r + first_step) / px)) + hw + 2)).any()
    # the last frame's trail is the sheet's trail of the same trace (where the robot of the last frame does not cover it)
    sheet = render.episode_sheet(env, out["traj_trace"], torch.tensor([T]), canvas=back.clone(), half_width=hw)
    st = (_words(sheet)[0] >> 24) == render.Z_TRAIL
    last = zz[T - 1]
    open_px = last != render.Z_ROBOT
    assert np.array_equal((last == render.Z_TRAIL)[open_px], st[open_px]) and st.sum() > 0
    trail_growth = [(zz[t] == render.Z_TRAIL).sum() + (zz[t] == render.Z_ROBOT).sum() for t in range(T)]
    assert trail_growth[-1] > trail_growth[0]
    # no beams, every third step: 4 frames, no beam pixels
    few = render.episode_frames(env, k, out["state_trace"], out["traj_trace"], beams=False, every=3, background=back)
    assert few.pixels.shape == (4, width, width) and not ((_words(few) >> 24) == render.Z_BEAM).any()


# ---- the script, in fresh processes -----------------------------------------------------------------------------------------------------------------
def _script(args, tmp_path):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "render_episodes.py"), "--eval-config", os.path.join(G, "eval_config_seed3.json")] + args,
                       capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-3000:]
    print(r.stdout)
    return r.stdout


def test_script_writes_a_sheet(torch, tmp_path):
    out = str(tmp_path / "sheet.png")
    text = _script(["--planner", "APF", "--worlds", "0:2", "--sheet", out, "--width", "96", "--max-steps", "80"], tmp_path)
    img = H.decode_png(open(out, "rb").read())
    assert img.shape == (96, 2 * 96 + 2, 3) and "2 tiles of 96 x 96" in text      # two tiles side by side, a gap of 2
    assert (img[:, 96:98] == 255).all() and ((img[..., 0] == 0xE8) & (img[..., 1] == 0x59) & (img[..., 2] == 0x0C)).sum() > 20      # the gap; the trail's colour


def test_script_writes_frames_of_a_replay(torch, tmp_path):
    d = str(tmp_path / "frames")
    text = _script(["--replay", os.path.join(G, "g6_pretrained_replay.npz"), "--subset", "greedy", "--episode", "0", "--max-steps", "9", "--every", "2",
                    "--frames", d, "--width", "80"], tmp_path)
    files = sorted(os.listdir(d))
    assert files == [f"frame_{f:04d}.png" for f in range(5)] and "5 frames of 80 x 80" in text
    imgs = [H.decode_png(open(os.path.join(d, f), "rb").read()) for f in files]
    assert all(i.shape == (80, 80, 3) for i in imgs) and not np.array_equal(imgs[0], imgs[4])
