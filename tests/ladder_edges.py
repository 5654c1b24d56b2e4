"""Hand-built inputs for the decision every transition ends in: the termination ladder of MarineNavEnv.step (marinenav_env.py:240-257) -- out of
boundary > too long > collision > reach goal > normal -- with its thresholds, its ties and the rule that only the obstacle with the NEAREST CENTRE is tested
(tests/test_ladder_edges_cpu.py, tests/test_ladder_edges_gpu.py; the reference's answers: tests/golden/g20_ladder_edges.npz, made by
tests/golden/make_golden.py g20).

The robot of a STATIONARY case stands still: speed 0, action 4 (a = 0, w = 0), a world without vortex cores.  Every sub-step then adds +0.0 to x and y, so
the ladder is evaluated on the pose the case states (`pose_after`: the input, a -0.0 coordinate as +0.0 because (-0) + (+0) = +0 in IEEE 754 -- in the
reference's `self.x += dis[0]` as in the kernels' fma), dis_before - dis_after is exactly 0 and the reward is exactly timestep_penalty, + collision_penalty or
+ goal_reward, in float64 and in float32.  Nothing about a stationary case has a tolerance.

THE REFERENCE OF THESE CASES IS `relations()`: exact rational arithmetic (fractions.Fraction) on the float values of a case --
  collide  <=>  no > 0  and  d2(nearest centre) <= thr^2,  thr the FLOAT sum r + robot_r, the nearest centre the first in generation order among the
                centres of least d2 (the project's rule; the reference asks scipy's KD-tree, whose answer on an exact tie is an accident of its build),
  goal     <=>  |p - goal|^2 <= goal_dis^2,
  out      <=>  x < 0 or x > width or y < 0 or y > height,
  long     <=>  episode_timesteps >= max_episode_steps,
and `expected()` is the first true rung.  It depends on no reference project, oracle or kernel.  A float evaluation (sqrt(dx^2 + dy^2) <= thr, as the
reference, the oracle and the query kernels write it; d2 <= thr^2 with a sqrt only next to the threshold, as the step kernel does) must give these truth
values, and `relations()` asserts of every case that it can: a compared pair is either (a) on an axis with an exact difference, where sqrt(fl(d^2)) = |d|
exactly (a correctly rounded sqrt undoes a correctly rounded square), (b) built from differences and squares that are all exact (Pythagorean offsets), or
(c) apart by more than 2^-30 relative.
  ONE FAMILY OF CASES IS BUILT WHERE THE TWO PART ("collision" cases with `rounded`): d2 is an exactly representable sum of two exact squares just ABOVE
thr^2 -- in exact arithmetic the robot is clear -- but below (thr + ulp(thr) / 2)^2, so the correctly rounded square root IS thr and the reference's
`d <= r + robot.r` holds.  There the expectation is the reference's own definition, RN(sqrt(d2)) <= thr, evaluated exactly as d2 < (thr + ulp / 2)^2;
every float form of d2 (with or without fma, the KD-tree's) gives the same d2 because no term rounds.  These are the inputs the step kernel's square
root inside its 2^-48 band exists for: the squared comparison alone calls them clear.  (The converse does not exist: if the squared comparison holds,
so does the rounded one.)

MIXED PRECISION reads obstacle centres as 2^-24 m fixed point and radii as float32: a case is `mixed_ok` iff its centres are multiples of 2^-24 and its
radii float32 values (computed from the case, never declared), and on such a case the mixed kernel owes the same info, done and reward as float64.

Groups: "goal", "collision" (the threshold; `band` says whether the step kernel's 2^-48 band around thr^2 holds the case), "nearest" (with the `by d2`
cases: two centres whose d2 differ by an ulp while their square roots round to one double -- the nearer one is the nearest), "tie", "priority",
"clock", "boundary", "moving" (speed 2 along +x: the only cases with a tolerance, and the only ones whose expectation rests on a predicted pose --
`predict_pose`, asserted to end at least 1e-3 clear of every threshold).  A case belongs to one PARAMETER SET (`PSETS`: a handle has one mn_params);
the device tests run one batch per set, the set's cases repeated cyclically to N_ENVS."""
import os
import sys
from fractions import Fraction as Fr

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import params_sets as PS      # noqa: E402

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURE = os.path.join(GOLD, "g20_ladder_edges.npz")
N_ENVS = 2117                     # 33 x 64 + 5: a ragged last tile; finished envs in every one of the 32 done-queue shards, shard 0 twice
NORMAL, OUT, TOO_LONG, COLLISION, GOAL = 0, 1, 2, 3, 4      # MN_INFO_* (include/marinenav_hip.h) = INFO_CODE of make_golden.py
MAXO = 10
GROUPS = ("goal", "collision", "nearest", "tie", "priority", "clock", "boundary", "moving")
FIX = 2.0 ** 24

# mn_default_params (tests/test_ladder_edges_cpu.py holds this copy to the library's): what the ladder and the stationary robot depend on
DEFAULTS = dict(width=50.0, height=50.0, goal_dis=2.0, robot_r=0.8, set_boundary=0, max_episode_steps=1000, timestep_penalty=-1.0, collision_penalty=-50.0,
                goal_reward=100.0, dt=0.1, N=10, max_speed=2.0)
assert PS.STEP_SETS[3][0] == "S4"
PSETS = [
    ("D0", {}),                                      # the defaults: no boundary
    ("D1", dict(set_boundary=1)),
    ("S4", dict(PS.STEP_SETS[3][1])),                # goal_dis 4, other penalties, boundary on a 60 x 36 map
    ("G5", dict(goal_dis=5.0)),                      # 3-4-5
    ("M0", dict(max_episode_steps=0)),               # the reference (and the CPU twin) cannot express these two: 1000 is written into its ladder
    ("M1", dict(max_episode_steps=1)),
    ("R75", dict(robot_r=0.75, set_boundary=1)),     # a dyadic robot radius: thr = r + robot_r lands on the fixed-point grid
]
PSET_NAMES = [n for n, _ in PSETS]


def pset_spec(name):
    return dict(PSETS[PSET_NAMES.index(name)][1])


def pset_params(name):
    """DEFAULTS overlaid with the set."""
    p = dict(DEFAULTS)
    p.update({k: v for k, v in pset_spec(name).items() if k in DEFAULTS})
    return p


class Case:
    __slots__ = ("name", "group", "pset", "obstacles", "goal", "pose", "ep_t", "tot_t", "action", "stationary", "tie", "band", "rounded")

    def __init__(self, **kw):
        for k, v in kw.items():
            setattr(self, k, v)

    @property
    def mixed_ok(self):
        return all(float(c * FIX) == np.floor(c * FIX) and abs(c) < 128.0 for o in self.obstacles for c in o[:2]) and \
            all(float(np.float32(o[2])) == o[2] for o in self.obstacles)


# ---- exact arithmetic ----------------------------------------------------------------------------------------------------------------------------------
def _fr(v):
    return Fr(float(v))


def _exact_diff(a, b):
    return _fr(float(a) - float(b)) == _fr(a) - _fr(b)


def _decided(name, what, px, py, cx, cy, thr):
    """d2 = |c - p|^2 against thr^2, exactly: -1 below, 0 equal, +1 above -- with the assertion that every float form of the test gives that answer
    (module docstring (a), (b), (c))."""
    d2, t2 = (_fr(cx) - _fr(px)) ** 2 + (_fr(cy) - _fr(py)) ** 2, _fr(thr) ** 2
    sign = (d2 > t2) - (d2 < t2)
    dx, dy = float(cx) - float(px), float(cy) - float(py)
    on_axis = (dx == 0.0 or dy == 0.0) and _exact_diff(cx, px) and _exact_diff(cy, py)
    all_exact = _exact_diff(cx, px) and _exact_diff(cy, py) and _fr(dx * dx) == _fr(dx) ** 2 and _fr(dy * dy) == _fr(dy) ** 2 and _fr(dx * dx + dy * dy) == d2 \
        and (float(np.sqrt(dx * dx + dy * dy)) > thr) - (float(np.sqrt(dx * dx + dy * dy)) < thr) == sign      # ... and the rounded root on the same side
    apart = t2 > 0 and abs(d2 - t2) > t2 * Fr(1, 2 ** 30)
    assert on_axis or all_exact or apart or (t2 == 0 and d2 > 0), (name, what, "a float evaluation of this comparison is not pinned by exact arithmetic")
    return sign


def _rounded_collide(name, px, py, cx, cy, thr):
    """The reference's float test RN(sqrt(d2)) <= thr on a d2 that no float form can round, decided exactly; asserts the case is one where exact
    arithmetic (d2 > thr^2: clear) and the squared float comparison (d2 > fl(thr^2): clear) both part from it (module docstring)."""
    dx, dy = float(cx) - float(px), float(cy) - float(py)
    d2 = _fr(dx) ** 2 + _fr(dy) ** 2
    assert _exact_diff(cx, px) and _exact_diff(cy, py) and _fr(dx * dx) == _fr(dx) ** 2 and _fr(dy * dy) == _fr(dy) ** 2 and _fr(dx * dx + dy * dy) == d2, name
    half = _fr(thr) + _fr(np.spacing(thr)) / 2
    assert _fr(thr) ** 2 < d2 < half ** 2 and dx * dx + dy * dy > thr * thr and float(np.sqrt(dx * dx + dy * dy)) == thr, name
    return True


def nearest(name, obstacles, px, py):
    """Index of the first obstacle in generation order among the centres of least exact d2, and whether another centre ties with it; asserts that a float
    d2 orders the centres the same way (a tie: every term exact; otherwise more than 2^-30 apart, or told apart by every float form of d2)."""
    d2 = [(_fr(ox) - _fr(px)) ** 2 + (_fr(oy) - _fr(py)) ** 2 for ox, oy, _ in obstacles]
    k = min(range(len(d2)), key=lambda i: (d2[i], i))
    tied = False
    for i, (ox, oy, _) in enumerate(obstacles):
        if i == k:
            continue
        if d2[i] == d2[k]:
            tied = True
            for j in (i, k):
                dx, dy = float(obstacles[j][0]) - float(px), float(obstacles[j][1]) - float(py)
                assert _exact_diff(obstacles[j][0], px) and _exact_diff(obstacles[j][1], py) and _fr(dx * dx) == _fr(dx) ** 2 and _fr(dy * dy) == _fr(dy) ** 2 \
                    and _fr(dx * dx + dy * dy) == d2[j], (name, "a tie whose float d2 is not exact")
        elif not d2[i] > d2[k] * (1 + Fr(1, 2 ** 30)):
            # nearly equally near ("nearest" cases `by d2`): pinned if the float d2 of the two are ordered like the exact ones whichever way they are
            # formed -- the differences and both squares exact, so fma(dx, dx, dy * dy) and dx * dx + dy * dy are the same single rounding of the exact sum
            f = []
            for j in (i, k):
                dx, dy = float(obstacles[j][0]) - float(px), float(obstacles[j][1]) - float(py)
                assert _exact_diff(obstacles[j][0], px) and _exact_diff(obstacles[j][1], py) and _fr(dx * dx) == _fr(dx) ** 2 and _fr(dy * dy) == _fr(dy) ** 2, name
                f.append(dx * dx + dy * dy)
            assert f[0] > f[1], (name, "two centres nearly equally near whose float d2 do not tell them apart")
    return k, tied


def predict_pose(case):
    """Where the sub-steps of a case without current leave the robot: robot.py:102-123 in plain float64 (the input +0.0 for a stationary case)."""
    p = pset_params(case.pset)
    x, y, theta, speed = (float(v) for v in case.pose)
    if case.stationary:
        return x + 0.0, y + 0.0, theta, speed
    assert case.action == 4 and theta == 0.0
    k = 0.4 / p["max_speed"]
    for _ in range(p["N"]):
        x += speed * np.cos(theta) * p["dt"]
        y += speed * np.sin(theta) * p["dt"]
        speed = min(max(speed + (0.0 - k * speed) * p["dt"], 0.0), p["max_speed"])
    return x, y, theta, speed


def relations(case):
    """dict(out, long, collide, goal: bool; nearest: index or -1; tied: bool; band: the step kernel's band test on the float values) -- see the module docstring."""
    p = pset_params(case.pset)
    x, y, _, _ = predict_pose(case)
    if not case.stationary:      # a predicted pose: every threshold at least 1e-3 away, whatever the last bits of the integration
        lo = []
        for ox, oy, r in case.obstacles:
            lo.append(abs(np.hypot(ox - x, oy - y) - (r + p["robot_r"])))
        lo.append(abs(np.hypot(case.goal[0] - x, case.goal[1] - y) - p["goal_dis"]))
        lo += [abs(x), abs(x - p["width"]), abs(y), abs(y - p["height"])]
        assert min(lo) >= 1e-3, (case.name, min(lo))
    out = x < 0.0 or x > p["width"] or y < 0.0 or y > p["height"]
    assert out == (_fr(x) < 0 or _fr(x) - _fr(p["width"]) > 0 or _fr(y) < 0 or _fr(y) - _fr(p["height"]) > 0)
    rel = dict(out=bool(out), long=case.ep_t >= p["max_episode_steps"], nearest=-1, tied=False, band=False)
    rel["collide"] = False
    if case.obstacles:
        k, tied = nearest(case.name, case.obstacles, x, y)
        ox, oy, r = case.obstacles[k]
        thr = float(r) + float(p["robot_r"])
        if case.rounded:
            rel["collide"] = _rounded_collide(case.name, x, y, ox, oy, thr)
        else:
            rel["collide"] = _decided(case.name, "collision", x, y, ox, oy, thr) <= 0
        rel["nearest"], rel["tied"] = k, tied
        dx, dy = float(ox) - x, float(oy) - y
        d2f, t2f = dx * dx + dy * dy, thr * thr
        rel["band"] = bool(abs(d2f - t2f) <= t2f * 2.0 ** -48)
    rel["goal"] = _decided(case.name, "goal", x, y, case.goal[0], case.goal[1], p["goal_dis"]) <= 0
    return rel


def ladder(p, rel):
    """The first true rung, and the reward a stationary robot collects with it."""
    if p["set_boundary"] and rel["out"]:
        return OUT, p["timestep_penalty"]
    if rel["long"]:
        return TOO_LONG, p["timestep_penalty"]
    if rel["collide"]:
        return COLLISION, p["timestep_penalty"] + p["collision_penalty"]
    if rel["goal"]:
        return GOAL, p["timestep_penalty"] + p["goal_reward"]
    return NORMAL, p["timestep_penalty"]


# ---- the table -----------------------------------------------------------------------------------------------------------------------------------------
FAR = [(5.0, 5.0, 1.0), (45.0, 5.0, 1.0), (5.0, 45.0, 1.0), (45.0, 45.0, 1.0), (25.0, 5.0, 1.0), (25.0, 45.0, 1.0), (5.0, 25.0, 1.0), (45.0, 25.0, 1.0),
       (8.0, 8.0, 1.0), (42.0, 8.0, 1.0)]      # all at 20 m or more from (25, 25), clear of it
NO_GOAL = (45.0, 45.5)            # far from every pose used below
UP = np.inf


def _build():
    t = []

    def add(group, name, pset, obstacles=(), goal=NO_GOAL, pose=(25.0, 25.0, 0.0, 0.0), ep_t=0, action=4, stationary=True):
        obstacles = [tuple(float(v) for v in o) for o in obstacles]
        assert len(obstacles) <= MAXO and group in GROUPS and pset in PSET_NAMES
        assert (not stationary) or (pose[3] == 0.0 and action == 4 and 0.0 <= pose[2] < 2 * np.pi)
        c = Case(name=f"{group}/{pset}/{name}", group=group, pset=pset, obstacles=obstacles, goal=(float(goal[0]), float(goal[1])),
                 pose=tuple(float(v) for v in pose), ep_t=int(ep_t), tot_t=7 + 3 * len(t), action=int(action), stationary=bool(stationary), tie=False, band=False, rounded=False)
        t.append(c)
        return c

    def na(v, to):
        return float(np.nextafter(v, to))

    # -- goal threshold (<=).  The robot sits at coordinate 0 of the axis, so goal - p is the distance itself
    for pset in ("D0", "S4", "G5"):
        g = pset_params(pset)["goal_dis"]
        for axis in (0, 1):
            for tag, d in (("exactly", g), ("one ulp inside", na(g, 0.0)), ("one ulp outside", na(g, UP)), ("-exactly", -g), ("-one ulp outside", -na(g, UP))):
                pose, goal = ((0.0, 20.0, 0.0, 0.0), (d, 20.0)) if axis == 0 else ((20.0, 0.0, 1.25, 0.0), (20.0, d))
                add("goal", f"{'xy'[axis]} axis, {tag} goal_dis", pset, goal=goal, pose=pose)
    for tag, goal in (("(3, 4): exactly 5", (13.0, 14.0)), ("(-4, 3): exactly 5", (6.0, 13.0)), ("(3, 4.001): outside", (13.0, 14.001)), ("(3, 3.999): inside", (13.0, 13.999))):
        add("goal", tag, "G5", goal=goal, pose=(10.0, 10.0, 0.5, 0.0))
    add("goal", "(1.5, 2): 2.5, outside", "D0", goal=(11.5, 12.0), pose=(10.0, 10.0, 0.0, 0.0))
    add("goal", "(0, 0): on the goal", "D0", goal=(10.0, 10.0), pose=(10.0, 10.0, 0.0, 0.0))

    # -- collision threshold: sqrt(d2) <= r + robot_r.  Per radius, side by side in the batch (one wavefront): three cases inside the step kernel's
    # 2^-48 band around thr^2 and two just outside it, which the squared comparison alone decides
    rng = np.random.RandomState(20)
    radii = np.concatenate([[1.0, 3.0], rng.uniform(1.0, 3.0, 62)])
    for i, r in enumerate(radii):
        thr = float(r) + 0.8
        for tag, d, band in (("below", na(thr, 0.0), True), ("at", thr, True), ("above", na(thr, UP), True), ("1 - 2^-40", thr * (1 - 2.0 ** -40), False),
                             ("1 + 2^-40", thr * (1 + 2.0 ** -40), False)):
            c = add("collision", f"r[{i}] {tag}", "D0", obstacles=[(d, 25.0, r)] if i % 2 == 0 else [(25.0, d, r)],
                    pose=(0.0, 25.0, 0.0, 0.0) if i % 2 == 0 else (25.0, 0.0, 2.0, 0.0))
            c.band = band
    # ... on the mixed kernel's grid: the two fixed-point centres that bracket thr (float32 radii)
    for i, r in enumerate(np.float32(rng.uniform(1.0, 3.0, 32))):
        thr = float(r) + 0.8
        lo, hi = float(np.floor(thr * FIX) / FIX), float(np.ceil(thr * FIX) / FIX)
        assert lo < thr < hi
        for tag, d in (("grid point below", lo), ("grid point above", hi)):
            add("collision", f"r32[{i}] {tag}", "D0", obstacles=[(d, 25.0, float(r))] if i % 2 == 0 else [(25.0, d, float(r))],
                pose=(0.0, 25.0, 0.0, 0.0) if i % 2 == 0 else (25.0, 0.0, 2.0, 0.0))
    # ... and with a dyadic robot radius, where thr itself is a grid point: ON the threshold (inside the band) in both precisions, robot in mid-map
    for i, r in enumerate(np.round(rng.uniform(1.0, 3.0, 16) * 2.0 ** 22) / 2.0 ** 22):
        thr = float(r) + 0.75
        for tag, d, band in (("at", thr, True), ("one grid step below", thr - 1 / FIX, False), ("one grid step above", thr + 1 / FIX, False)):
            c = add("collision", f"r22[{i}] {tag}", "R75", obstacles=[(16.0 + d, 24.0, r)] if i % 2 == 0 else [(16.0, 24.0 - d, r)], pose=(16.0, 24.0, 0.0, 0.0))
            c.band = band

    # ... and where the rounded square root decides (`rounded`, module docstring): off-axis centres on the 2^-24 grid, thr = RN(sqrt(d2)) = r + 0.75 exactly,
    # each beside the same centre with thr one ulp smaller (clear in every arithmetic), one ulp larger, and far outside the band
    made = 0
    while made < 24:
        ang, d = rng.uniform(0.0, 2 * np.pi), rng.uniform(1.8, 3.7)
        dx, dy = float(np.round(d * np.cos(ang) * FIX) / FIX), float(np.round(d * np.sin(ang) * FIX) / FIX)
        d2 = dx * dx + dy * dy
        thr = float(np.sqrt(d2))
        r = thr - 0.75
        if not (_fr(d2) == _fr(dx) ** 2 + _fr(dy) ** 2 and _fr(d2) > _fr(thr) ** 2 and d2 > thr * thr and _fr(r) + Fr(3, 4) == _fr(thr) and r + 0.75 == thr):
            continue
        c = add("collision", f"rounded[{made}] sqrt(d2) rounds onto thr", "R75", obstacles=[(16.0 + dx, 24.0 + dy, r)], pose=(16.0, 24.0, 0.0, 0.0))
        c.band, c.rounded = True, True
        for tag, th in (("thr one ulp smaller", na(thr, 0.0)), ("thr one ulp larger", na(thr, UP))):
            assert (th - 0.75) + 0.75 == th and _fr(th - 0.75) + Fr(3, 4) == _fr(th)
            add("collision", f"rounded[{made}] {tag}", "R75", obstacles=[(16.0 + dx, 24.0 + dy, th - 0.75)], pose=(16.0, 24.0, 0.0, 0.0)).band = True
        add("collision", f"rounded[{made}] thr smaller by 2^-40", "R75", obstacles=[(16.0 + dx, 24.0 + dy, r * (1 - 2.0 ** -40))], pose=(16.0, 24.0, 0.0, 0.0))
        made += 1

    # -- only the nearest centre is tested
    small_clear, big_overlap = (27.5, 25.0, 1.0), (25.0, 28.5, 3.0)        # 2.5 > 1.8 ; 3.5 <= 3.8
    near_overlap, far_clear = (27.0, 25.0, 1.5), (25.0, 31.0, 1.0)         # 2 <= 2.3 ; 6 > 1.8
    add("nearest", "small nearest clear, larger farther overlaps", "D0", obstacles=[small_clear, big_overlap])
    add("nearest", "larger farther overlaps, small nearest clear", "D0", obstacles=[big_overlap, small_clear])
    add("nearest", "nearest overlaps, farther clear", "D0", obstacles=[near_overlap, far_clear])
    add("nearest", "farther clear, nearest overlaps", "D0", obstacles=[far_clear, near_overlap])
    for k in range(MAXO):
        tab = list(FAR[:9])
        tab.insert(k, near_overlap)
        add("nearest", f"nearest (overlapping) in slot {k} of 10", "D0", obstacles=tab)
        tab = list(FAR[:8])
        tab.insert(k, small_clear)
        tab.insert((k + 5) % MAXO, big_overlap)
        add("nearest", f"nearest (clear) in slot {tab.index(small_clear)} of 10, an overlapping one farther away in slot {tab.index(big_overlap)}", "D0", obstacles=tab)
    for pset in ("D0", "D1"):
        add("nearest", "no obstacle, robot where a zero-padded row would put one", pset, pose=(0.0, 0.0, 0.0, 0.0))
        add("nearest", "two far obstacles, robot where a zero-padded row would put one", pset, obstacles=FAR[3:5], pose=(0.0, 0.0, 0.0, 0.0))
    add("nearest", "no obstacle, robot in mid-map", "D0")
    # ... the nearest by d2, not by the rounded distance (`by d2`): two centres whose float d2 differ by one ulp and whose square roots round to the SAME
    # double.  The nearer one is the nearest -- the reference's KD-tree compares squared distances --, although a scan over sqrt(d2) sees a tie
    made = 0
    while made < 8:
        dx = float(np.round(rng.uniform(2.2, 3.0) * FIX) / FIX)
        u = float(np.spacing(dx * dx))
        dy1, dy2 = (float(np.round(np.sqrt(k * u) * 2.0 ** 40) / 2.0 ** 40) for k in (2.0, 1.0))      # dy^2 = 2 and 1 ulp of dx^2
        D1, D2 = dx * dx + dy1 * dy1, dx * dx + dy2 * dy2
        if not (_fr(dx * dx) == _fr(dx) ** 2 and D1 > D2 and float(np.sqrt(D1)) == float(np.sqrt(D2))):
            continue
        far, near = (16.0 + dx, 24.0 + dy1), (16.0 - dx, 24.0 + dy2)
        for tag, tab in (("farther clear first, nearer overlapping second", [far + (1.0,), near + (2.5,)]), ("farther overlapping first, nearer clear second", [far + (2.5,), near + (1.0,)]),
                         ("nearer overlapping first, farther clear second", [near + (2.5,), far + (1.0,)]), ("nearer clear first, farther overlapping second", [near + (1.0,), far + (2.5,)])):
            add("nearest", f"by d2[{made}] {tag}", "R75", obstacles=tab, pose=(16.0, 24.0, 0.0, 0.0))
        made += 1

    # -- ties: equal d2, the first in generation order decides
    A, B, C3 = (22.0, 25.0, 1.0), (28.0, 25.0, 2.5), (25.0, 28.0, 1.25)     # all 3 m away: A and C3 clear (1.8, 2.05), B overlaps (3.3)
    P34, P50 = (28.0, 29.0, 1.0), (30.0, 25.0, 4.5)                           # (3, 4) and (5, 0): 5 m both; clear (1.8), overlapping (5.3)
    for order in ((A, B), (B, A), (A, B, C3), (B, A, C3), (C3, A, B), (C3, B, A), (A, C3, B), (B, C3, A), (P34, P50), (P50, P34)):
        names = {A: "A", B: "B", C3: "C", P34: "(3,4)", P50: "(5,0)"}
        add("tie", "table " + " ".join(names[o] for o in order), "D0", obstacles=list(order)).tie = True
    for i, j in ((0, 1), (0, 2), (0, 4), (0, 8), (3, 9), (1, 9)):      # same lane / different lanes of the group for L = 2, 4, 8, 16
        for first, second in ((A, B), (B, A), (P34, P50), (P50, P34)):
            tab = list(FAR[:8])
            tab.insert(i, first)
            tab.insert(j, second)
            assert tab[i] == first and tab[j] == second
            names = {A: "A", B: "B", P34: "(3,4)", P50: "(5,0)"}
            add("tie", f"{names[first]} in slot {i}, {names[second]} in slot {j} of 10", "D0", obstacles=tab).tie = True
    add("tie", "B in slot 9, A in slot 2, C in slot 5 of 10", "D0", obstacles=FAR[:2] + [A] + FAR[2:4] + [C3] + FAR[4:7] + [B]).tie = True
    add("tie", "B in slot 2, A in slot 9, C in slot 5 of 10", "D0", obstacles=FAR[:2] + [B] + FAR[2:4] + [C3] + FAR[4:7] + [A]).tie = True

    # -- priority: every combination of the four rungs, boundary off and on
    for pset, inside, outside in (("D0", (10.0, 25.0), (-1.0, 25.0)), ("D1", (10.0, 25.0), (-1.0, 25.0)), ("S4", (40.0, 20.0), (40.0, 40.0))):
        g = pset_params(pset)["goal_dis"]
        for bits in range(16):
            o, lg, co, go = bits >> 3 & 1, bits >> 2 & 1, bits >> 1 & 1, bits & 1
            x, y = outside if o else inside
            add("priority", f"out {o} long {lg} collide {co} goal {go}", pset, obstacles=[(x + 3.0, y, 2.5 if co else 1.0)],
                goal=(x, y + g - 1.0) if go else (x, y - 15.0), pose=(x, y, 0.0, 0.0), ep_t=1000 if lg else 5)

    # -- the episode clock
    for pset, clocks in (("D0", (999, 1000, 1001, 2 ** 31 - 2)), ("M0", (0, 1)), ("M1", (0, 1, 2))):
        for ep in clocks:
            add("clock", f"ep_t {ep}", pset, ep_t=ep)
            add("clock", f"ep_t {ep}, goal and collision hold too", pset, obstacles=[(27.0, 25.0, 1.5)], goal=(25.0, 26.0), ep_t=ep)
    add("clock", "ep_t 0", "D0")

    # -- boundary: strict < and >
    for pset in ("D1", "D0", "R75"):
        for axis in (0, 1):
            for v in (0.0, -0.0, -5e-324, 50.0, na(50.0, UP), 5e-324, na(50.0, 0.0)):
                add("boundary", f"{'xy'[axis]} = {v!r}", pset, pose=(v, 25.0, 0.0, 0.0) if axis == 0 else (25.0, v, 0.0, 0.0))
    for x, y in ((40.0, 20.0), (20.0, 40.0), (60.0, 20.0), (na(60.0, UP), 20.0), (20.0, 36.0), (20.0, na(36.0, UP)), (-5e-324, 20.0), (20.0, -5e-324),
                 (-0.0, -0.0), (60.0, 36.0)):
        add("boundary", f"60 x 36 map, ({x!r}, {y!r})", "S4", pose=(x, y, 0.0, 0.0), goal=(30.0, 5.0))

    # -- moving: speed 2 along +x for one step (1.81 m), no current: the ladder reads the pose AFTER the sub-steps
    mv = (10.0, 25.0, 0.0, 2.0)
    add("moving", "into the goal radius", "D0", goal=(13.5, 25.0), pose=mv, stationary=False)
    add("moving", "out of the goal radius", "D0", goal=(9.0, 25.0), pose=mv, stationary=False)
    add("moving", "into an obstacle", "D0", obstacles=[(13.25, 25.0, 1.0)], pose=mv, stationary=False)
    add("moving", "into an obstacle inside the goal radius", "D0", obstacles=[(13.25, 25.0, 1.0)], goal=(13.5, 25.0), pose=mv, stationary=False)
    add("moving", "past an obstacle that was overlapping", "D0", obstacles=[(9.0, 25.0, 1.0)], pose=mv, stationary=False)
    add("moving", "across the right edge", "D1", pose=(49.0, 25.0, 0.0, 2.0), stationary=False)
    add("moving", "in from beyond the left edge", "D1", pose=(-1.0, 25.0, 0.0, 2.0), stationary=False)
    add("moving", "nowhere near anything", "D0", pose=mv, stationary=False)
    return t


_TABLE = None


def table():
    """The cases, built once; every case checked by `relations()` and against what its group says it is."""
    global _TABLE
    if _TABLE is None:
        t = _build()
        assert len({c.name for c in t}) == len(t)
        for c in t:
            rel = relations(c)
            assert rel["tied"] == c.tie, c.name
            assert rel["band"] == c.band or c.group != "collision", (c.name, rel["band"])
        _TABLE = t
    return _TABLE


def cases_of(pset, mixed_only=False):
    """Indices into table() of a parameter set's cases."""
    return [i for i, c in enumerate(table()) if c.pset == pset and (c.mixed_ok or not mixed_only)]


def arrays(idx=None):
    """The inputs of cases `idx` (default: all) as arrays: the keys the fixture stores them under."""
    t = table()
    idx = range(len(t)) if idx is None else idx
    cs = [t[i] for i in idx]
    tab = np.zeros((len(cs), MAXO, 3))
    for i, c in enumerate(cs):
        if c.obstacles:
            tab[i, :len(c.obstacles)] = c.obstacles
    return dict(names=np.array([c.name for c in cs]), pset=np.array([PSET_NAMES.index(c.pset) for c in cs], dtype=np.int32), obs_tab=tab,
                n_obs=np.array([len(c.obstacles) for c in cs], dtype=np.int32), goal=np.array([c.goal for c in cs]), pose=np.array([c.pose for c in cs]),
                ep_t=np.array([c.ep_t for c in cs], dtype=np.int32), tot_t=np.array([c.tot_t for c in cs], dtype=np.int64),
                action=np.array([c.action for c in cs], dtype=np.int32), mixed_ok=np.array([c.mixed_ok for c in cs]), stationary=np.array([c.stationary for c in cs]),
                tie=np.array([c.tie for c in cs]), rounded=np.array([c.rounded for c in cs]), group=np.array([GROUPS.index(c.group) for c in cs], dtype=np.int32))


def expected(idx=None):
    """What exact arithmetic says of cases `idx`: info, done, reward (float64; of a stationary case exact, of a moving one WITHOUT dis_before - dis_after),
    the flags collide / out / goal, the pose after the step (exact for a stationary case, predicted for a moving one) and the counters."""
    t = table()
    idx = range(len(t)) if idx is None else idx
    out = dict(info=[], reward=[], collide=[], out=[], goal=[], state=[], ep_t=[], tot_t=[])
    for i in idx:
        c = t[i]
        rel = relations(c)
        info, reward = ladder(pset_params(c.pset), rel)
        x, y, theta, speed = predict_pose(c)
        out["info"].append(info); out["reward"].append(reward)
        for k in ("collide", "out", "goal"):
            out[k].append(rel[k])
        out["state"].append([x, y, theta, speed, 0.0, 0.0])
        out["ep_t"].append(c.ep_t + 1); out["tot_t"].append(c.tot_t + 1)
    r = {k: np.array(v) for k, v in out.items()}
    r["info"] = r["info"].astype(np.uint8)
    r["done"] = r["info"] != NORMAL
    r["ep_t"] = r["ep_t"].astype(np.int32)
    return r


def worlds(idx):
    """Cases `idx` as VecMarineNavEnv.load_worlds dicts (no vortex cores; start = the pose, so the first observation is the pose's)."""
    t = table()
    return [dict(cores=np.zeros((0, 4)), obstacles=np.array(t[i].obstacles, dtype=np.float64).reshape(-1, 3), start=t[i].pose[:2], goal=t[i].goal,
                 init_theta=t[i].pose[2], init_speed=t[i].pose[3]) for i in idx]


def states(idx):
    """[len(idx), 6] set_state rows: x, y, theta, speed, velocity 0."""
    t = table()
    s = np.zeros((len(idx), 6))
    s[:, :4] = [t[i].pose for i in idx]
    return s


def cyclic(idx, n=N_ENVS):
    """`idx` repeated cyclically to n entries."""
    idx = np.asarray(idx)
    return idx[np.arange(n) % len(idx)]


def bits64(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def expressible(idx=None):
    """The reference can run the case: its ladder holds 1000 for the episode limit."""
    t = table()
    idx = range(len(t)) if idx is None else idx
    return np.array([pset_params(t[i].pset)["max_episode_steps"] == 1000 for i in idx])
