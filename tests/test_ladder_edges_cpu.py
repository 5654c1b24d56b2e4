"""The termination ladder on its thresholds, ties and coinciding rungs (tests/ladder_edges.py), without a GPU: the case table against its own exact
arithmetic, the reference's recorded answers (tests/golden/g20_ladder_edges.npz) against that arithmetic, and the two CPU restatements -- OracleEnv
(oracle/marinenav_oracle.c) and the CPU twin (oracle/mn_cpu_twin.c through the mn_* entry points) -- against both.  Stationary cases have no tolerance:
info, done, counters identical, reward equal, pose bit for bit.  tests/test_ladder_edges_gpu.py holds every kernel to the same table."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import ladder_edges as LE      # noqa: E402
import params_sets as PS       # noqa: E402
from test_cpu_twin import TWIN, bind, numpy_driver      # noqa: E402


@pytest.fixture(scope="module")
def g20():
    return np.load(LE.FIXTURE)


def test_the_table_is_what_its_names_say():
    """`table()` runs the exact-arithmetic assertions of every case; here what the groups owe: members the mixed kernel can read, the radii, the band, all
    32 coinciding combinations, and the copy of the library's defaults the expectations are computed from."""
    from distributional_rl_navigation_amd import _capi
    t = LE.table()
    p = _capi.default_params()
    for k, v in LE.DEFAULTS.items():
        assert getattr(p, k) == v, k
    for name, spec in LE.PSETS:
        assert set(spec) <= {f[0] for f in _capi.MnParams._fields_}, name
    by_group = {g: [c for c in t if c.group == g] for g in LE.GROUPS}
    for g, cs in by_group.items():
        assert len(cs) >= 4 and sum(c.mixed_ok for c in cs) >= 1, g
    thr = by_group["collision"]
    assert len({c.obstacles[0][2] for c in thr if c.mixed_ok}) >= 32 and len({c.obstacles[0][2] for c in thr if not c.mixed_ok}) >= 64
    assert len({c.obstacles[0][2] for c in thr if c.band}) >= 64 and sum(c.band and c.mixed_ok for c in thr) >= 16
    rel = [LE.relations(c) for c in thr]
    assert all(r["collide"] for c, r in zip(thr, rel) if c.name.endswith((" below", " at", " 1 - 2^-40"))) and not any(
        r["collide"] for c, r in zip(thr, rel) if c.name.endswith((" above", " 1 + 2^-40")))
    rounded = [(c, r) for c, r in zip(thr, rel) if c.rounded]      # the square root's rounding decides: exact arithmetic and the squared comparison say clear
    assert len(rounded) >= 16 and all(r["collide"] and r["band"] for _, r in rounded)
    assert not any(r["collide"] for c, r in zip(thr, rel) if c.name.endswith(("thr one ulp smaller", "thr smaller by 2^-40"))) and all(
        r["collide"] for c, r in zip(thr, rel) if c.name.endswith("thr one ulp larger"))
    # band and far cases side by side: every 4 consecutive envs (one wavefront at 16 lanes per env) of the D0 batch's threshold stretch hold both
    d0 = [t[i] for i in LE.cases_of("D0")]
    first = next(i for i, c in enumerate(d0) if c.group == "collision")
    stretch = [c.band for c in d0[first:first + 64 * 5]]
    assert all(any(stretch[i:i + 4]) and not all(stretch[i:i + 4]) for i in range(0, len(stretch) - 3))
    for pset in ("D0", "D1", "S4"):
        combos = {(r["out"], r["long"], r["collide"], r["goal"]) for c in by_group["priority"] if c.pset == pset for r in [LE.relations(c)]}
        assert len(combos) == 16, pset
    assert {(LE.relations(c)["tied"], c.group == "tie") for c in t} == {(True, True), (False, False)}
    by_d2 = [c for c in by_group["nearest"] if "by d2" in c.name]      # roots that round together: the nearer one decides, first or second in the table
    assert len(by_d2) >= 32 and [LE.relations(c)["collide"] for c in by_d2[:4]] == [True, False, True, False]
    assert {LE.relations(c)["nearest"] for c in by_d2} == {0, 1} and not any(LE.relations(c)["tied"] for c in by_d2)
    for c in by_d2:
        d = [float(np.sqrt((ox - c.pose[0]) ** 2 + (oy - c.pose[1]) ** 2)) for ox, oy, _ in c.obstacles]
        assert d[0] == d[1], c.name
    both = [c for c in by_group["tie"] if len(c.obstacles) == LE.MAXO]
    assert {LE.relations(c)["collide"] for c in both} == {True, False}
    e = LE.expected()
    assert set(np.unique(e["info"])) == {0, 1, 2, 3, 4}
    print(f"[ladder edges] {len(t)} cases: " + ", ".join(f"{g} {len(cs)} ({sum(c.mixed_ok for c in cs)} mixed)" for g, cs in by_group.items()))


def test_the_fixture_is_current(g20):
    inp = LE.arrays()
    for k, v in inp.items():
        assert g20[k].dtype == v.dtype and np.array_equal(g20[k], v), k
    assert np.array_equal(LE.bits64(g20["pose"]), LE.bits64(inp["pose"])) and np.array_equal(LE.bits64(g20["obs_tab"]), LE.bits64(inp["obs_tab"]))      # -0.0 is not 0.0
    assert [str(s) for s in g20["set_names"]] == LE.PSET_NAMES and np.array_equal(g20["ref_ok"], LE.expressible())


def _check(what, idx, exp, info, done, reward, state, ep_t, tot_t, ref=None, tol=1e-9):
    """Outputs of cases `idx` (one row each) against exact arithmetic `exp` (rows of LE.expected(idx)) and, where `ref` = (fixture, rows) is given, the
    reference.  Stationary: no tolerance.  Moving: info exact, floats within `tol` of the reference."""
    t = LE.table()
    names = np.array([t[i].name for i in idx])
    st = np.array([t[i].stationary for i in idx])
    bad = np.nonzero(np.asarray(info) != exp["info"])[0]
    assert len(bad) == 0, (what, [(names[i], int(info[i]), int(exp["info"][i])) for i in bad[:8]])
    assert np.array_equal(np.asarray(done).astype(bool), exp["done"]), what
    assert np.array_equal(ep_t, exp["ep_t"]) and np.array_equal(tot_t, exp["tot_t"]), what
    bad = np.nonzero(st & (np.asarray(reward, dtype=np.float64) != exp["reward"]))[0]
    assert len(bad) == 0, (what, [(names[i], float(reward[i]), float(exp["reward"][i])) for i in bad[:8]])
    bad = np.nonzero(st & (LE.bits64(state[:, :4]) != LE.bits64(exp["state"][:, :4])).any(axis=1))[0]
    assert len(bad) == 0, (what, "pose moved", [names[i] for i in bad[:8]])
    if ref is not None:
        z, rows = ref
        m = ~st
        assert z["ref_ok"][rows][m].all()
        assert np.array_equal(np.asarray(info)[m], z["ref_info"][rows][m])
        np.testing.assert_allclose(np.asarray(reward, dtype=np.float64)[m], z["ref_reward"][rows][m], rtol=0, atol=tol)
        np.testing.assert_allclose(state[m][:, :4], z["ref_state"][rows][m][:, :4], rtol=0, atol=tol)


def test_the_reference_against_exact_arithmetic(g20):
    """Every case the reference can express and that is no tie: its recorded info, done, counters, reward and pose ARE what exact arithmetic says.  Ties:
    what its KD-tree answered, printed, not asserted."""
    ok = g20["ref_ok"] & ~g20["tie"]
    idx = np.nonzero(ok)[0]
    exp = {k: v[idx] for k, v in LE.expected().items()}
    _check("reference", idx, exp, g20["ref_info"][idx], g20["ref_done"][idx], g20["ref_reward"][idx], g20["ref_state"][idx], g20["ref_ep_t"][idx],
           g20["ref_tot_t"][idx])
    mv = ~g20["stationary"][idx]
    assert mv.sum() >= 6 and (np.abs(g20["ref_state"][idx][mv][:, :2] - exp["state"][mv][:, :2]) < 1e-9).all()      # predict_pose is the reference's motion
    assert (np.abs(g20["ref_reward"][idx][mv] - exp["reward"][mv]) > 0.1).all()                                  # ... and dis_before - dis_after is in the reward
    tie = np.nonzero(g20["tie"])[0]
    e = LE.expected(tie)
    same = g20["tie_ref_info"][tie] == e["info"]
    print(f"[ladder edges] ties: the reference's KD-tree agrees with first-in-generation-order on {int(same.sum())} of {len(tie)}")
    for i, s in zip(tie, same):
        print(f"    {'same   ' if s else 'DIFFERS'} {g20['names'][i]}: KD-tree took obstacle {int(g20['tie_ref_nearest'][i])}, the first of the nearest is "
              f"{LE.relations(LE.table()[i])['nearest']}")


def test_oracle_env_on_the_default_parameter_cases(g20):
    """OracleEnv has setters for the boundary flag only: the cases of the two default-parameter sets, ties included (its scan is first-of-equals)."""
    from oracle.oracle import OracleEnv
    t = LE.table()
    for pset in ("D0", "D1"):
        idx = np.array(LE.cases_of(pset))
        info, done, rew, st, ep, tot = [], [], [], [], [], []
        for i in idx:
            c = t[i]
            env = OracleEnv(seed=0)
            env.set_flags(set_boundary=bool(LE.pset_params(pset)["set_boundary"]))
            env.load_world(np.zeros((0, 4)), 0, np.array(c.obstacles).reshape(-1, 3), len(c.obstacles), c.pose[:2], c.goal, c.pose[2], c.pose[3])
            env.set_total_timesteps(c.tot_t)
            env.set_state(list(c.pose) + [0.0, 0.0], c.ep_t)
            _, r, d, code = env.step(c.action)
            s, e_, t_ = env.get_state()
            info.append(code); done.append(d); rew.append(r); st.append(s); ep.append(e_); tot.append(t_)
        _check(f"OracleEnv {pset}", idx, LE.expected(idx), np.array(info), np.array(done), np.array(rew), np.array(st), np.array(ep), np.array(tot), ref=(g20, idx))


@pytest.mark.parametrize("pset", LE.PSET_NAMES)
def test_cpu_twin_on_every_case_it_can_express(g20, pset):
    """The twin keeps the reference's 1000-step limit (mn_set_params refuses another one): sets M0 and M1 are the device's alone, held to exact arithmetic
    in tests/test_ladder_edges_gpu.py."""
    idx = np.array(LE.cases_of(pset))
    L = bind(TWIN)
    d = numpy_driver(L, len(idx))
    if LE.pset_params(pset)["max_episode_steps"] != 1000:
        PS.apply(d.p, LE.pset_spec(pset))
        assert L.mn_set_params(d.h, C.byref(d.p)) != 0
        d.close()
        return
    PS.driver_set(d, LE.pset_spec(pset))
    a = LE.arrays(idx)
    n = len(idx)
    d.load_worlds(np.zeros((n, 8, 4)), np.zeros(n, np.int32), a["obs_tab"], a["n_obs"], a["pose"][:, :2], a["goal"], a["pose"][:, 2], a["pose"][:, 3])
    s, ep, tot = LE.states(idx), a["ep_t"], a["tot_t"]
    assert L.mn_set_state(d.h, 0, n, s.ctypes.data_as(C.POINTER(C.c_double)), ep.ctypes.data_as(C.POINTER(C.c_int32)), tot.ctypes.data_as(C.POINTER(C.c_int64))) == 0
    _, rew, done, info = d.step(a["action"], d.set_actions)
    st, ep1, tot1 = d.state()
    _check(f"CPU twin {pset}", idx, LE.expected(idx), info, done, rew, st, ep1, tot1, ref=(g20, idx))
    assert np.array_equal(d.host(d.rew)[a["stationary"]], rew[a["stationary"]].astype(np.float32))
    d.close()
