"""The step kernels against the build BEFORE their loads were reordered, bit for bit: tests/golden/step_bits_parent.npz holds what that build wrote in the
scenario of tests/step_bits_scenario.py (37 envs, all nine actions in every step, episodes ending by their clocks, both precisions, the default parameters
and a set with other beam tables and a snapped vertical beam) -- observations, rewards, done / info flags, pose, counters, the observation after
`reset_done` and the 37 ring rows of every step.  Replayed here through `mn_step` at every lanes-per-env mapping, through `mn_step_append` and through
`mn_rollout` with the same actions.  Moving loads, table reads and two host-side reciprocals changes no arithmetic: raw bits are compared, no tolerance."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import step_bits_scenario as sc      # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def parent():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return np.load(sc.FIXTURE)


def _same(z, prec, case, got, keys):
    for k in keys:
        ref = z[f"{prec}/{case}/{k}"]
        assert got[k].dtype == ref.dtype and got[k].shape == ref.shape, (k, got[k].dtype, got[k].shape, ref.dtype, ref.shape)
        bad = np.argwhere(got[k] != ref)
        assert len(bad) == 0, (prec, case, k, len(bad), bad[:4].tolist())


def test_fixture_exercises_what_it_is_for(parent):
    for prec in ("f64", "mixed"):
        assert sc.snapped_hits(parent, prec) > 0
        for case in ("default", "S3"):
            assert (parent[f"{prec}/{case}/done"].sum(axis=0) >= 1).all()                 # every env's episode ended (and its world was rebuilt)
            a = parent[f"{prec}/{case}/ring_actions"].reshape(sc.T, sc.N)
            assert all(set(a[t].tolist()) == set(range(9)) for t in range(sc.T))           # all nine actions in every step
        assert not np.array_equal(parent[f"{prec}/default/obs"], parent[f"{prec}/S3/obs"])


@pytest.mark.parametrize("lanes", [0, 1, 2, 4, 8])
@pytest.mark.parametrize("prec,case", sc.CASES)
def test_step_equals_the_parent_build(parent, prec, case, lanes):
    _same(parent, prec, case, sc.run_loop(prec, case, step_lanes=lanes), sc.ENV_KEYS)


@pytest.mark.parametrize("lanes", [0, 1, 2, 4, 8])
@pytest.mark.parametrize("prec,case", sc.CASES)
def test_step_append_equals_the_parent_build(parent, prec, case, lanes):
    _same(parent, prec, case, sc.run_loop(prec, case, step_lanes=lanes, append=True), sc.ENV_KEYS + sc.RING_KEYS)


@pytest.mark.parametrize("lanes", [0, 2, 4, 8, 16])
@pytest.mark.parametrize("prec,case", sc.CASES)
def test_rollout_with_given_actions_equals_the_parent_build(parent, prec, case, lanes):
    """One mn_rollout launch = T x (mn_step, mn_reset_done): its traces are the loop's step outputs, what it leaves behind the loop's last observations and state."""
    got = sc.run_rollout(prec, case, rollout_lanes=lanes)
    _same(parent, prec, case, got, ("obs", "reward", "done", "info"))
    z = lambda k: parent[f"{prec}/{case}/{k}"]
    assert np.array_equal(got["final_obs"], z("obs_next")[-1])
    assert np.array_equal(got["ep_t"], _after_reset(z("ep_t")[-1], z("done")[-1])) and np.array_equal(got["tot_t"], z("tot_t")[-1])
    keep = z("done")[-1] == 0      # (an env that ended in the last step: the fixture has its terminal pose, the handle the new episode's)
    assert np.array_equal(got["state"][keep], z("state")[-1][keep])


def _after_reset(ep_t, done):
    return np.where(done != 0, 0, ep_t.view(np.int32)).astype(np.int32).view(np.uint32)
