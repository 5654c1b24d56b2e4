"""The classical baselines branch by branch, as far as it goes without a GPU: golden G19 (tests/golden/make_golden.py g19) records the actions of
the reference's APF.py / BA.py on float32-exact rows -- class by class, under five (a, w) tables -- and which rows are `stable`: the action survives
8 copies of the row perturbed by 1e-9 relative, seven orders above what a libm's last ulps can move.  On those rows every faithful float64
evaluation must give the reference's action, so the bound is EQUALITY, on every stable row and on every hand-written `exact` row, for

  * the tensor formulation of planners.py in float64, and
  * the device functions of csrc/mn_planners.h themselves: they are __host__ __device__, tests/planners_host.hip compiles the same text for the
    CPU (hipcc --cuda-host-only -O2 -ffp-contract=off) and writes mn_policy_act for every (table, kind, row).

tests/test_planner_branches_gpu.py holds the kernels to the same file."""
import os
import struct
import subprocess

import numpy as np
import pytest
import torch

from distributional_rl_navigation_amd.planners import apf_act_batch, ba_act_batch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "distributional_rl_navigation_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
KINDS = ("APF", "BA")      # the order of the fixture's second axis


def load_g19():
    z = np.load(os.path.join(ROOT, "tests", "golden", "g19_planner_branches.npz"))
    g = {k: z[k] for k in z.files}
    g["names"] = [str(s) for s in g["cls_names"]]
    g["exact"] = g["cls"] == g["names"].index("exact")
    g["checked"] = g["stable"] | g["exact"][None, None, :]      # rows on which equality is required
    return g


G19 = load_g19()


def tensor_actions(obs32, tables):
    """planners.py in float64 on the float32 rows: [T][2][n] int64."""
    obs = torch.from_numpy(np.ascontiguousarray(obs32)).double()
    return np.stack([np.stack([apf_act_batch(obs, t[0], t[1]).numpy(), ba_act_batch(obs, t[0], t[1]).numpy()]) for t in tables])


def mismatches(got, want, mask, g=G19):
    """A readable list of the first rows of `mask` at which got != want: (table, kind, row, class, got, want)."""
    bad = np.argwhere((got != want) & mask)
    return [(str(g["table_names"][t]), KINDS[k], int(i), g["names"][g["cls"][i]], int(got[t, k, i]), int(want[t, k, i])) for t, k, i in bad[:12]], len(bad)


def build_host(out_dir, extra=(), source=None, csrc=CSRC):
    exe = os.path.join(str(out_dir), "planners_host")
    r = subprocess.run([HIPCC, "--cuda-host-only", "-O2", "-std=c++17", "-ffp-contract=off", *extra, "-I" + os.path.join(ROOT, "include"), "-I" + csrc,
                        "-o", exe, source or os.path.join(ROOT, "tests", "planners_host.hip")], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def run_host(exe, tmp_dir, obs32, tables):
    """The host program on rows [n][26] float32 and tables [T][2][3]: int8 [T][2][n]."""
    obs32 = np.ascontiguousarray(obs32, dtype="<f4")
    tables = np.ascontiguousarray(tables, dtype="<f8")
    n, nt = len(obs32), len(tables)
    fin, fout = os.path.join(str(tmp_dir), "rows.in"), os.path.join(str(tmp_dir), "rows.out")
    with open(fin, "wb") as f:
        f.write(struct.pack("<2i", n, nt))
        f.write(tables.tobytes())
        f.write(obs32.tobytes())
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    out = np.fromfile(fout, dtype=np.int8)
    assert out.size == nt * 2 * n
    return out.reshape(nt, 2, n)


@pytest.fixture(scope="module")
def host_actions(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    d = tmp_path_factory.mktemp("planners_host")
    return run_host(build_host(d), d, G19["obs"], G19["tables"])


@pytest.fixture(scope="module")
def tensor_g19():
    return tensor_actions(G19["obs"], G19["tables"])


# ---- the fixture's own conditions -----------------------------------------------------------------------------------------------------------------------
def test_fixture_meets_its_conditions():
    g = G19
    n = len(g["obs"])
    T = len(g["tables"])
    assert g["obs"].dtype == np.float32 and g["obs"].shape == (n, 26)
    assert np.array_equal(g["obs"].astype(np.float64).astype(np.float32).view(np.uint32), g["obs"].view(np.uint32))      # its own float32 round trip
    assert g["cls"].dtype == np.int16 and g["cls"].shape == (n,) and g["cls"].min() == 0 and g["cls"].max() == len(g["names"]) - 1
    assert g["tables"].dtype == np.float64 and g["tables"].shape == (T, 2, 3) and T >= 5 and len(g["table_names"]) == T
    assert g["act"].dtype == np.int8 and g["act"].shape == (T, 2, n) and g["act"].min() >= 0 and g["act"].max() <= 8
    assert g["stable"].dtype == np.bool_ and g["stable"].shape == (T, 2, n)
    tabs = {str(k): v for k, v in zip(g["table_names"], g["tables"])}
    assert np.array_equal(tabs["S1"], [[-0.6, 0.0, 0.5], [-0.7, 0.1, 0.4]])
    assert (tabs["positive_unsorted"] > 0).all(axis=1)[0] and (tabs["no_positive_a"][0] <= 0).all()
    assert tabs["duplicates"][0][0] == tabs["duplicates"][0][1] and tabs["duplicates"][1][0] == tabs["duplicates"][1][1]
    for name in ["real"] + [f"returns_{k}" for k in range(12)] + ["still", "crawl", "slow", "fast", "behind", "span", "wall_vertical", "wall_near_vertical",
                                                                   "wall_sloped", "two_same_x", "two_flip", "exact"]:
        assert name in g["names"], name
    count = lambda name: int((g["cls"] == g["names"].index(name)).sum())
    assert count("real") == 2048 and min(count("returns_1"), count("returns_2"), count("returns_3")) >= 200 and 0 < count("exact") <= 64
    assert count("exact") == len(g["exact_reasons"])
    pts = g["obs"][:, 4:].reshape(n, 11, 2)
    n_ret = ((pts[:, :, 0] != 0) | (pts[:, :, 1] != 0)).sum(axis=1)
    for k in range(12):
        assert (n_ret[g["cls"] == g["names"].index(f"returns_{k}")] == k).all()
    speed = np.hypot(g["obs"][:, 0].astype(np.float64), g["obs"][:, 1].astype(np.float64))
    assert (speed[g["cls"] == g["names"].index("still")] == 0).all()
    crawl = speed[g["cls"] == g["names"].index("crawl")]
    assert (crawl < 1e-3).sum() >= 20 and (crawl > 1e-3).sum() >= 20 and crawl.max() < 1e-2
    # the 1 % cap over all classes but `exact`, at least 20 stable rows per class, the recorded counts
    unstable = (~g["stable"][:, :, ~g["exact"]]).sum(axis=2)
    assert np.array_equal(unstable, g["unstable_counts"])
    assert (unstable <= 0.01 * int((~g["exact"]).sum())).all(), unstable
    for c, name in enumerate(g["names"]):
        if name != "exact":
            assert (g["stable"][:, :, g["cls"] == c].sum(axis=2) >= 20).all(), name
    print(f"G19: {n} rows, {len(g['names'])} classes, unstable per (table, kind) {unstable.tolist()}")


# ---- planners.py and the host build of mn_planners.h against the reference's actions -----------------------------------------------------------------------
def test_tensor_formulation_equals_the_reference_on_every_stable_row(tensor_g19):
    bad, n_bad = mismatches(tensor_g19, G19["act"], G19["stable"])
    assert n_bad == 0, (n_bad, bad)


def test_host_program_equals_the_reference_on_every_stable_and_exact_row(host_actions):
    bad, n_bad = mismatches(host_actions, G19["act"], G19["checked"])
    assert n_bad == 0, (n_bad, bad)
    assert host_actions.min() >= 0 and host_actions.max() <= 8      # the unstable rows included
    print("host program != reference on unstable rows:", ((host_actions != G19["act"]) & ~G19["checked"]).sum(axis=2).tolist())


def test_host_program_equals_the_tensor_formulation_on_every_stable_row(host_actions, tensor_g19):
    bad, n_bad = mismatches(host_actions, tensor_g19, G19["stable"])
    assert n_bad == 0, (n_bad, bad)
