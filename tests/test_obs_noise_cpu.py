"""Observation noise without a GPU: the rule's body (csrc/mn_obs_noise_body.h) compiled for the host (tests/obs_noise_host.hip) against the numpy twin
(tests/obs_noise_twin.py) word for word -- row keys, channel words, z values and the perceived rows --, obs_noise.perturb on CPU tensors against the same
words, the properties the rule promises (off means untouched, no-return beams stay, the key decides the draws), the statistics of the draws, and the
refusals at construction."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import obs_noise_twin as TW      # noqa: E402

CSRC = os.path.join(ROOT, "distributional_rl_navigation_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
SEED = 20261021

# (name, vel_sigma, goal_sigma, sonar_rel_sigma, sonar_miss_p): each channel alone, all together, a miss probability at each end, all off
SPECS = [("vel", 0.05, 0.0, 0.0, 0.0), ("goal", 0.0, 0.5, 0.0, 0.0), ("sonar", 0.0, 0.0, 0.1, 0.0), ("miss", 0.0, 0.0, 0.0, 0.2),
         ("all", 0.03, 0.3, 0.05, 0.05), ("miss1", 0.0, 0.0, 0.02, 1.0), ("off", 0.0, 0.0, 0.0, 0.0)]


def clean_rows(n, rng):
    """n observation-like float32 rows: velocities, goals and sonar points of the env's magnitudes; a third all-hit, a third no-hit, a third mixed
    (each beam a return with probability 1/2); a few -0.0 in the velocity and in no-return beams."""
    obs = np.zeros((n, 26), dtype=np.float32)
    obs[:, 0:2] = rng.normal(0.0, 1.0, (n, 2))
    obs[:, 2:4] = rng.uniform(-50.0, 50.0, (n, 2))
    pts = rng.uniform(-20.0, 20.0, (n, 11, 2)).astype(np.float32)
    kind = np.arange(n) % 3
    hit = np.where(kind[:, None] == 0, True, np.where(kind[:, None] == 1, False, rng.random((n, 11)) < 0.5))
    obs[:, 4:] = np.where(hit[:, :, None], pts, np.float32(0.0)).reshape(n, 22)
    obs[::7, 0] = np.float32(-0.0)
    nohit = np.flatnonzero(kind == 1)
    obs[nohit[::3], 4] = np.float32(-0.0)      # a no-return beam whose x word is -0.0: "no reflection" all the same
    return obs


def keys(n, rng):
    """env indices (small, around 2^31 and 2^32, near 2^63) and episode_timesteps (0, 999 and between) of n rows."""
    env = rng.integers(0, 4096, n).astype(np.uint64)
    env[1::5] = np.uint64(1 << 31) + rng.integers(0, 1000, len(env[1::5])).astype(np.uint64)
    env[2::5] = np.uint64(1 << 32) + rng.integers(0, 1000, len(env[2::5])).astype(np.uint64)
    env[3::5] = np.uint64((1 << 63) - 7) + rng.integers(0, 1000, len(env[3::5])).astype(np.uint64)
    ep = rng.integers(0, 1000, n).astype(np.int32)
    ep[0::4] = 0
    ep[1::4] = 999
    return env, ep


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    exe = str(tmp_path_factory.mktemp("obs_noise_host") / "obs_noise_host")
    r = subprocess.run([HIPCC, "--cuda-host-only", "-O2", "-std=c++17", "-ffp-contract=off", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-o", exe,
                        os.path.join(ROOT, "tests", "obs_noise_host.hip")], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def run_host(exe, tmp_path, tag, obs, env, ep, seed, spec):
    from distributional_rl_navigation_amd.obs_noise import MnObsNoise
    fin, fout = str(tmp_path / f"{tag}.in"), str(tmp_path / f"{tag}.out")
    n = len(obs)
    with open(fin, "wb") as f:
        f.write(np.array([n], dtype="<i8").tobytes())
        f.write(bytes(MnObsNoise(seed & ((1 << 64) - 1), *spec)))
        f.write(env.astype("<u8").tobytes()); f.write(ep.astype("<i4").tobytes()); f.write(obs.astype("<f4").tobytes())
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    raw = open(fout, "rb").read()
    status, thr = np.frombuffer(raw[:8], dtype="<i4")[0], np.frombuffer(raw[4:8], dtype="<u4")[0]
    if status:
        assert len(raw) == 8
        return int(status), int(thr), None, None, None
    o = 8
    rows = np.frombuffer(raw[o:o + n * 104], dtype="<f4").reshape(n, 26); o += n * 104
    words = np.frombuffer(raw[o:o + n * 31 * 8], dtype="<u8").reshape(n, 31); o += n * 31 * 8
    z = np.frombuffer(raw[o:], dtype="<f4").reshape(n, 15)
    return 0, int(thr), rows, words, z


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize("spec", SPECS, ids=[s[0] for s in SPECS])
def test_host_build_equals_the_twin_word_for_word(host, tmp_path, spec):
    rng = np.random.default_rng(SEED)
    n = 3000
    obs = clean_rows(n, rng)
    env, ep = keys(n, rng)
    for seed in (0, 0x0123456789ABCDEF, (1 << 64) - 1):
        status, thr, rows, words, z = run_host(host, tmp_path, spec[0], obs, env, ep, seed, spec[1:])
        assert status == 0 and thr == TW.miss_threshold(spec[4])
        key = TW.row_key(seed, env, ep)
        assert np.array_equal(words[:, 0], key)
        for c in range(TW.CHANNELS):
            assert np.array_equal(words[:, 1 + 2 * c], TW.word(key, c, 0)) and np.array_equal(words[:, 2 + 2 * c], TW.word(key, c, 1))
            assert np.array_equal(bits(z[:, c]), bits(TW.z_of(TW.word(key, c, 0))))
        want = TW.perturb(obs, env, ep, seed, *spec[1:])
        assert np.array_equal(bits(rows), bits(want))
        if spec[0] == "off":
            assert np.array_equal(bits(rows), bits(obs))
        elif spec[0] != "miss1":
            assert not np.array_equal(bits(rows), bits(obs))


@pytest.mark.parametrize("spec", SPECS, ids=[s[0] for s in SPECS])
def test_torch_perturb_equals_the_twin(spec):
    import torch
    from distributional_rl_navigation_amd.obs_noise import ObsNoise, perturb
    rng = np.random.default_rng(SEED + 1)
    n = 2000
    obs = clean_rows(n, rng)
    env, ep = keys(n, rng)
    for seed in (5, (1 << 64) - 3):
        noise = ObsNoise(seed, *spec[1:])
        got = perturb(torch.from_numpy(obs), torch.from_numpy(env.view(np.int64)), torch.from_numpy(ep), noise).numpy()
        assert np.array_equal(bits(got), bits(TW.perturb(obs, env, ep, seed, *spec[1:])))
        assert noise.miss_threshold == TW.miss_threshold(spec[4]) and noise.is_off == (spec[0] == "off")
    # a [T][n][26] trace with per-step counters, and Python ints for the keys
    tr = obs[:1998].reshape(3, 666, 26)
    e3, t3 = np.arange(666, dtype=np.uint64) + np.uint64(77), np.array([0, 1, 2], dtype=np.int32)[:, None]
    noise = ObsNoise(9, *spec[1:])
    got = perturb(torch.from_numpy(tr), torch.from_numpy(e3.view(np.int64)), torch.from_numpy(t3), noise).numpy()
    assert np.array_equal(bits(got), bits(TW.perturb(tr, e3, t3, 9, *spec[1:])))
    got1 = perturb(torch.from_numpy(obs[:1]), 12, 34, noise).numpy()
    assert np.array_equal(bits(got1), bits(TW.perturb(obs[:1], np.uint64(12), np.int32(34), 9, *spec[1:])))


def test_off_means_untouched_and_no_return_beams_stay():
    rng = np.random.default_rng(SEED + 2)
    obs = clean_rows(999, rng)
    env, ep = keys(999, rng)
    assert (bits(obs) == 0x80000000).any()
    assert np.array_equal(bits(TW.perturb(obs, env, ep, 3)), bits(obs))      # all-zero description: every bit, the -0.0 words included
    nohit = (obs[:, 4::2] == 0) & (obs[:, 5::2] == 0)
    assert nohit.any() and (~nohit).any()
    for spec in SPECS:
        out = TW.perturb(obs, env, ep, 3, *spec[1:])
        assert np.array_equal(bits(out[:, 4::2])[nohit], bits(obs[:, 4::2])[nohit]) and np.array_equal(bits(out[:, 5::2])[nohit], bits(obs[:, 5::2])[nohit])
        if spec[1] == 0:
            assert np.array_equal(bits(out[:, 0:2]), bits(obs[:, 0:2]))      # a channel whose parameter is zero is skipped
        if spec[2] == 0:
            assert np.array_equal(bits(out[:, 2:4]), bits(obs[:, 2:4]))
        if spec[3] == 0 and spec[4] == 0:
            assert np.array_equal(bits(out[:, 4:]), bits(obs[:, 4:]))
    allmiss = TW.perturb(obs, env, ep, 3, sonar_miss_p=1.0)
    assert (allmiss[:, 4:] == 0).all() and np.array_equal(bits(allmiss[:, :4]), bits(obs[:, :4]))


def test_the_key_decides_the_draws():
    rng = np.random.default_rng(SEED + 3)
    obs = np.repeat(clean_rows(3, rng)[:1], 512, axis=0)      # one all-hit clean row, 512 times
    assert (obs[0, 4:] != 0).all()
    spec = dict(vel_sigma=0.05, goal_sigma=0.5, sonar_rel_sigma=0.1)
    env, ep = np.arange(512, dtype=np.uint64), np.full(512, 17, dtype=np.int32)
    base = TW.perturb(obs, env, ep, 1, **spec)
    # equal keys and equal clean rows: equal perceived rows -- whatever else is in the batch
    assert np.array_equal(bits(TW.perturb(obs[:7], env[100:107], ep[:7], 1, **spec)), bits(base[100:107]))
    assert np.array_equal(bits(TW.perturb(obs[::-1], env[::-1], ep, 1, **spec)), bits(base[::-1]))
    # another seed, env index or ep_t: other draws -- every row differs, and all but a few of the 512 x 26 words (z takes 2^18 values and a float32
    # sum rounds: two draws give the same word with probability below 1e-3, so 99 % is a bound with room)
    for other in (TW.perturb(obs, env, ep, 2, **spec), TW.perturb(obs, env + np.uint64(512), ep, 1, **spec), TW.perturb(obs, env, ep + 1, 1, **spec)):
        differs = bits(other) != bits(base)
        assert differs.any(axis=1).all() and differs.mean() > 0.99
    assert len({r.tobytes() for r in base}) == 512      # and no two envs perceive the same
    # the miss words are the key's too
    m = [TW.perturb(obs, env, ep, s, sonar_miss_p=0.5)[:, 4::2] == 0 for s in (1, 2)]
    assert m[0].any() and not m[0].all() and not np.array_equal(m[0], m[1])


def test_statistics_of_the_draws():
    """N draws of z and of the miss word: mean, variance and miss rate within five standard errors, computed here from N.  z = the centred sum of four
    uniform 16-bit words over sqrt((2^32 - 1) / 3): variance 1, fourth moment 2.7 (the kurtosis of a sum of four uniforms: 3 - 1.2 / 4)."""
    N = 15 * 40000
    env = np.arange(40000, dtype=np.uint64)
    key = TW.row_key(77, env, np.int32(5))
    z = np.concatenate([TW.z_of(TW.word(key, c, 0)) for c in range(TW.CHANNELS)]).astype(np.float64)
    assert len(z) == N and np.abs(z).max() <= 131070 * float(TW.Z_SCALE)
    se_mean = 1.0 / np.sqrt(N)
    se_var = np.sqrt((2.7 - 1.0) / N)      # Var(z^2) = E z^4 - 1
    assert abs(z.mean()) < 5 * se_mean, (z.mean(), se_mean)
    assert abs(z.var() - 1.0) < 5 * se_var, (z.var(), se_var)
    for p in (0.05, 0.2, 0.5):
        thr = TW.miss_threshold(p)
        q = thr / 16777216.0      # the probability the threshold stands for
        miss = np.concatenate([(TW.word(key, c, 1) >> np.uint64(40)) < np.uint64(thr) for c in range(4, TW.CHANNELS)])
        se = np.sqrt(q * (1 - q) / len(miss))
        assert abs(miss.mean() - q) < 5 * se, (p, miss.mean(), se)
        assert abs(q - p) < 2.0 ** -24 + 1e-9      # float32(p) truncated to 24 bits
    # the normal word and the miss word of a channel are different words
    assert not np.array_equal(TW.word(key, 4, 0), TW.word(key, 4, 1))


def test_refusals_name_their_parameter():
    from distributional_rl_navigation_amd.obs_noise import ObsNoise
    for name in ("vel_sigma", "goal_sigma", "sonar_rel_sigma"):
        for bad in (-0.01, float("nan"), float("inf"), 1e39):
            with pytest.raises(ValueError, match=name):
                ObsNoise(1, **{name: bad})
    for bad in (-1e-9, 1.0000001, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="sonar_miss_p"):
            ObsNoise(1, sonar_miss_p=bad)
    ok = ObsNoise(1, 0.0, 0.0, 0.0, 1.0)
    assert ok.miss_threshold == 1 << 24 and not ok.is_off and ObsNoise().is_off and ObsNoise(5).is_off


def test_host_program_refuses_what_the_library_refuses(host, tmp_path):
    obs = np.zeros((1, 26), dtype=np.float32)
    env, ep = np.zeros(1, dtype=np.uint64), np.zeros(1, dtype=np.int32)
    for k, name in enumerate(("vel_sigma", "goal_sigma", "sonar_rel_sigma", "sonar_miss_p")):
        for bad in ((-0.5, float("nan"), float("inf")) if k < 3 else (-0.5, 1.5, float("nan"))):
            spec = [0.0, 0.0, 0.0, 0.0]
            spec[k] = bad
            status, _, rows, _, _ = run_host(host, tmp_path, f"bad{k}", obs, env, ep, 1, spec)
            assert status == 1 + k and rows is None, (name, bad)


def test_header_declares_and_capi_binds():
    import re
    from distributional_rl_navigation_amd import _capi
    from distributional_rl_navigation_amd.obs_noise import MnObsNoise
    with open(os.path.join(ROOT, "include", "marinenav_hip.h")) as f:
        h = f.read()
    sig = {s[0]: s for s in _capi.SIGNATURES}
    for name, nargs in (("mn_obs_perturb", 7), ("mn_set_obs_noise", 3), ("mn_env_perturb_obs", 4)):
        assert re.search(r"int %s\(" % name, h) and len(sig[name][2]) == nargs
    assert C.sizeof(MnObsNoise) == 24
    for const in ("0xC2B2AE3D27D4EB4F", "0x165667B19E3779F9", "0x1.bb67aep-16f"):      # the header states the rule's constants
        assert const in h
    with open(os.path.join(CSRC, "mn_obs_noise_body.h")) as f:
        body = f.read()
    assert "0x%016X" % int(TW.ROW_KEY) in body and "0x%016X" % int(TW.CHANNEL_KEY) in body and "0x1.bb67aep-16f" in body
