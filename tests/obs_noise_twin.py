"""Host twin of the observation-noise rule (include/marinenav_hip.h "Observation noise"; csrc/mn_obs_noise_body.h), in plain numpy: uint64 arithmetic
with wrap-around for the words, float32 -- every product and sum rounded on its own -- for the values.  Written from the header's text.  No torch, no GPU.
tests/test_obs_noise_cpu.py holds the CPU build of the body and obs_noise.perturb to these words; tests/test_obs_noise_gpu.py the kernels.
Plain helper module, no fixtures."""
import numpy as np

from rng_twin import mix64, u64

GOLDEN = np.uint64(0x9E3779B97F4A7C15)
ROW_KEY = np.uint64(0xC2B2AE3D27D4EB4F)
CHANNEL_KEY = np.uint64(0x165667B19E3779F9)
CHANNELS = 15                                          # velocity x, y | goal x, y | eleven beams
Z_SCALE = np.float32(float.fromhex("0x1.bb67aep-16"))  # float32(1 / sqrt((2^32 - 1) / 3))
Z_CENTRE = 131070                                      # 2 * 65535


def miss_threshold(p):
    """(uint32)(double(float32 p) * 2^24): the 24-bit threshold the host computes once."""
    return int(float(np.float32(p)) * 16777216.0)


def row_key(seed, env, ep_t):
    """mix64(mix64(seed + golden (env + 1)) ^ (ROW_KEY (ep_t + 1))); env and ep_t broadcast against each other."""
    with np.errstate(over="ignore"):
        base = mix64(u64(seed) + GOLDEN * (u64(env) + np.uint64(1)))
        return mix64(base ^ (ROW_KEY * (u64(ep_t) + np.uint64(1))))


def word(key, c, w):
    """W(c, w): word w (0 normal, 1 miss) of channel c under the row key(s)."""
    with np.errstate(over="ignore"):
        return mix64(u64(key) ^ (CHANNEL_KEY * np.uint64(2 * c + w + 1)))


def z_of(w):
    """The standard-normal stand-in of a word: the centred sum of its four 16-bit fields, times Z_SCALE; float32."""
    w = u64(w)
    m = np.uint64(0xFFFF)
    s = ((w & m) + ((w >> np.uint64(16)) & m) + ((w >> np.uint64(32)) & m) + (w >> np.uint64(48))).astype(np.int64) - Z_CENTRE
    return s.astype(np.float32) * Z_SCALE


def perturb(obs, env, ep_t, seed, vel_sigma=0.0, goal_sigma=0.0, sonar_rel_sigma=0.0, sonar_miss_p=0.0):
    """The perceived rows of clean float32 rows obs [..., 26]; env / ep_t of the leading shape (or broadcastable to it)."""
    obs = np.asarray(obs)
    assert obs.dtype == np.float32 and obs.shape[-1] == 26
    out = obs.copy()
    lead = obs.shape[:-1]
    key = np.broadcast_to(row_key(seed, np.asarray(env), np.asarray(ep_t)), lead)
    vs, gs, ss = np.float32(vel_sigma), np.float32(goal_sigma), np.float32(sonar_rel_sigma)
    thr = miss_threshold(sonar_miss_p)
    for c in range(4):
        sigma = vs if c < 2 else gs
        if sigma != 0:
            d = (sigma * z_of(word(key, c, 0))).astype(np.float32)
            out[..., c] = obs[..., c] + d
    for b in range(11):
        c, k = 4 + b, 4 + 2 * b
        x, y = obs[..., k], obs[..., k + 1]
        hit = ~((x == 0) & (y == 0))
        miss = np.zeros(lead, dtype=bool)
        if thr != 0:
            miss = hit & ((word(key, c, 1) >> np.uint64(40)) < np.uint64(thr))
        nx, ny = x.copy(), y.copy()
        if ss != 0:
            d = (ss * z_of(word(key, c, 0))).astype(np.float32)
            f = (np.float32(1.0) + d).astype(np.float32)
            scale = hit & ~miss
            nx = np.where(scale, (x * f).astype(np.float32), nx)
            ny = np.where(scale, (y * f).astype(np.float32), ny)
        nx = np.where(miss, np.float32(0.0), nx)
        ny = np.where(miss, np.float32(0.0), ny)
        out[..., k], out[..., k + 1] = nx, ny
    return out
