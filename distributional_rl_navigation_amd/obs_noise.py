"""Observation noise: what the robot perceives of an observation row (include/marinenav_hip.h, "Observation noise").

`ObsNoise` is the description -- a seed, additive sigmas for the DVL velocity and the goal, a relative range error per sonar beam and the probability
that a beam with a return reports none -- and `perturb` the rule itself as torch integer and float32 operations on any device: the CPU path, and a
second twin of the kernels (csrc/mn_obs_noise_body.h; mn_obs_perturb, and the NOISE forms of the episode kernels).  The perceived row is a pure function
of the clean float32 row and the key (seed, global env index, episode_timesteps when the observation was made): traces keep the clean rows, and
`perturb` re-derives what a policy saw.  `VecMarineNavEnv.set_obs_noise` / `.perturb` apply it on the device."""
import ctypes as C
import math
from dataclasses import dataclass

import torch

CHANNELS = 15
_GOLDEN = 0x9E3779B97F4A7C15
_ROW_KEY = 0xC2B2AE3D27D4EB4F
_CHANNEL_KEY = 0x165667B19E3779F9
_Z_SCALE = float.fromhex("0x1.bb67aep-16")      # float32(1 / sqrt((2^32 - 1) / 3))
_Z_CENTRE = 131070


class MnObsNoise(C.Structure):
    """mn_obs_noise (include/marinenav_hip.h)."""
    _fields_ = [("seed", C.c_uint64), ("vel_sigma", C.c_float), ("goal_sigma", C.c_float), ("sonar_rel_sigma", C.c_float), ("sonar_miss_p", C.c_float)]


@dataclass(frozen=True)
class ObsNoise:
    """seed: 64-bit key of the draws.  vel_sigma [m/s] and goal_sigma [m]: additive, one draw per component.  sonar_rel_sigma: relative range error, one
    draw per beam, both coordinates of the beam's point scaled by 1 + sonar_rel_sigma * z.  sonar_miss_p: probability that a beam with a return reports
    none.  z has mean 0, variance 1 and support +-3.464.  Validated here: a negative or non-finite sigma, or sonar_miss_p outside [0, 1], raises
    ValueError naming the parameter."""
    seed: int = 0
    vel_sigma: float = 0.0
    goal_sigma: float = 0.0
    sonar_rel_sigma: float = 0.0
    sonar_miss_p: float = 0.0

    def __post_init__(self):
        for name in ("vel_sigma", "goal_sigma", "sonar_rel_sigma"):
            v = float(getattr(self, name))
            if not (math.isfinite(v) and v >= 0.0 and math.isfinite(_f32(v))):
                raise ValueError(f"ObsNoise: {name} = {v!r} must be finite and not negative")
        p = float(self.sonar_miss_p)
        if not (0.0 <= p <= 1.0):
            raise ValueError(f"ObsNoise: sonar_miss_p = {p!r} must be in [0, 1]")

    @property
    def is_off(self):
        """Every channel off (as float32): the perceived row is the clean row, bit for bit."""
        return _f32(self.vel_sigma) == 0.0 and _f32(self.goal_sigma) == 0.0 and _f32(self.sonar_rel_sigma) == 0.0 and self.miss_threshold == 0

    @property
    def miss_threshold(self):
        """The 24-bit threshold the miss words are compared with: (uint32)(double(float32 p) * 2^24)."""
        return int(_f32(self.sonar_miss_p) * 16777216.0)

    def c_struct(self):
        return MnObsNoise(int(self.seed) & ((1 << 64) - 1), float(self.vel_sigma), float(self.goal_sigma), float(self.sonar_rel_sigma), float(self.sonar_miss_p))


def _f32(x):
    return C.c_float(float(x)).value


def _i64(x):
    """A 64-bit pattern as the Python int torch.int64 holds it."""
    x &= (1 << 64) - 1
    return x - (1 << 64) if x >= (1 << 63) else x


def _shr(x, k):
    """Logical right shift of int64 words."""
    return (x >> k) & ((1 << (64 - k)) - 1)


def _mix64(x):
    x = (x ^ _shr(x, 30)) * _i64(0xBF58476D1CE4E5B9)
    x = (x ^ _shr(x, 27)) * _i64(0x94D049BB133111EB)
    return x ^ _shr(x, 31)


def _word(key, c, w):
    return _mix64(key ^ _i64(_CHANNEL_KEY * (2 * c + w + 1)))


def _z(word):
    s = (word & 0xFFFF) + (_shr(word, 16) & 0xFFFF) + (_shr(word, 32) & 0xFFFF) + _shr(word, 48) - _Z_CENTRE
    return s.to(torch.float32) * torch.tensor(_Z_SCALE, dtype=torch.float32, device=word.device)


def perturb(obs, env_index, ep_t, noise):
    """The rows a policy is fed: `obs` [..., 26] float32 (clean), `env_index` / `ep_t` integer tensors of the leading shape (or broadcastable to it;
    Python ints are taken for every row) -- the GLOBAL env index and the env's episode_timesteps when the observation was made.  Integer words in int64
    (two's complement wrap-around is the uint64 arithmetic of the rule), float32 values, every product and sum rounded on its own.  Returns a new tensor."""
    if obs.dtype != torch.float32 or obs.shape[-1] != 26:
        raise ValueError("perturb: obs must be float32 [..., 26]")
    dev, lead = obs.device, obs.shape[:-1]
    out = obs.clone()
    if noise is None or noise.is_off:
        return out
    env = torch.as_tensor(env_index, device=dev).to(torch.int64)
    t = torch.as_tensor(ep_t, device=dev).to(torch.int64)
    base = _mix64(_i64(int(noise.seed)) + _i64(_GOLDEN) * (env + 1))
    key = _mix64(base ^ (_i64(_ROW_KEY) * (t + 1))).broadcast_to(lead)
    f32 = lambda v: torch.tensor(_f32(v), dtype=torch.float32, device=dev)      # noqa: E731
    thr = noise.miss_threshold
    for c in range(4):
        sigma = noise.vel_sigma if c < 2 else noise.goal_sigma
        if _f32(sigma) != 0.0:
            out[..., c] = obs[..., c] + f32(sigma) * _z(_word(key, c, 0))
    rel = _f32(noise.sonar_rel_sigma) != 0.0
    for b in range(11):
        c, k = 4 + b, 4 + 2 * b
        x, y = obs[..., k], obs[..., k + 1]
        hit = ~((x == 0) & (y == 0))
        miss = hit & (_shr(_word(key, c, 1), 40) < thr) if thr else torch.zeros_like(hit)
        nx, ny = x, y
        if rel:
            f = 1.0 + f32(noise.sonar_rel_sigma) * _z(_word(key, c, 0))
            scale = hit & ~miss
            nx, ny = torch.where(scale, x * f, x), torch.where(scale, y * f, y)
        zero = torch.zeros((), dtype=torch.float32, device=dev)
        out[..., k], out[..., k + 1] = torch.where(miss, zero, nx), torch.where(miss, zero, ny)
    return out
