"""`mn_episode_log` / `episode_log.EpisodeLog`: the training-episode record kept on the device must be, bit for bit, what the numpy twin
`episode_log.replay_traces` computes from the same traces -- records (canonical order), running state and counter -- for a partial last
wavefront, a single env and one full wavefront; and an overflowing log must count what it drops, write nothing past its capacity and say so."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
T, MAX_EPISODE_STEPS = 160, 40
EPS = np.linspace(1.0, 0.05, T).astype(np.float32)


@pytest.fixture(scope="module")
def torch():
    import torch as t
    if not t.cuda.is_available():
        pytest.skip("no GPU")
    return t


_traces = {}


def traces(torch, n):
    """T random-policy vector steps of n envs (episodes of at most 40 steps), computed once per n and shared: device traces, numpy traces, the twin's result."""
    if n not in _traces:
        from distributional_rl_navigation_amd.episode_log import replay_traces
        from distributional_rl_navigation_amd.marinenav_env.vec_env import VecMarineNavEnv
        env = VecMarineNavEnv(n, seed=5, device=DEV, precision="f64")
        env.params.max_episode_steps = MAX_EPISODE_STEPS
        env.set_attrs(num_cores=8, num_obs=10, min_start_goal_dis=40.0)
        env.reset()
        tr = env.rollout(T, action_seed=17, trace=("reward", "done", "info"))
        dev = {k: tr[k].clone() for k in ("reward", "done", "info")}
        host = {k: v.cpu().numpy() for k, v in dev.items()}
        discount = env.discount
        env.close()
        _traces[n] = (dev, host, discount, replay_traces(host["reward"], host["done"], host["info"], discount, EPS))
    return _traces[n]


def feed(log, dev):
    for t in range(T):
        log.step(dev["reward"][t], dev["done"][t], dev["info"][t], t, float(EPS[t]))


def assert_same_records(got, want):
    assert set(got) == set(want)
    for k in want:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
    assert np.array_equal(got["ret"].view(np.int64), want["ret"].view(np.int64))
    assert np.array_equal(got["eps"].view(np.int32), want["eps"].view(np.int32))
    for k in ("step", "env", "length", "info"):
        assert np.array_equal(got[k], want[k]), k


@pytest.mark.parametrize("n", [200, 1, 64])      # three full wavefronts and one of eight lanes; one lane; exactly one wavefront
def test_records_state_and_counter_equal_the_numpy_twin(torch, n):
    from distributional_rl_navigation_amd.episode_log import EpisodeLog, summarize
    dev, host, discount, (want, want_state) = traces(torch, n)
    # conditions on the input: every env finished an episode, and not every episode ended the same way
    assert (host["done"] != 0).any(axis=0).all()
    if n == 200:
        assert len(np.unique(host["info"][host["done"] != 0])) >= 2
    total = int((host["done"] != 0).sum())
    assert len(want["step"]) == total
    log = EpisodeLog(n, n * T, discount, DEV, full=True)
    feed(log, dev)
    assert int(log.count.cpu().numpy().view(np.uint32)[0]) == total
    log.drain(T * n)
    rows = log.close()
    assert_same_records(log.episodes(), want)
    for got, ref in zip(log.state(), want_state):
        assert got.dtype == ref.dtype
        assert np.array_equal(got.view(np.int64) if got.dtype == np.float64 else got, ref.view(np.int64) if ref.dtype == np.float64 else ref)
    assert int(log.count.cpu()[0]) == 0      # the drain zeroed the counter
    assert len(rows) == 1 and rows[0]["episodes"] == total and rows[0]["timestep"] == T * n
    ref_row = summarize(want, T * n)
    assert np.array_equal(rows[0]["info_counts"], ref_row["info_counts"]) and rows[0]["return_mean"] == ref_row["return_mean"]


def test_two_drains_give_two_rows_and_the_same_records(torch):
    from distributional_rl_navigation_amd.episode_log import EpisodeLog
    dev, host, discount, (want, _) = traces(torch, 200)
    log = EpisodeLog(200, 200 * (T // 2), discount, DEV, full=True)
    for t in range(T):
        log.step(dev["reward"][t], dev["done"][t], dev["info"][t], t, float(EPS[t]))
        if t + 1 in (T // 2, T):
            assert log.due()
            log.drain((t + 1) * 200)
    rows = log.close()
    assert_same_records(log.episodes(), want)
    assert [r["timestep"] for r in rows] == [T // 2 * 200, T * 200]
    assert [r["episodes"] for r in rows] == [int((host["done"][:T // 2] != 0).sum()), int((host["done"][T // 2:] != 0).sum())]


def test_overflow_counts_what_it_drops_and_writes_nothing_past_capacity(torch):
    from distributional_rl_navigation_amd import _capi
    from distributional_rl_navigation_amd.episode_log import EpisodeLog, EpisodeLogOverflow
    n = 200
    dev, host, discount, (want, _) = traces(torch, n)
    total = len(want["step"])
    cap, guard = total // 2, 256
    L = _capi.lib()
    p = lambda t: C.c_void_p(t.data_ptr())
    ret, disc, length = torch.zeros(n, dtype=torch.float64, device=DEV), torch.ones(n, dtype=torch.float64, device=DEV), torch.zeros(n, dtype=torch.int32, device=DEV)
    count = torch.zeros(1, dtype=torch.int32, device=DEV)
    kinds = dict(step=torch.int64, env=torch.int32, length=torch.int32, info=torch.uint8, ret=torch.float64, eps=torch.float32)
    SENT = 0x5A
    rec = {k: torch.full(((cap + guard) * torch.empty(0, dtype=dt).element_size(),), SENT, dtype=torch.uint8, device=DEV) for k, dt in kinds.items()}
    for t in range(T):
        _capi.check(L.mn_episode_log(p(dev["reward"][t]), p(dev["done"][t]), p(dev["info"][t]), n, discount, t, float(EPS[t]), p(ret), p(disc), p(length),
                                     p(rec["step"]), p(rec["env"]), p(rec["length"]), p(rec["info"]), p(rec["ret"]), p(rec["eps"]), cap, p(count),
                                     _capi.stream_ptr(torch.device(DEV))))
    assert int(count.cpu().numpy().view(np.uint32)[0]) == total      # the counter keeps counting: total - cap records were dropped
    got = {}
    for k, dt in kinds.items():
        size = torch.empty(0, dtype=dt).element_size()
        raw = rec[k].cpu()
        assert bool((raw[cap * size:] == SENT).all()), k                # the region behind slot `cap` is untouched
        got[k] = raw[:cap * size].view(dt).numpy()
    # every written slot is one of the twin's records, none twice
    key = lambda r, i: (int(r["step"][i]), int(r["env"][i]))
    index = {key(want, i): i for i in range(total)}
    seen = set()
    for i in range(cap):
        j = index[key(got, i)]
        assert j not in seen
        seen.add(j)
        assert got["length"][i] == want["length"][j] and got["info"][i] == want["info"][j]
        assert got["ret"][i:i + 1].view(np.int64)[0] == want["ret"][j:j + 1].view(np.int64)[0] and got["eps"][i] == want["eps"][j]
    # the class says so with both numbers
    log = EpisodeLog(n, cap, discount, DEV)
    feed(log, dev)
    with pytest.raises(EpisodeLogOverflow, match=f"{total} .* {cap}"):
        log.drain(T * n, wait=True)
