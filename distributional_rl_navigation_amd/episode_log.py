"""The per-episode record of TRAINING, kept on the device (C-ABI mn_episode_log, csrc/mn_episode_log.hip).

The reference prints a block at every training episode end -- length, discounted return, result, exploration rate, timestep
(thirdparty/IQN/agent.py:152-165) -- the only view of training between two evaluations.  The batched loops could give it only with
`learn_vec(verbose=True)`, five host synchronisations per vector step.  Here one small launch per vector step advances every env's
running (return, discount, length) and appends one record per finished episode to device arrays; the host looks at them once per
evaluation interval, through an asynchronous copy it only reads at the NEXT drain: a run without a host synchronisation gets none
from the log.

* `EpisodeLog`: the device state, `step()` per vector step, `drain()` per evaluation point, `close()` at the end; one summary row
  per evaluation interval (`rows`, `save`), with `full=True` the raw records too (`episodes()`).
* `replay_traces`: the numpy twin -- the same records from [T][n] traces, the same operation order in float64.  What the GPU test
  compares against and what runs on a machine without a GPU.

The return of a record is the running-product form  ret += disc * reward; disc *= discount  -- not the reference's
`discount ** ep_length` power (documented in include/marinenav_hip.h).  Records are kept in the canonical order (step, env).
"""
import ctypes as C

import numpy as np

RECORD_FIELDS = (("step", np.int64), ("env", np.int32), ("length", np.int32), ("info", np.uint8), ("ret", np.float64), ("eps", np.float32))
N_INFO = 5      # MN_INFO_NORMAL ... MN_INFO_REACH_GOAL (include/marinenav_hip.h)
SUMMARY_FIELDS = ("timestep", "episodes", "info_counts", "return_mean", "return_std", "length_mean", "eps_mean")


def empty_records():
    return {k: np.zeros(0, dtype=t) for k, t in RECORD_FIELDS}


def canonical(rec):
    """`rec` (dict of equally long arrays, RECORD_FIELDS) in the canonical order: by step, then by env."""
    order = np.lexsort((rec["env"], rec["step"]))
    return {k: np.ascontiguousarray(np.asarray(rec[k])[order], dtype=t) for k, t in RECORD_FIELDS}


def concat_records(chunks):
    chunks = list(chunks)
    if not chunks:
        return empty_records()
    return {k: np.concatenate([c[k] for c in chunks]).astype(t, copy=False) for k, t in RECORD_FIELDS}


def summarize(rec, timestep):
    """One summary row of the records `rec`: the last timestep of the interval, the number of episodes, how many ended with each
    MN_INFO_* code, mean and (population) std of the return, mean length, mean exploration rate.  Means of no episode are nan."""
    k = int(len(rec["step"]))
    f = lambda a: float(np.mean(np.asarray(a, dtype=np.float64))) if k else float("nan")
    return dict(timestep=int(timestep), episodes=k, info_counts=np.bincount(np.asarray(rec["info"], dtype=np.int64), minlength=N_INFO)[:N_INFO].astype(np.int64),
                return_mean=f(rec["ret"]), return_std=float(np.std(np.asarray(rec["ret"], dtype=np.float64))) if k else float("nan"),
                length_mean=f(rec["length"]), eps_mean=f(rec["eps"]))


def rows_to_arrays(rows):
    """The summary rows as the arrays of training_log.npz."""
    return dict(timesteps=np.array([r["timestep"] for r in rows], dtype=np.int64), episodes=np.array([r["episodes"] for r in rows], dtype=np.int64),
                info_counts=np.array([r["info_counts"] for r in rows], dtype=np.int64).reshape(len(rows), N_INFO),
                **{k: np.array([r[k] for r in rows], dtype=np.float64) for k in ("return_mean", "return_std", "length_mean", "eps_mean")})


def replay_traces(reward, done, info, discount, eps, first_step=0, state=None):
    """The records `EpisodeLog.step` writes for the traces reward / done / info [T][n] of T vector steps (step t has index first_step + t and
    exploration rate eps[t]), in canonical order, by the kernel's own arithmetic: float64, one rounding per operation, in its order.
    Returns (records, state) with state = (ret [n] f64, disc [n] f64, length [n] i32) behind the last step; `state` continues an earlier call."""
    reward, done, info = np.asarray(reward), np.asarray(done), np.asarray(info)
    T, n = reward.shape
    eps = np.broadcast_to(np.asarray(eps, dtype=np.float32), (T,))
    discount = np.float64(discount)
    if state is None:
        ret, disc, length = np.zeros(n, np.float64), np.ones(n, np.float64), np.zeros(n, np.int32)
    else:
        ret, disc, length = (np.array(s, copy=True) for s in state)
    chunks = []
    for t in range(T):
        ret = ret + disc * reward[t].astype(np.float64)
        disc = disc * discount
        length = length + np.int32(1)
        fin = np.flatnonzero(np.asarray(done[t]) != 0)
        if len(fin):
            chunks.append(dict(step=np.full(len(fin), first_step + t, np.int64), env=fin.astype(np.int32), length=length[fin].copy(),
                               info=np.asarray(info[t])[fin].astype(np.uint8), ret=ret[fin].copy(), eps=np.full(len(fin), eps[t], np.float32)))
            ret[fin], disc[fin], length[fin] = 0.0, 1.0, 0
    return canonical(concat_records(chunks)), (ret, disc, length.astype(np.int32))


class EpisodeLogOverflow(RuntimeError):
    pass


class EpisodeLog:
    """Device-side episode log of `n` envs stepped side by side.

    `step(reward, done, info, step_index, eps)` enqueues ONE launch on the current stream (mn_episode_log).  `drain(timestep)` enqueues the
    copy of the counter and of the slots that can be in use to pinned host memory, zeroes the counter on the stream and returns at once; the
    copy is read at a later drain, once its event has passed, or at `close()`.  Every `drain(..., row=True)` closes one summary row
    (`summarize`) over what was recorded since the last one.
    `capacity`: record slots between two drains.  An env ends at most one episode per vector step, so n x (vector steps between drains)
    cannot overflow; `max_steps_between_drains` is that bound for this capacity and `due()` says when it is reached.  A counter beyond the
    capacity makes the drain that reads it raise `EpisodeLogOverflow` with both numbers.
    `full`: keep the raw records too (`episodes()`: canonical order)."""

    def __init__(self, n, capacity, discount, device, full=False):
        import torch
        from . import _capi
        self.L = _capi.lib()
        self.n, self.capacity, self.discount, self.full = int(n), int(capacity), float(discount), bool(full)
        assert self.n >= 1 and self.capacity >= 1
        self.device = dev = torch.device(device)
        self.ep_ret = torch.zeros(self.n, dtype=torch.float64, device=dev)
        self.ep_disc = torch.ones(self.n, dtype=torch.float64, device=dev)
        self.ep_len = torch.zeros(self.n, dtype=torch.int32, device=dev)
        self.count = torch.zeros(1, dtype=torch.int32, device=dev)      # (the kernel's u32)
        self.rec = self._record_tensors(self.capacity, dev, False)
        self.max_steps_between_drains = max(1, self.capacity // self.n)
        self.steps_since_drain = 0
        self.row_open = False     # steps were logged since the last drain that closed a summary row
        self._in_flight = []      # (host count, host records, slots copied, event, timestep, closes a row) in drain order
        self._free = []
        self._interval = []       # record chunks of the open summary row
        self.rows = []
        self._all = []            # `full`: every chunk
        self.dropped = 0

    @staticmethod
    def _record_tensors(k, device, pinned):
        import torch
        kw = dict(device=device, pin_memory=True) if pinned else dict(device=device)
        tt = dict(step=torch.int64, env=torch.int32, length=torch.int32, info=torch.uint8, ret=torch.float64, eps=torch.float32)
        return {name: torch.zeros(k, dtype=tt[name], **kw) for name, _ in RECORD_FIELDS}

    def step(self, reward, done, info, step_index, eps):
        """One vector step: reward [n] f32, done / info [n] u8 device tensors (a step's outputs), the step's index and exploration rate."""
        from ._capi import check, stream_ptr
        assert reward.dtype.is_floating_point and reward.element_size() == 4 and done.element_size() == 1 and info.element_size() == 1
        assert reward.numel() == self.n and done.numel() == self.n and info.numel() == self.n
        assert reward.is_contiguous() and done.is_contiguous() and info.is_contiguous()
        r, p = self.rec, lambda t: C.c_void_p(t.data_ptr())
        check(self.L.mn_episode_log(p(reward), p(done), p(info), self.n, self.discount, int(step_index), float(eps), p(self.ep_ret), p(self.ep_disc),
                                    p(self.ep_len), p(r["step"]), p(r["env"]), p(r["length"]), p(r["info"]), p(r["ret"]), p(r["eps"]), self.capacity,
                                    p(self.count), stream_ptr(self.device)))
        self.steps_since_drain += 1
        self.row_open = True

    def due(self):
        """True once another `step` without a drain could overflow the record arrays."""
        return self.steps_since_drain >= self.max_steps_between_drains

    def drain(self, timestep, row=True, wait=False):
        """Enqueue the copy of what was recorded since the last drain (no host wait) and take in the earlier copies that have arrived.
        `timestep`: the last timestep of the chunk; `row`: the chunk closes a summary row; `wait`: look at this copy now (synchronises)."""
        import torch
        k = min(self.capacity, self.n * self.steps_since_drain)
        host = self._free.pop() if self._free else (torch.zeros(1, dtype=torch.int32, pin_memory=True), self._record_tensors(self.capacity, "cpu", True))
        host[0].copy_(self.count, non_blocking=True)
        for name in host[1]:
            if k:
                host[1][name][:k].copy_(self.rec[name][:k], non_blocking=True)
        self.count.zero_()
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(self.device))
        self._in_flight.append((host, k, ev, int(timestep), bool(row)))
        self.steps_since_drain = 0
        if row:
            self.row_open = False
        self._collect(wait=bool(wait))

    def _collect(self, wait):
        while self._in_flight and (wait or self._in_flight[0][2].query()):
            host, k, ev, timestep, row = self._in_flight.pop(0)
            if wait:
                ev.synchronize()
            count = int(host[0].numpy().view(np.uint32)[0])
            if count > self.capacity:
                self.dropped += count - self.capacity
                raise EpisodeLogOverflow(f"episode log overflow: {count} episodes ended since the last drain, the record arrays hold {self.capacity} "
                                         f"({count - self.capacity} records dropped)")
            assert count <= k
            self._take(canonical({name: host[1][name][:count].numpy().copy() for name, _ in RECORD_FIELDS}), timestep, row)
            self._free.append(host)

    def _take(self, chunk, timestep, row):
        self._interval.append(chunk)
        if self.full:
            self._all.append(chunk)
        if row:
            self.rows.append(summarize(concat_records(self._interval), timestep))
            self._interval = []

    def close(self):
        """Wait for the copies still in flight and take them in.  Returns the summary rows."""
        self._collect(wait=True)
        return self.rows

    def episodes(self):
        """`full`: every drained record so far, canonical order."""
        assert self.full, "EpisodeLog(full=True) keeps the raw records"
        return canonical(concat_records(self._all))

    def state(self):
        """(ret, disc, length) of the running episodes as numpy (synchronises)."""
        return self.ep_ret.cpu().numpy(), self.ep_disc.cpu().numpy(), self.ep_len.cpu().numpy()

    # ---- checkpoints ---------------------------------------------------------------------------
    def state_dict(self):
        """The log as CPU tensors, numpy arrays and plain numbers: the running episodes' accumulators, the counter and the record slots in use since the last
        drain (device side), the open summary row's chunks, the closed rows and -- `full` -- every record taken so far (host side).  The copies still in
        flight are waited for and taken in first, in drain order, exactly as a later drain would take them."""
        self._collect(wait=True)
        k = min(self.capacity, self.n * self.steps_since_drain)
        return dict(n=self.n, capacity=self.capacity, full=self.full, ep_ret=self.ep_ret.cpu(), ep_disc=self.ep_disc.cpu(), ep_len=self.ep_len.cpu(),
                    count=self.count.cpu(), rec={name: self.rec[name][:k].cpu() for name, _ in RECORD_FIELDS}, steps_since_drain=int(self.steps_since_drain),
                    row_open=bool(self.row_open), interval=[dict(c) for c in self._interval], rows=[dict(r) for r in self.rows],
                    all=[dict(c) for c in self._all], dropped=int(self.dropped))

    def load_state_dict(self, sd):
        if (int(sd["n"]), int(sd["capacity"]), bool(sd["full"])) != (self.n, self.capacity, self.full):
            raise ValueError(f"EpisodeLog.load_state_dict: the state is of a log of {sd['n']} envs, {sd['capacity']} slots, full={sd['full']}; this one has "
                             f"{self.n}, {self.capacity}, full={self.full}")
        self._collect(wait=True)
        self.ep_ret.copy_(sd["ep_ret"]); self.ep_disc.copy_(sd["ep_disc"]); self.ep_len.copy_(sd["ep_len"]); self.count.copy_(sd["count"])
        for name, _ in RECORD_FIELDS:
            k = sd["rec"][name].numel()
            self.rec[name][:k].copy_(sd["rec"][name])
        self.steps_since_drain, self.row_open, self.dropped = int(sd["steps_since_drain"]), bool(sd["row_open"]), int(sd["dropped"])
        self._interval, self.rows, self._all = [dict(c) for c in sd["interval"]], [dict(r) for r in sd["rows"]], [dict(c) for c in sd["all"]]

    def save(self, directory):
        """training_log.npz (the summary rows) and, with `full`, training_episodes.npz (the records, canonical order) in `directory`."""
        import os
        np.savez(os.path.join(directory, "training_log.npz"), **rows_to_arrays(self.rows))
        if self.full:
            np.savez(os.path.join(directory, "training_episodes.npz"), **self.episodes())
