"""Training-time episode statistics of ``DeviceRollout(stats=True)`` (``rr_rollout_collect_stats``):
what SB3 logs from Monitor-wrapped envs every iteration (``rollout/ep_rew_mean``,
``rollout/ep_len_mean``, ``train/explained_variance``), from the collect launch itself.

A statistics block is 16 slots of 8 bytes (``include/rocket_hip.h`` ``RR_RSTAT_*``): int64 counts
and fp64 sums / extremes. ``stats_dict`` turns one into the log dict and needs no GPU."""
import math

import numpy as np

from ._lib import (RR_RSTAT_D_SQ, RR_RSTAT_D_SUM, RR_RSTAT_END_BOUNDS, RR_RSTAT_END_EVENT, RR_RSTAT_END_NONFINITE,
                   RR_RSTAT_END_TRUNCATED, RR_RSTAT_EPISODES, RR_RSTAT_INT_SLOTS, RR_RSTAT_LANDED, RR_RSTAT_LEN_SUM,
                   RR_RSTAT_RET_MAX, RR_RSTAT_RET_MIN, RR_RSTAT_RET_SQ, RR_RSTAT_RET_SUM, RR_RSTAT_SAMPLES,
                   RR_RSTAT_SLOTS, RR_RSTAT_Y_SQ, RR_RSTAT_Y_SUM)

FLOAT_SLOTS = tuple(s for s in range(RR_RSTAT_SLOTS) if s not in RR_RSTAT_INT_SLOTS)


def empty_block():
    """The block of no collect at all: zeros, +inf / -inf in the min / max slots (what ``accum``
    starts a window with)."""
    b = np.zeros(RR_RSTAT_SLOTS, dtype=np.int64)
    f = b.view(np.float64)
    f[RR_RSTAT_RET_MIN], f[RR_RSTAT_RET_MAX] = np.inf, -np.inf
    return b


def make_block(ints=None, floats=None):
    """A block from {slot: int} and {slot: float} (tests, documentation)."""
    b = empty_block()
    for s, v in (ints or {}).items():
        assert s in RR_RSTAT_INT_SLOTS
        b[s] = v
    for s, v in (floats or {}).items():
        assert s in FLOAT_SLOTS
        b.view(np.float64)[s] = v
    return b


def fold_blocks(blocks):
    """The fold ``accum`` receives: blocks in order, sums add, min / max fold (fmin / fmax)."""
    acc = empty_block()
    af = acc.view(np.float64)
    for b in blocks:
        b = np.ascontiguousarray(b, dtype=np.int64)
        bf = b.view(np.float64)
        for s in range(RR_RSTAT_SLOTS):
            if s in RR_RSTAT_INT_SLOTS:
                acc[s] += b[s]
            elif s == RR_RSTAT_RET_MIN:
                af[s] = np.fmin(af[s], bf[s])
            elif s == RR_RSTAT_RET_MAX:
                af[s] = np.fmax(af[s], bf[s])
            else:
                af[s] = af[s] + bf[s]
    return acc


def stats_dict(block):
    """The log dict of one statistics block (16 x 8 bytes, any integer / float64 array of 16 words).

    With zero episodes the ``rollout/ep_*`` keys and the ending fractions are left out (SB3 logs
    nothing then); ``train/explained_variance`` is 1 - Var(d) / Var(y) over the samples, NaN where
    Var(y) is zero (SB3 ``explained_variance``)."""
    b = np.ascontiguousarray(block).reshape(-1)
    if b.size != RR_RSTAT_SLOTS or b.dtype.itemsize != 8:
        raise ValueError("a statistics block is 16 words of 8 bytes")
    i, f = b.view(np.int64), b.view(np.float64)
    ep = int(i[RR_RSTAT_EPISODES])
    out = {"rollout/episodes": ep}
    if ep > 0:
        mean = float(f[RR_RSTAT_RET_SUM]) / ep
        var = float(f[RR_RSTAT_RET_SQ]) / ep - mean * mean
        out["rollout/ep_rew_mean"] = mean
        out["rollout/ep_rew_std"] = math.sqrt(var) if var > 0.0 else (0.0 if var == var else math.nan)
        out["rollout/ep_rew_min"] = float(f[RR_RSTAT_RET_MIN])
        out["rollout/ep_rew_max"] = float(f[RR_RSTAT_RET_MAX])
        out["rollout/ep_len_mean"] = int(i[RR_RSTAT_LEN_SUM]) / ep
        out["rollout/success_rate"] = int(i[RR_RSTAT_LANDED]) / ep
        out["rollout/end_event"] = int(i[RR_RSTAT_END_EVENT]) / ep
        out["rollout/end_bounds"] = int(i[RR_RSTAT_END_BOUNDS]) / ep
        out["rollout/end_truncated"] = int(i[RR_RSTAT_END_TRUNCATED]) / ep
        out["rollout/end_nonfinite"] = int(i[RR_RSTAT_END_NONFINITE]) / ep
    n = int(i[RR_RSTAT_SAMPLES])
    ev = math.nan
    if n > 0:
        my, md = float(f[RR_RSTAT_Y_SUM]) / n, float(f[RR_RSTAT_D_SUM]) / n
        var_y = float(f[RR_RSTAT_Y_SQ]) / n - my * my
        var_d = float(f[RR_RSTAT_D_SQ]) / n - md * md
        if var_y > 0.0:
            ev = 1.0 - max(var_d, 0.0) / var_y
    out["train/explained_variance"] = ev
    return out


class RolloutStats:
    """The device blocks of a ``DeviceRollout(stats=True)``: ``out`` (the last collect's totals),
    ``accum`` (running totals since the last ``window()``) and the per-wave ``partials`` scratch.
    All are static tensors, so a captured collect keeps writing them."""

    def __init__(self, n_envs, device, lib):
        import torch

        rows = int(lib.rr_rollout_stats_rows(int(n_envs)))
        # 128-B aligned rows: torch's allocations are, but a slice of a pool need not be
        raw = torch.zeros(rows * RR_RSTAT_SLOTS + 16, dtype=torch.int64, device=device)
        skip = (-raw.data_ptr() % 128) // 8
        self._raw = raw
        self.partials = raw[skip: skip + rows * RR_RSTAT_SLOTS].view(rows, RR_RSTAT_SLOTS)
        self._empty = torch.from_numpy(empty_block()).to(device)
        self.out = self._empty.clone()
        self.accum = self._empty.clone()

    def struct(self):
        from . import _lib

        return _lib.RrRolloutStats(partials=self.partials.data_ptr(), out=self.out.data_ptr(),
                                   accum=self.accum.data_ptr())

    def last_block(self):
        return self.out.cpu().numpy()

    def last(self):
        """The last collect's figures (one copy back, one synchronisation)."""
        return stats_dict(self.last_block())

    def window_block(self):
        b = self.accum.cpu().numpy()
        self.accum.copy_(self._empty)  # in stream order: the next collect folds into an empty window
        return b

    def window(self):
        """The figures of every collect since the previous ``window()`` (or the start), then an
        empty window: a loop of captured collects can be read every k iterations."""
        return stats_dict(self.window_block())
