"""DOF angle distributions kept on the device: what R/models_Fk_GAN/special_operate.py my_draw_DOF_angle_distribute (:347-364)
and my_draw_distribute_for_paper (:420-442) build in Python loops, as one accumulator over dhaug_dof_histogram /
dhaug_dof_pair_histogram (csrc/dhaug_dof.hip), plus the monitor that feeds it from the generator on the reference's schedule
(R/models_Fk_GAN/Fk_generator.py:172: the first and every 500th call).

Not here: circular statistics for slots that span +-180 degrees (mean / std are linear), bin widths other than the reference's
one degree, per-frame distributions of the video generator (its (B R, 37) rows are pooled)."""
import os

import numpy as np
import torch

from .. import _lib
from .. import ops

BINS = _lib.DOF_BINS


def monitor_enabled(args):
    """whether the model factories attach a DofMonitor: args.dof_monitor, or DHAUG_DOF_MONITOR=1; off by default"""
    return bool(getattr(args, "dof_monitor", False)) or os.environ.get("DHAUG_DOF_MONITOR", "") in ("1", "true", "yes")


class DofDistribution:
    """per-slot histograms (361 one-degree bins, bin = int(angle) + 180), pair histograms, moments and limit-saturation counts
    of (rows, D) angle tables, summed over batches in one device record; result() reads it once.

    pairs: slot pairs (i, j) whose 361 x 361 joint table is kept as well.  limits: a (lo, hi) pair of D entries each; at_lo /
    at_hi then count the values with a <= fl32(lo + tol) / a >= fl32(hi - tol).  add() enqueues its launches on the current
    stream and never synchronises.  Integer words are exact and the whole record is reproducible bit for bit (include/dhaug.h)."""

    def __init__(self, D=37, pairs=(), limits=None, tol=0.0, device=None):
        D = int(D)
        if not 1 <= D <= _lib.DOF_MAX_SLOTS:
            raise ValueError("DofDistribution: D must be in 1..%d, got %r" % (_lib.DOF_MAX_SLOTS, D))
        self.D = D
        try:
            self.pairs = [(int(i), int(j)) for i, j in pairs]
        except (TypeError, ValueError):
            raise ValueError("DofDistribution: pairs is a sequence of (i, j) slot pairs")
        bad = [p for p in self.pairs if not (0 <= p[0] < D and 0 <= p[1] < D)]
        if bad:
            raise ValueError("DofDistribution: slot(s) outside [0, %d) in %s" % (D, bad))
        if not float(tol) >= 0.0:
            raise ValueError("DofDistribution: tol must not be negative, got %r" % (tol,))
        self.tol = float(tol)
        lim = None
        if limits is not None:
            try:
                lo, hi = limits
                lim = [[float(v) for v in (x.detach().reshape(-1).cpu().tolist() if torch.is_tensor(x) else list(x))] for x in (lo, hi)]
            except (TypeError, ValueError):
                raise ValueError("DofDistribution: limits is a (lo, hi) pair of %d entries each" % D)
            if len(lim[0]) != D or len(lim[1]) != D:
                raise ValueError("DofDistribution: limits have %d entries each, got %d and %d" % (D, len(lim[0]), len(lim[1])))
            if any(not lim[0][i] <= lim[1][i] for i in range(D)):
                raise ValueError("DofDistribution: lo > hi at slot(s) %s" % [i for i in range(D) if not lim[0][i] <= lim[1][i]])
        self.device = torch.device(device if device is not None else "cuda")
        self.limits = None if lim is None else torch.tensor(lim, dtype=torch.float32, device=self.device)
        self.record = ops.dof_record(D, self.device)
        self.table = torch.zeros((len(self.pairs), BINS, BINS), dtype=torch.int64, device=self.device)

    def zero(self):
        self.record.copy_(ops.dof_record(self.D, self.device))
        self.table.zero_()
        return self

    def add(self, angles, residual=None, max_residual=None):
        """angles (rows, D) fp32 on the device (a row-strided view is read in place).  With residual (rows) and max_residual,
        rows whose residual is larger, or NaN, are left out and counted in `skipped`."""
        if not torch.is_tensor(angles) or angles.dim() != 2 or angles.shape[1] != self.D:
            raise ValueError("DofDistribution.add: angles must be a (rows, %d) tensor, got %s"
                             % (self.D, tuple(angles.shape) if torch.is_tensor(angles) else type(angles).__name__))
        lo, hi = (None, None) if self.limits is None else (self.limits[0], self.limits[1])
        ops.dof_histogram(angles, self.record, residual, max_residual, lo, hi, self.tol)
        for k in range(0, len(self.pairs), _lib.DOF_MAX_PAIRS):
            ops.dof_pair_histogram(angles, self.pairs[k:k + _lib.DOF_MAX_PAIRS], self.table[k:k + _lib.DOF_MAX_PAIRS], residual,
                                   max_residual)
        return self

    def result(self):
        """one host read -> dict of numpy arrays: counts (D, 361) int64, pair_counts (len(pairs), 361, 361) int64, rows, skipped
        (ints), nan, outside, inf, at_lo, at_hi (D,) int64, min, max (D,) fp32, mean, std (D,) fp64 over the FINITE values (population
        std; NaN for a slot without any)."""
        D, off = self.D, _lib.dof_record_offsets(self.D)
        w = self.record.cpu().numpy()
        f = w.view(np.float64)
        take = lambda a, k: a[off[k]:off[k] + D].copy()
        counts = w[off["counts"]:off["counts"] + D * BINS].reshape(D, BINS).copy()
        nan, outside = take(w, "nan"), take(w, "outside")
        mn, mx = take(f, "min"), take(f, "max")
        s, q = take(f, "sum"), take(f, "sumsq")
        n = (counts.sum(axis=1) - take(w, "inf")).astype(np.float64)       # the finite values: what sum / sumsq hold
        with np.errstate(invalid="ignore", divide="ignore"):
            mean = np.where(n > 0, s / n, np.nan)
            std = np.where(n > 0, np.sqrt(np.maximum(q / n - mean * mean, 0.0)), np.nan)
        return dict(counts=counts, pair_counts=self.table.cpu().numpy(), rows=int(w[off["rows"]]), skipped=int(w[off["skipped"]]),
                    nan=nan, outside=outside, inf=take(w, "inf"), at_lo=take(w, "at_lo"), at_hi=take(w, "at_hi"), min=mn.astype(np.float32),
                    max=mx.astype(np.float32), mean=mean, std=std)

    def normalised(self):
        """counts / counts.max(axis=1): the table the reference draws (a slot without counts gives NaN, as 0 / 0 does there)"""
        c = self.result()["counts"].astype(np.float64)
        with np.errstate(invalid="ignore", divide="ignore"):
            return c / c.max(axis=1, keepdims=True)

    def limits_from(self, coverage=0.999):
        """per slot the outer integer-degree edges (lo, hi) of the smallest central run of bins that holds `coverage` of the
        slot's counts: bins are dropped from whichever end holds fewer counts (the low end on a tie) while what is left still
        holds the share.  Returned as two lists that ik_limits / fit_pose(limits=...) accept; a slot without counts gives (0, 0)."""
        return limits_from_counts(self.result()["counts"], coverage)


def bin_edges(b):
    """the integer-degree interval [lo, hi] that bin b of the reference's table covers: bin 180 holds (-1, 1), a bin above it
    [b - 180, b - 179), a bin below it (b - 181, b - 180]"""
    if b == 180:
        return -1, 1
    return (b - 180, b - 179) if b > 180 else (b - 181, b - 180)


def limits_from_counts(counts, coverage=0.999):
    """host arithmetic of DofDistribution.limits_from on a (D, 361) table of counts"""
    if not 0.0 < float(coverage) <= 1.0:
        raise ValueError("limits_from: coverage must be in (0, 1], got %r" % (coverage,))
    counts = np.asarray(counts)
    if counts.ndim != 2 or counts.shape[1] != BINS:
        raise ValueError("limits_from: counts must be (D, %d), got %s" % (BINS, counts.shape))
    lo_out, hi_out = [], []
    for row in counts:
        total = int(row.sum())
        if total == 0:
            lo_out.append(0.0)
            hi_out.append(0.0)
            continue
        nz = np.nonzero(row)[0]
        a, b = int(nz[0]), int(nz[-1])
        # kept >= coverage * total, compared exactly: a float is a ratio of two integers
        num, den = float(coverage).as_integer_ratio()
        kept = total
        while a < b:
            end = a if row[a] <= row[b] else b
            if (kept - int(row[end])) * den < num * total:
                break
            kept -= int(row[end])
            if end == a:
                a += 1
                while row[a] == 0:
                    a += 1
            else:
                b -= 1
                while row[b] == 0:
                    b -= 1
        lo_out.append(float(bin_edges(a)[0]))
        hi_out.append(float(bin_edges(b)[1]))
    return lo_out, hi_out


class DofMonitor:
    """feeds a DofDistribution from a generator on the reference's schedule: due(train_num) is true for train_num % every == 1
    (R/models_Fk_GAN/Fk_generator.py:172, the first and every `every`-th call; every=1 means every call)."""

    def __init__(self, distribution, every=500):
        every = int(every)
        if every < 1:
            raise ValueError("DofMonitor: every must be at least 1, got %r" % (every,))
        if not isinstance(distribution, DofDistribution):
            raise ValueError("DofMonitor: distribution must be a DofDistribution")
        self.distribution = distribution
        self.every = every

    def due(self, train_num):
        return int(train_num) % self.every == 1 % self.every

    def feed(self, angles):
        self.distribution.add(angles)


def generator_monitor(every=500, device=None):
    """the monitor the model factories attach: 37 slots, the generator's limits, the paper's pair (8, 3)"""
    return DofMonitor(DofDistribution(37, pairs=((8, 3),), limits=(ops.IK_GENERATOR_LO, ops.IK_GENERATOR_HI), device=device), every)
