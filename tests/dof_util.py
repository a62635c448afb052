"""The numpy restatement of the DOF angle distributions (dhaug_dof_histogram / dhaug_dof_pair_histogram) and the inputs of their
tests: np.trunc on the fp32 values for the bins, np.add.at for the integer counts, math.fsum for the fp64 sums."""
import math

import numpy as np

BINS = 361
F32 = np.float32


def bins_of(a):
    """(bin, nan, outside, inf) per fp32 value: bin = int(trunc(a)) + 180 inside, the end bin outside, -1 for a NaN"""
    a = np.asarray(a, dtype=F32)
    nan = np.isnan(a)
    inf = np.isinf(a)
    with np.errstate(invalid="ignore"):
        t = np.trunc(a.astype(np.float64))
        outside = ~nan & (inf | (np.abs(t) > 180))
    b = np.where(nan, -1, np.where(outside, np.where(np.signbit(a), 0, BINS - 1),
                                   np.where(nan | outside, 0, t).astype(np.int64) + 180))
    return b.astype(np.int64), nan, outside, inf


def kept_rows(rows, residual=None, max_residual=None):
    """the skip rule: residual <= max_residual keeps a row (equal is kept, a NaN residual is not)"""
    if residual is None:
        return np.ones(rows, dtype=bool)
    with np.errstate(invalid="ignore"):
        return np.asarray(residual, dtype=F32) <= F32(max_residual)


def _extreme(v, lowest):
    """exact fp32 min / max of the non-NaN values; of two zeros min keeps -0 and max +0; none -> +inf / -inf"""
    v = v[~np.isnan(v)]
    if v.size == 0:
        return F32(np.inf if lowest else -np.inf)
    m = v.min() if lowest else v.max()
    if m == 0:
        neg = bool(np.signbit(v[v == 0]).any()) if lowest else bool(np.signbit(v[v == 0]).all())
        return F32(-0.0) if neg else F32(0.0)
    return F32(m)


def histogram(angles, residual=None, max_residual=None, lo=None, hi=None, tol=0.0):
    """the whole record of one dof_histogram call on a fresh record, as a dict of numpy arrays; sum / sumsq by math.fsum, with
    sum_abs (the sum of |a|) next to them for the error bound"""
    a = np.asarray(angles, dtype=F32)
    rows, D = a.shape
    keep = kept_rows(rows, residual, max_residual)
    k = a[keep]
    b, nan, outside, inf = bins_of(k)
    counts = np.zeros((D, BINS), dtype=np.int64)
    cols = np.broadcast_to(np.arange(D), k.shape)
    np.add.at(counts, (cols[~nan], b[~nan]), 1)
    out = dict(rows=rows, skipped=int(rows - keep.sum()), counts=counts, nan=nan.sum(axis=0).astype(np.int64),
               outside=outside.sum(axis=0).astype(np.int64), inf=inf.sum(axis=0).astype(np.int64))
    if lo is not None:
        lo_t = (np.asarray(lo, dtype=F32) + F32(tol)).astype(F32)
        hi_t = (np.asarray(hi, dtype=F32) - F32(tol)).astype(F32)
        with np.errstate(invalid="ignore"):
            out["at_lo"] = (k <= lo_t).sum(axis=0).astype(np.int64)
            out["at_hi"] = (k >= hi_t).sum(axis=0).astype(np.int64)
    else:
        out["at_lo"] = out["at_hi"] = np.zeros(D, dtype=np.int64)
    out["min"] = np.array([_extreme(k[:, d], True) for d in range(D)], dtype=F32)
    out["max"] = np.array([_extreme(k[:, d], False) for d in range(D)], dtype=F32)
    fin = np.isfinite(k)
    k64 = k.astype(np.float64)
    out["n_finite"] = fin.sum(axis=0)
    out["sum"] = np.array([math.fsum(k64[fin[:, d], d]) for d in range(D)])
    out["sumsq"] = np.array([math.fsum(k64[fin[:, d], d] ** 2) for d in range(D)])      # a * a of an fp32 value is exact in fp64
    out["sum_abs"] = np.array([math.fsum(np.abs(k64[fin[:, d], d])) for d in range(D)])
    return out


def sum_bounds(ref):
    """|sum - fsum| <= n 2^-52 sum|a| and |sumsq - fsum| <= n 2^-52 sum a^2 per slot: the first-order bound of n - 1 roundings
    of relative size 2^-53 each, in any order, on partial sums that never exceed the sum of the magnitudes -- with a factor 2 to
    spare; derived, not measured"""
    n = ref["n_finite"].astype(np.float64)
    return n * 2.0 ** -52 * ref["sum_abs"], n * 2.0 ** -52 * ref["sumsq"]


def pair_tables(angles, pairs, residual=None, max_residual=None):
    a = np.asarray(angles, dtype=F32)
    k = a[kept_rows(a.shape[0], residual, max_residual)]
    b, nan, _, _ = bins_of(k)
    out = np.zeros((len(pairs), BINS, BINS), dtype=np.int64)
    for p, (i, j) in enumerate(pairs):
        ok = ~(nan[:, i] | nan[:, j])
        np.add.at(out[p], (b[ok, i], b[ok, j]), 1)
    return out


def ulp_step(x, up):
    return np.nextafter(F32(x), F32(np.inf if up else -np.inf)).astype(F32)


def trial_angles(rows, D, seed, specials=True, nans=True):
    """(rows, D) fp32: uniform in (-185, 185), mixed with exact integers, values 1 ulp either side of integers, -0.0, +-180,
    +-180.5, +-181, and (nans) NaN and +-inf"""
    g = np.random.default_rng(seed)
    a = g.uniform(-185.0, 185.0, size=(rows, D)).astype(F32)
    if not specials:
        return a
    kind = g.integers(0, 8, size=(rows, D))
    ints = g.integers(-182, 183, size=(rows, D)).astype(F32)
    a = np.where(kind == 1, ints, a)
    a = np.where(kind == 2, ulp_step(ints, True), a)
    a = np.where(kind == 3, ulp_step(ints, False), a)
    pool = [-0.0, 0.0, 180.0, -180.0, 180.5, -180.5, 181.0, -181.0, -0.5, 0.999, -180.9, 12.5]
    if nans:
        pool += [np.nan, np.inf, -np.inf]
    pick = np.asarray(pool, dtype=F32)[g.integers(0, len(pool), size=(rows, D))]
    return np.where(kind == 4, pick, a).astype(F32)
