"""fp64 restatements of the four detailed pose errors (mpjpe_byjoint, weighted_mpjpe, n_mpjpe, mean_velocity_error) and the
error bounds of a comparison with them, shared by tests/test_eval_detail_cpu.py and tests/test_gpu_eval_detail.py.  No
reference code and no data files are needed.

Every restatement takes the fp32 inputs, casts them to fp64 and returns SUMS (the functions' means are sum / count) with a
bound on |kernel sum - restated sum|.  None of the bounds is measured on the code under test.

Derivation (u = 2^-53 is the unit roundoff of fp64, so 2^-52 = 2u pays for one rounding on each of the two sides):

 * A distance |a - b| of fp32 values, in fp64: the differences are exact up to u each, three squares, two adds, one square
   root -- at most 4u relative on either side.  A sum of n non-negative terms, in any order, adds at most (n - 1) u relative
   to the sum.  Together (n + 3) u per side, and  (n + 8) 2^-52 |ref|  covers both sides with room for the second-order terms.
 * Terms with cancellation carry an ABSOLUTE error that |ref| does not see; it is bounded through A, the sum of the absolute
   values that enter the cancelling differences, by  8 * 2^-52 * A = 16 u A:
     - velocity, d = (p' - p) - (t' - t) per component: |err d| <= u (|p' - p| + |t' - t|) + u |d| <= 2u (|p'| + |p| + |t'| +
       |t|) per side, and a norm moves by at most the sum of its components' errors: 4u A for both sides, A = the sum of
       |p'| + |p| + |t'| + |t| over all pairs, joints and components.
     - N-MPJPE, d = s p - t per component with s = (sum t.p) / (sum p.p) over the pose's 48 components.  The kernel sums both dot
       products as a tree with at most 7 roundings on any path (scaled_errors_kernel, csrc/dhaug_eval_detail.hip), so
       |err s| <= (7 + 7 + 1) u S with S = (sum |t.p|) / (sum p.p) >= |s|: the scale over ABSOLUTE products, because the numerator
       may itself cancel.  Here the
       restatement forms the two dot products in extended precision and rounds s once (u S).  Per component then
       |err d| <= 15u S |p| + u |s p| + u |d| <= 17u S |p| + u |t| in the kernel and 3u S |p| + u |t| in the restatement, summed:
       20u S |p| + 2u |t|.  With A = the sum of S |p| + |t| over all joints and components this is <= 16 u A whenever
       sum S |p| <= 3.5 sum |t|, i.e. unless the rescaled prediction is several times LARGER than the target;
       scaled_sum() returns both sums and the tests assert the condition on their inputs.
     - signed weights, the sum of w e: each term carries 5u |w| e per side (the distance and one product), 10u A for both with
       A = the sum of |w| e.  The accumulation of a signed sum is bounded relative to A, not to |ref|: D u A per side, D the
       number of roundings on the longest path of the summation.  D <= n always, and D <= 80 at the sizes tested here: the
       kernel adds the 4 joints of at most 2 poses per lane up to P = 2 * 64 * 2048, then a 6-level butterfly, the 4 waves, at
       most 32 workgroup partials per lane and another butterfly (55); numpy sums pairwise.  So both sides stay within
       (2 min(n, 80) + 10) u A, which  (n + 8) 2^-52 |ref| + 16u A  covers while |ref| >= 0.9 A: then it is at least
       (1.8 n + 30.4) u A >= (2 min(n, 80) + 10) u A for every n.
       weighted_sum() returns A, and the tests that choose their own weights assert |ref| >= 0.9 A on them.
 * A result returned in fp32 is rounded once more: 2^-24 |ref|.
"""
import numpy as np

E52 = 2.0 ** -52
E24 = 2.0 ** -24


def center32(a):
    """(..., 16, 3) fp32 minus each pose's first joint, in fp32 (what center != 0 does)"""
    a = np.asarray(a, dtype=np.float32)
    return a - a[..., :1, :]


def distances(y, x):
    """fp64 joint distances |y - x| of fp32 (..., 3) inputs"""
    d = np.asarray(y, dtype=np.float64) - np.asarray(x, dtype=np.float64)
    return np.sqrt((d * d).sum(-1))


def sum_bound(ref, n):
    return (n + 8) * E52 * np.abs(ref)


def column_sums(y, x):
    """(rows, ..., 3) -> (sums over the rows per column, flattened to (cols,); their bounds)"""
    e = distances(y, x).reshape(y.shape[0], -1)
    ref = e.sum(0)
    return ref, sum_bound(ref, y.shape[0])


def velocity_sum(y, x):
    """(rows, ..., 3) -> (sum over consecutive row pairs and columns of |diff y - diff x|, its bound)"""
    y, x = np.asarray(y, dtype=np.float64), np.asarray(x, dtype=np.float64)
    d = (y[1:] - y[:-1]) - (x[1:] - x[:-1])
    ref = np.sqrt((d * d).sum(-1)).sum()
    A = (np.abs(y[1:]) + np.abs(y[:-1]) + np.abs(x[1:]) + np.abs(x[:-1])).sum()
    n = d.size // 3
    return ref, sum_bound(ref, n) + 8 * E52 * A


def weighted_sum(y, x, w):
    """w broadcast against the joint distances -> (sum of w e, its bound, A = sum of |w| e)"""
    e = distances(y, x)
    t = np.asarray(w, dtype=np.float64) * e
    assert t.shape == e.shape
    ref, A = t.sum(), np.abs(t).sum()
    return ref, sum_bound(ref, e.size) + 8 * E52 * A, A


def scaled_sum(y, x):
    """(..., 16, 3) -> (sum of |s y - x|, its bound, sum S |y|, sum |x|): per pose s = (sum x.y) / (sum y.y), the dot products in
    extended precision, everything else fp64"""
    y, x = np.asarray(y, dtype=np.float64).reshape(-1, 48), np.asarray(x, dtype=np.float64).reshape(-1, 48)
    yl, xl = y.astype(np.longdouble), x.astype(np.longdouble)
    with np.errstate(invalid="ignore", divide="ignore"):
        pp = (yl * yl).sum(1)
        s = ((xl * yl).sum(1) / pp).astype(np.float64)[:, None]
        S = (np.abs(xl * yl).sum(1) / pp).astype(np.float64)[:, None]
    d = (s * y - x).reshape(-1, 16, 3)
    ref = np.sqrt((d * d).sum(-1)).sum()
    Sy, ax = (S * np.abs(y)).sum(), np.abs(x).sum()
    return ref, sum_bound(ref, y.shape[0] * 16) + 8 * E52 * (Sy + ax), Sy, ax


FIXTURE_WEIGHTS = ("w_j4", "w_p4", "w_b4", "w_j3", "w_p3")


def fixture_forms(G, case):
    """the two input forms of a case of tests/golden/pose_eval_detail.npz: {"3": (128, 16, 3), "4": (32, 4, 16, 3)} pairs"""
    y, x = G[case + "_pred"], G[case + "_target"]
    return {"3": (y, x), "4": (y.reshape(32, 4, 16, 3), x.reshape(32, 4, 16, 3))}


def fixture_restated(G, case):
    """record name of the fixture -> (mean, bound of the mean) from the formulas above on the fixture's fp32 inputs"""
    F = fixture_forms(G, case)
    out = {}
    for d, (y, x) in F.items():
        ref, b = column_sums(y, x)
        out["bj" + d] = (ref.reshape(y.shape[1:-1]) / y.shape[0], b.reshape(y.shape[1:-1]) / y.shape[0])
        ref, b = velocity_sum(y, x)
        n = (y.shape[0] - 1) * int(np.prod(y.shape[1:-1]))
        out["v" + d] = (ref / n, b / n)
    for k in FIXTURE_WEIGHTS:
        y, x = F[k[-1]]
        ref, b, _ = weighted_sum(y, x, G[k])
        out[k.replace("_", "")] = (ref / (y.size // 3), b / (y.size // 3))
    y, x = F["4"]
    ref, b, Sy, ax = scaled_sum(y, x)
    assert Sy <= 3.5 * ax
    out["n4"] = (ref / (y.size // 3), b / (y.size // 3))
    return out
