"""fp64 restatements of the three criteria kernels (dhaug_pose_nmpjpe, dhaug_pose_wmpjpe, dhaug_pose_byjoint_backward: loss and
gradient, with the zero-residual rule) and the bounds of a comparison with them, shared by tests/test_pose_criteria_cpu.py,
tests/test_gpu_pose_criteria_kernels.py and tests/test_gpu_pose_criteria.py.  Nothing here imports the package under test, and
none of the bounds is measured on it.

The bounds.  u = 2^-53 is the unit roundoff of fp64, ulp32(v) the spacing of fp32 at |v|.

 * The weighted and the per-joint gradient, w d / (e J) and cot d / (e rows), and all three losses: a handful of fp64 operations
   on exact differences of fp32 values (relative error a few u, or n u for a loss of n non-negative terms) followed by ONE
   rounding to fp32 (half an ulp).  Bound: 1 ulp32 at the fp64 value -- as argued in tests/test_gpu_posetrain_mpjpe.py.  (The
   weighted LOSS is a signed sum of n terms: its accumulated error is at most n u sum |w| e, which stays below a quarter of an
   ulp32 of the result, 2^-26 |sum w e|, while |sum w e| / sum |w| e >= n 2^-27.  The tests assert that on their inputs:
   weighted_sum_survives().)

 * The N-MPJPE gradient  g_k J = s u_k + c b_k,  c = a / pp,  b_k = t_k - 2 s p_k,  is a difference of two terms and can be small by
   cancellation, so besides 1 ulp32 at the fp64 value it gets an ABSOLUTE term  K u T_k / J,  K = 48: the number of roundings a
   48-term dot product can put on one path (one product, 47 additions; any summation order, the kernel's tree and numpy's
   pairwise sums included).  First-order error of one side, with
       S = sum |t.p| / pp >= |s|,   A = sum |u.p| >= |a|,   m_k = S |p_k| + |t_k|,   M_j = the sum of m_k over joint j's 3 components,
       rho_j = M_j / e_j  (how much larger the cancelling terms of r_j are than the residual),   R = sum_k rho_j(k) |p_k|,
       B_k = |t_k| + 2 S |p_k| >= |b_k|:
     1. |d pp| <= K u pp and |d tp| <= K u sum |t.p|, so |d s| <= (2K + 1) u S  (the quotient adds one u).
     2. r_k = s p_k - t_k: |d r_k| <= |d s| |p_k| + 2u (|s p_k| + |t_k|) <= (2K + 3) u m_k.
     3. e_j = |r_j|: |d e_j| <= sum_j |d r_k| + 3u e_j.  u_k = r_k / e_j with |u_k| <= 1:
        |d u_k| <= |d r_k| / e_j + |u_k| |d e_j| / e_j + u |u_k| <= (2K + 3) u (2 rho_j + |u_k|).
     4. a = sum u.p over 48 terms: |d a| <= sum |d u_k| |p_k| + K u A <= (3K + 3) u (A + 2R).
     5. c = a / pp: |d c| <= (|d a| + (K + 1) u |a|) / pp <= (4K + 4) u (A + 2R) / pp.
     6. b_k: |d b_k| <= 2 |d s| |p_k| + 2u |s p_k| + u |b_k| <= (2K + 3) u B_k.
     7. g_k J: |d s| |u_k| + |s| |d u_k| + |d c| |b_k| + |c| |d b_k| + 3u (|s u_k| + |c b_k|)
               <= (6K + 10) u [S (|u_k| + rho_j) + (A + 2R) B_k / pp].
   Two sides (the kernel and this restatement): (12K + 20) u [...] <= 13 K u [...] for K >= 20.  So
       T_k = 13 [S (|u_k| + rho_j) + (A + 2R) B_k / pp]
   -- the formula's terms with magnitudes, sum |t.p|, sum p.p and sum |u.p| standing for the dot products, plus rho where a unit
   vector is formed from a cancelling difference.  The division by J and the rounding to fp32 are the ulp32 term.  A joint with
   e_j == 0 has rho_j = inf: the bound says nothing about its pose, and the tests assert such poses exactly (all-zero rows).
"""
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "pose_criteria.npz")

U53 = 2.0 ** -53
K_SUM = 48                                      # roundings on one path of a 48-term dot product
SHAPES = ((1, 1, 16, 3), (5, 3, 16, 3), (2, 9, 16, 3))          # group (a) of the golden file
LOOPS = ("video", "gan")
CRITERIA = ("n", "w16")                         # group (b): the reference's n_mpjpe, and weighted_mpjpe with LOOP_W16 expanded
# wrists and ankles weighted up, knees and elbows half as much (the 16-joint H36M order: 0 hip, 1-3 / 4-6 legs, 7-9 spine to
# head, 10-12 / 13-15 arms)
LOOP_W16 = np.array([1, 1, 1.5, 2, 1, 1.5, 2, 1, 1, 1, 1, 1.5, 2, 1, 1.5, 2], dtype=np.float32)


def load_golden():
    z = np.load(GOLDEN)
    return {k: z[k] for k in z.files}


def loop_view(G, clips, criterion, loop):
    """group (b) of one criterion and loop under the key names posetrain_util's helpers read (<loop>_init_<key>,
    <loop>_final_<key>, <loop>_losses, <loop>_norms, v_b3d, v_b2d); clips: posetrain_mpjpe_util.load_golden()"""
    out = dict(v_b3d=clips["v_b3d"], v_b2d=clips["v_b2d"])
    pre = "%s_%s_" % (criterion, loop)
    for k, a in G.items():
        if k.startswith("init_"):
            out["%s_%s" % (loop, k)] = a
        elif k.startswith(pre):
            out["%s_%s" % (loop, k[len(pre):])] = a
    return out


def ulp32(ref64):
    """the spacing of fp32 at |ref|"""
    return np.spacing(np.abs(np.asarray(ref64, dtype=np.float64)).astype(np.float32)).astype(np.float64)


def make_case(shape, seed):
    """fp32 inputs of one case: pred, target, a per-pose weight (..., 1), a per-joint weight (...), a 16-vector weight and a
    per-joint cotangent shape[1:-1]; the weights' signs are mixed -- every fifth weight is negative -- so that they stay positive
    on balance (see weighted_cancellation)"""
    rng = np.random.default_rng(seed)
    f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    signed = lambda s: f32(rng.uniform(0.5, 2.0, s) * np.where(np.arange(int(np.prod(s))).reshape(s) % 5 == 4, -1.0, 1.0))
    target = f32(rng.normal(0, 1.0, shape))
    pred = f32(target * rng.uniform(0.6, 1.6, shape[:-2] + (1, 1)) + rng.normal(0, 0.3, shape))
    return dict(pred=pred, target=target, w_pose=signed(shape[:-2] + (1,)), w_joint=signed(shape[:-1]), w16=signed((16,)),
                cot=f32(rng.normal(0, 1.0, shape[1:-1])))


def nmpjpe(y, x, dtype=np.float64):
    """(loss, grad, T) of N-MPJPE over (..., 16, 3) poses evaluated in `dtype` from the fp32 values: grad exactly 0 contributions
    from joints with e == 0; T the per-element magnitude of the module docstring (fp64)"""
    shape = np.shape(y)
    y, x = np.asarray(y).astype(dtype).reshape(-1, 48), np.asarray(x).astype(dtype).reshape(-1, 48)
    J = dtype(16 * y.shape[0])
    with np.errstate(invalid="ignore", divide="ignore"):
        pp, tp = (y * y).sum(1, keepdims=True), (x * y).sum(1, keepdims=True)
        s = tp / pp
        r = (s * y - x).reshape(-1, 16, 3)
        e = np.sqrt((r * r).sum(-1, keepdims=True))
        u = np.where(e == 0, dtype(0), r / e).reshape(-1, 48)
        a = (u * y).sum(1, keepdims=True)
        grad = (s * u + (a / pp) * (x - 2 * s * y)) / J
        loss = e.sum() / J
        # the magnitudes
        S = np.abs(x * y).sum(1, keepdims=True) / pp
        A = np.abs(u * y).sum(1, keepdims=True)
        m = (S * np.abs(y) + np.abs(x)).reshape(-1, 16, 3)
        rho = np.broadcast_to(m.sum(-1, keepdims=True) / e, m.shape).reshape(-1, 48)
        R = (rho * np.abs(y)).sum(1, keepdims=True)
        B = np.abs(x) + 2 * S * np.abs(y)
        T = 13 * (S * (np.abs(u) + rho) + (A + 2 * R) * B / pp)
    return loss, grad.reshape(shape), np.asarray(T, dtype=np.float64).reshape(shape)


def nmpjpe_abs_term(T, poses):
    """K u T_k / J"""
    return K_SUM * U53 * T / (16.0 * poses)


def nmpjpe_bound(grad64, T, poses):
    return ulp32(grad64) + nmpjpe_abs_term(T, poses)


def wmpjpe(y, x, w):
    """(loss, grad) of mean(w |y - x|) in fp64, w broadcast against the joint distances; grad exactly 0 where the distance is 0"""
    y, x = np.asarray(y, dtype=np.float64), np.asarray(x, dtype=np.float64)
    d = y - x
    e = np.sqrt((d * d).sum(-1, keepdims=True))
    wb = np.broadcast_to(np.asarray(w, dtype=np.float64), e.shape[:-1])[..., None]
    J = float(e.size)
    with np.errstate(invalid="ignore", divide="ignore"):
        grad = np.where(e == 0, 0.0, wb * d / (e * J))
    return (wb * e).sum() / J, grad


def weighted_sum_survives(y, x, w):
    """whether enough of the weighted sum survives its signs for the 1-ulp32 bound of the loss: |sum w e| / sum |w| e >= n 2^-27
    (module docstring)"""
    e = np.sqrt(((np.asarray(y, dtype=np.float64) - np.asarray(x, dtype=np.float64)) ** 2).sum(-1))
    t = np.broadcast_to(np.asarray(w, dtype=np.float64), e.shape) * e
    return bool(abs(t.sum()) >= e.size * 2.0 ** -27 * np.abs(t).sum())


def byjoint(y, x, cot):
    """(value, grad): mean over the first axis of |y - x| (shape y.shape[1:-1]) and the backward of it for the cotangent cot, in
    fp64; grad exactly 0 where the distance is 0"""
    y, x = np.asarray(y, dtype=np.float64), np.asarray(x, dtype=np.float64)
    d = y - x
    e = np.sqrt((d * d).sum(-1, keepdims=True))
    c = np.broadcast_to(np.asarray(cot, dtype=np.float64).reshape(y.shape[1:-1]), e.shape[:-1])[..., None]
    with np.errstate(invalid="ignore", divide="ignore"):
        grad = np.where(e == 0, 0.0, c * d / (e * float(y.shape[0])))
    return e[..., 0].mean(0), grad


def torch_n_mpjpe(predicted, target):
    """the reference's n_mpjpe expression in stock torch"""
    import torch
    norm_predicted = torch.mean(torch.sum(predicted ** 2, dim=3, keepdim=True), dim=2, keepdim=True)
    norm_target = torch.mean(torch.sum(target * predicted, dim=3, keepdim=True), dim=2, keepdim=True)
    return torch.mean(torch.norm(norm_target / norm_predicted * predicted - target, dim=len(target.shape) - 1))


def torch_weighted_mpjpe(predicted, target, w):
    """the reference's weighted_mpjpe expression in stock torch"""
    import torch
    return torch.mean(w * torch.norm(predicted - target, dim=len(target.shape) - 1))


def torch_mpjpe_byjoint(predicted, target):
    """the reference's mpjpe_byjoint expression in stock torch"""
    import torch
    return torch.mean(torch.norm(predicted - target, dim=len(target.shape) - 1), dim=0)
