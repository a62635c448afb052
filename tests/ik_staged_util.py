"""Reference side of the staged, joint-weighted inverse-kinematics tests.  TEST INFRASTRUCTURE ONLY.

The fp64 restatement of fit_pose_staged (csrc/dhaug_ik_math.h): ik_util.lm_fit with a weight w_j >= 0 per joint on the residual,

    cost = sum_j w_j^2 |r_j|^2,   H = Jw^T Jw,  g = Jw^T rw   with the rows of joint j of J and r times w_j,

run stage after stage: every stage starts from the angles the one before left, lambda back at lambda0, the cost taken anew under
its own weights.  The residual is the largest joint distance over the joints of weight > 0 in the last stage.  Joint 0 is the root:
its residual is 0 by construction and its weight is not used.

COARSE_TO_FINE restates ops.IK_COARSE_TO_FINE (tests/test_ik_staged_cpu.py compares the two)."""
import os

import numpy as np
import torch

import ik_util as K

F64 = K.F64
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ik_staged.npz")
GOLDEN_POSES = 256
ALL = list(range(16))


def row(joints):
    return [1.0 if j in joints else 0.0 for j in range(16)]


COARSE_TO_FINE = [(row([1, 4, 7]), 8), (row([1, 4, 7, 8, 10, 13]), 8), (row([1, 4, 7, 8, 10, 13, 9, 2, 5, 11, 14]), 8), (row(ALL), 16)]


def weights64(w):
    w = torch.as_tensor(w, dtype=F64).reshape(16).clone()
    w[0] = 0.0
    return w


def weighted_cost64(angles, bone_len, root, pose, w):
    """sum_j w_j^2 |FK(angles)_j - pose_j|^2 per pose, fp64"""
    r = K.fk64(angles, bone_len, root) - pose.double().reshape(-1, 16, 3)
    return ((r ** 2).sum(dim=2) * weights64(w) ** 2).sum(dim=1)


def joint_error_over(angles, bone_len, root, pose, w):
    """largest joint distance over the joints of weight > 0, metres, fp64"""
    d = (K.fk64(angles, bone_len, root) - pose.double().reshape(-1, 16, 3)).norm(dim=2)
    return d[:, weights64(w) > 0].max(dim=1).values


def cost_allowance(cost):
    """what two fp64 costs of fp32 solutions may differ by through the fp32 FK's own error (1e-5 m per joint coordinate): the allowance
    of tests/test_gpu_ik_kernels.py::exact_properties"""
    return 2 * cost.sqrt() * (45 ** 0.5) * 1e-5 + 1e-10


def lm_stage(pose, ang, bl, root, w, iters, lo, hi, lambda0):
    """`iters` weighted steps from ang (N,37) fp64, already inside the limits; returns the new angles"""
    N = pose.shape[0]
    w = weights64(w)
    w3 = w.repeat_interleave(3)                                   # per row of J / r
    lam = torch.full((N,), float(min(max(lambda0, K.LAM_MIN), K.LAM_MAX)), dtype=F64)
    r = K.fk64(ang, bl, root) - pose
    cost = ((r ** 2).sum(dim=2) * w ** 2).sum(dim=1)
    eye = torch.eye(len(K.LIVE), dtype=F64)
    for _ in range(iters):
        J = K.jacobian64(ang, bl)[:, :, K.LIVE] * w3[None, :, None]
        H = J.transpose(1, 2) @ J
        g = J.transpose(1, 2) @ (r.reshape(N, 48) * w3).reshape(N, 48, 1)
        A = H + lam[:, None, None] * torch.diag_embed(H.diagonal(dim1=1, dim2=2)) + K.EPS_DIAG * eye
        delta = torch.cholesky_solve(g, torch.linalg.cholesky(A)).reshape(N, -1)
        trial = ang.clone()
        trial[:, K.LIVE] = torch.minimum(torch.maximum(ang[:, K.LIVE] - delta, lo[K.LIVE]), hi[K.LIVE])
        r2 = K.fk64(trial, bl, root) - pose
        cost2 = ((r2 ** 2).sum(dim=2) * w ** 2).sum(dim=1)
        acc = cost2 < cost
        ang = torch.where(acc[:, None], trial, ang)
        r = torch.where(acc[:, None, None], r2, r)
        cost = torch.where(acc, cost2, cost)
        lam = (lam * torch.where(acc, K.LAM_DOWN, K.LAM_UP)).clamp(K.LAM_MIN, K.LAM_MAX)
    return ang


def lm_fit_staged(pose, stages, init=None, lo=None, hi=None, bone_len=None, lambda0=K.LAMBDA0):
    """the restatement, fp64, batched.  stages: (weights16, iters) pairs.  Returns (angles (N,37), bone_len, root, residual), fp64"""
    pose = pose.double().reshape(-1, 16, 3)
    N = pose.shape[0]
    lo = K.LO if lo is None else torch.as_tensor(lo, dtype=F64)
    hi = K.HI if hi is None else torch.as_tensor(hi, dtype=F64)
    root = pose[:, 0].clone()
    bl = K.bone_lengths64(pose) if bone_len is None else bone_len.double().reshape(N, 15).clone()
    ang = torch.zeros(N, 37, dtype=F64) if init is None else init.double().clone()
    ang = torch.minimum(torch.maximum(ang, lo), hi)
    ang[:, K.DEAD] = 0.0
    for w, iters in stages:
        ang = lm_stage(pose, ang, bl, root, w, iters, lo, hi, lambda0)
    return ang, bl, root, joint_error_over(ang, bl, root, pose, stages[-1][0])


def golden_inputs(N=GOLDEN_POSES):
    """the poses of the recording: the first N of ik_util.trial_fit_inputs (seed 20261021)"""
    return K.trial_fit_inputs(GOLDEN_POSES)["pose"][:N]


def cold_errors(N):
    """fp64 joint error per pose of the restatement from the T-pose with the default schedule, on the first N recorded poses"""
    pose = golden_inputs(N)
    ang, bl, root, _ = lm_fit_staged(pose, COARSE_TO_FINE)
    return K.joint_error(ang, bl, root, pose)


def load_golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}
