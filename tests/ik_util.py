"""Reference side of the inverse-kinematics tests.  TEST INFRASTRUCTURE ONLY.

The original project has no IK, so the reference is (a) its FK -- oracle/dhaug_oracle.py: fk_forward16 in fp64 -- and (b) this
fp64 torch restatement of the algorithm of csrc/dhaug_ik_math.h, with the Jacobian taken by autograd through the oracle's FK:

    root = joint 0, bone_len = the 15 joint distances, then `iters` times
        H = J^T J, g = J^T r, (H + lambda diag(H) + EPS_DIAG I) delta = g by Cholesky, theta' = clamp(theta - delta, lo, hi),
        accepted when the cost falls (lambda *= 0.3), else theta stays (lambda *= 5); lambda in [1e-9, 1e6].

A solution is judged by the pose it reproduces, never by its angles (several slots are redundant for the joint positions): a pose
CONVERGED when the fp64 oracle FK of the returned angles, lengths and root lies within CONVERGED_M of the target at every joint.

The trial inputs: angles uniform in the middle 30 % of each generator range, default bone lengths +- 20 %, root (0.1, -0.2, 4.5);
a fit starts 5 degrees off per live slot; a tracked sequence moves at most 3 degrees per slot and frame."""
import math

import torch

from oracle import dhaug_oracle as O

F64 = torch.float64
LIVE = list(O.LIVE_SLOTS)                     # the generator's 31 slots
DEAD = list(O.ZERO_SLOTS)                     # pinned to 0: 4, 9, 22, 23, 28, 33
STILL = [27, 32]                              # live slots that turn a leaf frame: no joint moves
CONVERGED_M = 1e-4
EPS_DIAG = 1e-8
LAMBDA0 = 1e-3
LAM_MIN, LAM_MAX, LAM_DOWN, LAM_UP = 1e-9, 1e6, 0.3, 5.0
DEFAULT_LEN = [0.5, 0.5, 0.6, 0.6, 0.25, 0.25, 0.25, 0.2, 0.4, 0.4, 0.4, 0.4, 0.35, 0.35, 0.15]
ROOT = (0.1, -0.2, 4.5)
LO = torch.tensor(O.ANGLE_LO, dtype=F64)
HI = torch.tensor(O.ANGLE_HI, dtype=F64)
JAC_TOL = 1e-5 * math.pi / 180                # the FK's 1e-5 m carried through the derivative's scale (m per degree)


def fk64(angles, bone_len, root):
    """(N,37), (N,15), (N,3) of any float type -> (N,16,3) fp64"""
    return O.fk_forward16(angles.double(), bone_len.double(), root.double())


def jacobian64(angles, bone_len):
    """(N,48,37) fp64: d joint coordinate / d angle slot (m per degree) by autograd through the oracle's FK -- one forward and one
    backward pass over 48 copies of the batch, copy k selecting output coordinate k"""
    N = angles.shape[0]
    a = angles.detach().double().repeat_interleave(48, 0).requires_grad_(True)
    b = bone_len.detach().double().repeat_interleave(48, 0)
    out = O.fk_forward16(a, b, torch.zeros(48 * N, 3, dtype=F64)).reshape(N, 48, 48)
    out.diagonal(dim1=1, dim2=2).sum().backward()
    return a.grad.reshape(N, 48, 37)


def bone_lengths64(pose):
    p = pose.double().reshape(-1, 16, 3)
    return torch.stack([(p[:, c] - p[:, q]).norm(dim=1) for q, c in O.BONE_PAIRS], dim=1)


def joint_error(angles, bone_len, root, pose):
    """largest joint distance per pose, metres, fp64: what decides `converged`"""
    return (fk64(angles, bone_len, root) - pose.double().reshape(-1, 16, 3)).norm(dim=2).max(dim=1).values


def cost64(angles, bone_len, root, pose):
    return ((fk64(angles, bone_len, root) - pose.double().reshape(-1, 16, 3)) ** 2).sum(dim=(1, 2))


def lm_fit(pose, init=None, lo=None, hi=None, iters=12, lambda0=LAMBDA0):
    """the restatement, fp64, batched.  Returns (angles (N,37), bone_len, root, residual), all fp64"""
    pose = pose.double().reshape(-1, 16, 3)
    N = pose.shape[0]
    lo = LO if lo is None else torch.as_tensor(lo, dtype=F64)
    hi = HI if hi is None else torch.as_tensor(hi, dtype=F64)
    root = pose[:, 0].clone()
    bl = bone_lengths64(pose)
    ang = torch.zeros(N, 37, dtype=F64) if init is None else init.double().clone()
    ang = torch.minimum(torch.maximum(ang, lo), hi)
    ang[:, DEAD] = 0.0
    lam = torch.full((N,), float(min(max(lambda0, LAM_MIN), LAM_MAX)), dtype=F64)
    r = fk64(ang, bl, root) - pose
    cost = (r ** 2).sum(dim=(1, 2))
    eye = torch.eye(len(LIVE), dtype=F64)
    for _ in range(iters):
        J = jacobian64(ang, bl)[:, :, LIVE]
        H = J.transpose(1, 2) @ J
        g = (J.transpose(1, 2) @ r.reshape(N, 48, 1))
        A = H + lam[:, None, None] * torch.diag_embed(H.diagonal(dim1=1, dim2=2)) + EPS_DIAG * eye
        delta = torch.cholesky_solve(g, torch.linalg.cholesky(A)).reshape(N, -1)
        trial = ang.clone()
        trial[:, LIVE] = torch.minimum(torch.maximum(ang[:, LIVE] - delta, lo[LIVE]), hi[LIVE])
        r2 = fk64(trial, bl, root) - pose
        cost2 = (r2 ** 2).sum(dim=(1, 2))
        acc = cost2 < cost
        ang = torch.where(acc[:, None], trial, ang)
        r = torch.where(acc[:, None, None], r2, r)
        cost = torch.where(acc, cost2, cost)
        lam = (lam * torch.where(acc, LAM_DOWN, LAM_UP)).clamp(LAM_MIN, LAM_MAX)
    return ang, bl, root, r.norm(dim=2).max(dim=1).values


def lm_track(pose, offsets, init=None, lo=None, hi=None, iters=8, lambda0=LAMBDA0):
    """the restatement over concatenated sequences: frame t of every sequence that has one is one batched lm_fit"""
    pose = pose.double().reshape(-1, 16, 3)
    T, S = pose.shape[0], len(offsets) - 1
    ang = torch.zeros(T, 37, dtype=F64)
    bl, root, res = torch.zeros(T, 15, dtype=F64), torch.zeros(T, 3, dtype=F64), torch.zeros(T, dtype=F64)
    prev = torch.zeros(S, 37, dtype=F64) if init is None else init.double().clone()
    for t in range(max(offsets[s + 1] - offsets[s] for s in range(S))):
        seqs = [s for s in range(S) if offsets[s] + t < offsets[s + 1]]
        rows = [offsets[s] + t for s in seqs]
        a, b, r0, e = lm_fit(pose[rows], prev[seqs], lo, hi, iters, lambda0)
        ang[rows], bl[rows], root[rows], res[rows] = a, b, r0, e
        prev[seqs] = a
    return ang, bl, root, res


# ---------------------------------------------------------------------------------------------------------- the trial's inputs
def trial_angles(N, g, spread=0.3):
    mid, half = (LO + HI) / 2, (HI - LO) / 2
    a = mid + spread * half * (torch.rand(N, 37, generator=g, dtype=F64) * 2 - 1)
    a[:, DEAD] = 0.0
    return a.float()


def trial_lengths(N, g):
    return (torch.tensor(DEFAULT_LEN, dtype=F64) * (0.8 + 0.4 * torch.rand(N, 15, generator=g, dtype=F64))).float()


def perturbed(angles, g, degrees):
    """angles +- `degrees` per live slot, inside the generator's limits, dead slots 0; fp32"""
    a = angles.double() + degrees * (torch.rand(angles.shape, generator=g, dtype=F64) * 2 - 1)
    a = torch.minimum(torch.maximum(a, LO), HI)
    a[:, DEAD] = 0.0
    return a.float()


def trial_fit_inputs(N, seed=20261021):
    """dict of fp32 tensors: truth (N,37), bone_len (N,15), root (N,3), pose (N,16,3) = fp64 oracle FK rounded, init (N,37)"""
    g = torch.Generator().manual_seed(seed)
    truth, bl = trial_angles(N, g), trial_lengths(N, g)
    root = torch.tensor(ROOT, dtype=torch.float32).repeat(N, 1)
    return {"truth": truth, "bone_len": bl, "root": root, "pose": fk64(truth, bl, root).float(), "init": perturbed(truth, g, 5.0)}


def ragged_lengths(S, frames=24):
    """S sequence lengths of at most `frames`, a length of 1 among them where S > 1"""
    n = [frames, 1, 17, 24, 9, 2, 13]
    return [n[s % len(n)] for s in range(S)]


def trial_track_inputs(S, lengths=None, seed=20261022, step=3.0):
    """concatenated sequences: frame 0 from the trial's angles, each later frame at most `step` degrees per live slot from the one
    before; lengths and root fixed per sequence.  dict: pose (T,16,3), offsets (S+1 ints), init (S,37), truth (T,37)"""
    g = torch.Generator().manual_seed(seed)
    lengths = [24] * S if lengths is None else list(lengths)
    a0, bl0 = trial_angles(S, g), trial_lengths(S, g)
    init = perturbed(a0, g, step)
    offsets, truth, bls = [0], [], []
    for s in range(S):
        a = a0[s:s + 1]
        for t in range(lengths[s]):
            if t:
                a = perturbed(a, g, step)
            truth.append(a)
            bls.append(bl0[s:s + 1])
        offsets.append(offsets[-1] + lengths[s])
    truth, bls = torch.cat(truth), torch.cat(bls)
    root = torch.tensor(ROOT, dtype=torch.float32).repeat(truth.shape[0], 1)
    return {"pose": fk64(truth, bls, root).float(), "offsets": offsets, "init": init, "truth": truth, "bone_len": bls}


def off_manifold(pose, g, sigma=0.005):
    """targets the model cannot reach exactly: FK poses plus Gaussian noise of `sigma` metres per coordinate"""
    return (pose.double() + sigma * torch.randn(pose.shape, generator=g, dtype=F64)).float()


def not_converged(err):
    return int((err > CONVERGED_M).sum())
