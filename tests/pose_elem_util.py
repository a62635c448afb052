"""Seeded inputs, fp64 / fp32 restatements and the tolerance rule of tests/test_gpu_pose_elem.py.  Everything here runs on the host
with torch and the oracle only (no code of the package), so the references and the input statistics can be checked without a GPU."""
import math

import torch

import golden_util as GU
from oracle import dhaug_oracle as O

U32 = 2.0 ** -24                     # unit roundoff of fp32 (round to nearest)

# ---- launch shapes of csrc/dhaug_pose.hip / csrc/dhaug_elem.hip that the multi-pass sizes are derived from.  A changed constant in
# the source is a size to revisit here.
GRID_CAP = 256 * 16                  # grid1d(): at most 4 096 workgroups per launch
JOINT_BLOCK = 256                    # camera kernels: one lane per joint, 256 per workgroup, 16 joints per pose
TILE = 64                            # kcs_* / bone_swap / d3_penalty: 64 poses per workgroup
FLIP_BLOCK = 256                     # center_flip: one lane per pose, 256 per workgroup
GP_ROWS_PER_BLOCK = 4                # gp_penalty: one wave per row, four waves per workgroup
WM_THREADS, WM_UNROLL = 1024, 4      # weighted_means: ONE workgroup of 1 024 lanes, four accumulators per lane
CS_BLOCKS, CS_THREADS = 64, 256      # critic_scalars stage 1: 64 workgroups of 256 lanes

POSES_PER_PASS_JOINT = GRID_CAP * JOINT_BLOCK // 16         # 65 536 (the headline batch is exactly one pass)
POSES_PER_PASS_TILE = GRID_CAP * TILE                       # 262 144
POSES_PER_PASS_FLIP = GRID_CAP * FLIP_BLOCK                 # 1 048 576
ROWS_PER_PASS_GP = GRID_CAP * GP_ROWS_PER_BLOCK             # 16 384
ELEMS_PER_PASS = GRID_CAP * 256                             # 1 048 576: every one-lane-per-element kernel (frame_*, gp_assemble)
ELEMS_PER_TRIP_WM = WM_THREADS * WM_UNROLL                  # 4 096
LOGITS_PER_PASS_CS = CS_BLOCKS * CS_THREADS                 # 16 384

RAGGED = [1, 63, 64, 65, 1000]
N_JOINT = RAGGED + [POSES_PER_PASS_JOINT + 17]              # second pass: 17 poses = 272 joints, two workgroups, one ragged
N_TILE = RAGGED + [POSES_PER_PASS_TILE + 65]                # second pass: two tiles, the last with one row
N_FLIP = RAGGED + [POSES_PER_PASS_FLIP + 3]                 # second pass: three lanes of one workgroup
B_GP = RAGGED + [ROWS_PER_PASS_GP * 4 + 1]                  # five passes, the fifth with one wave
N_REDUCE = 3 * 65536 + 5                                    # weighted_means: 49 trips of the unrolled loop; critic_scalars: 13 passes

FLIP_PERM = list(range(16))
for _l, _r in zip(O.FLIP_LEFT, O.FLIP_RIGHT):
    FLIP_PERM[_l], FLIP_PERM[_r] = _r, _l


def gen(seed):
    return torch.Generator().manual_seed(seed)


def maxabs(a, b):
    return (a.detach().double().cpu() - b.detach().double().cpu()).abs().max().item()


def rule(name, got, ref64, ref32, t_project, keep=None, slack=None):
    """The tolerance rule of the size sweeps: max|gpu - ref64| <= max(T_project, 4 max|ref32 - ref64|), the second term measured on
    the reference alone (the same operation rounded to fp32 in another order is as far from fp64 as the fp32 reference is; the factor
    4 covers FMA contraction and 1/z once instead of two divisions).  Prints the figures, returns (err, bound).
    keep: boolean mask (broadcastable) of the elements compared.  slack: per-element allowance taken off |gpu - ref64| first (the
    half ulp of a bf16 output).  The comparison runs where `got` lives."""
    dv = got.device
    ref64 = ref64.detach().to(dv).double().reshape(got.shape)
    d_g = (got.detach().double() - ref64).abs()
    d_r = (ref32.detach().to(dv).double().reshape(got.shape) - ref64).abs()
    if slack is not None:
        d_g = (d_g - slack.to(dv)).clamp_min(0.0)
    if keep is not None:
        keep = keep.to(dv).expand_as(d_g)
        d_g, d_r = d_g[keep], d_r[keep]
    err, e32 = d_g.max().item(), d_r.max().item()
    bound = max(t_project, 4.0 * e32)
    print("%-58s err %.3e  bound %.3e  (T_project %.3e, 4 x |ref32 - ref64| %.3e)" % (name, err, bound, t_project, 4.0 * e32))
    assert math.isfinite(err) and err <= bound, (name, err, bound)
    return err, bound


# ------------------------------------------------------------------------------------------------------------------ camera
def camera_case(N, seed):
    """camera-space points x, y ~ N(0, 2), z ~ U(0.5, 6) (about a fifth of the ratios x/z, y/z beyond +-1), taken to world space with
    the fp64 oracle and rounded to fp32; one camera (q, t, cam9) for world_to_camera_project, per-sample ones for camera_to_world /
    project_to_2d.  Intrinsics with non-zero radial and tangential terms, different in every row."""
    g = gen(seed)
    xc = torch.cat([torch.randn(N, 16, 2, generator=g, dtype=torch.float64) * 2.0,
                    torch.rand(N, 16, 1, generator=g, dtype=torch.float64) * 5.5 + 0.5], dim=-1)
    q = torch.randn(1, 4, generator=g, dtype=torch.float64)
    q = (q / q.norm()).float()
    t = (torch.randn(1, 3, generator=g, dtype=torch.float64) * 2.0).float()
    X = O.camera_to_world(xc, q.double().expand(N, 4), t.double().expand(N, 3)).float()

    def cams(n):
        f = 2.0 + 0.5 * torch.rand(n, 2, generator=g)
        c = 0.1 * torch.randn(n, 2, generator=g)
        k = torch.randn(n, 3, generator=g) * torch.tensor([0.2, 0.05, 0.01])
        p = 0.01 * torch.randn(n, 2, generator=g)
        return torch.cat([f, c, k, p], dim=1)
    cam = cams(1)
    qn = torch.randn(N, 4, generator=g)
    qn = qn / qn.norm(dim=1, keepdim=True)
    tn = torch.randn(N, 3, generator=g) * 2.0
    g3 = torch.randn(N, 16, 3, generator=g)
    g2 = torch.randn(N, 16, 2, generator=g)
    return dict(X=X, q=q, t=t, cam=cam, xc=xc.float(), qn=qn, tn=tn, camn=cams(N), g3=g3, g2=g2)


def w2c_project_ref(c, dtype, g3=None, g2=None):
    """(cam3d, proj2d, grad_pose or None) of the oracle at dtype; the gradient by autograd with the cotangents given"""
    X = c["X"].detach().to(dtype, copy=True).requires_grad_(g3 is not None or g2 is not None)
    Xc = O.world_to_camera(X, c["q"].to(dtype), c["t"].to(dtype))
    p2 = O.project_to_2d(Xc, c["cam"].to(dtype))
    grad = None
    if X.requires_grad:
        s = 0.0
        if g3 is not None:
            s = s + (Xc * g3.to(dtype)).sum()
        if g2 is not None:
            s = s + (p2 * g2.to(dtype)).sum()
        grad, = torch.autograd.grad(s, X)
    return Xc.detach(), p2.detach(), grad


def clamp_stats(Xc64, margin=1e-4):
    """of the fp64 camera-space points: the ratios (N,16,2), which are clamped, and the joints (N,16,1) with a ratio within margin of +-1"""
    r = Xc64[..., :2] / Xc64[..., 2:]
    clamped = r.abs() > 1.0
    near = ((r.abs() - 1.0).abs() <= margin).any(dim=-1, keepdim=True)
    return r, clamped, near


# ------------------------------------------------------------------------------------------------------------- bone kernels
def fk_poses(N, seed):
    """(N,16,3) fp32 poses of the oracle's FK on golden_util.synth_fk_inputs: every bone at least 0.1 m"""
    a, bl, rt = GU.synth_fk_inputs(N, seed)
    return O.fk_forward16(a, bl, rt).reshape(N, 16, 3).contiguous()


def kcs_vjp_ref(x, gf, wl, dtype):
    xd = x.detach().to(dtype, copy=True).requires_grad_(True)
    f = O.kcs_features(xd, with_lengths=wl)
    grad, = torch.autograd.grad((f * gf.to(dtype)).sum(), xd)
    return f.detach(), grad


def kcs_jvp_ref(x, tan, wl, dtype):
    return torch.func.jvp(lambda p: O.kcs_features(p, with_lengths=wl), (x.to(dtype),), (tan.to(dtype),))[1]


def d3_penalty_ref(x, gk, gp, coef, dtype):
    """tangent of the KCS branch (N,30), of the pose branch (N,48), penalty (N): dhaug_d3_penalty restated on the oracle"""
    N = x.shape[0]
    _, gx = kcs_vjp_ref(x, gk, True, dtype)
    g = gx.reshape(N, 48) + gp.to(dtype)
    n = g.norm(dim=1, keepdim=True)
    k = torch.where(n > 0, coef * (n - 1) / n.clamp_min(1e-300 if dtype == torch.float64 else 1e-30), torch.zeros_like(n))
    v = k * g
    tk = kcs_jvp_ref(x, v.reshape(N, 16, 3), True, dtype)
    return tk, v, ((n - 1) ** 2)[:, 0]


def gp_penalty_ref(g, coef, dtype):
    g = g.to(dtype)
    n = g.norm(dim=1, keepdim=True)
    k = torch.where(n > 0, coef * (n - 1) / n.clamp_min(1e-300 if dtype == torch.float64 else 1e-30), torch.zeros_like(n))
    return k * g, ((n - 1) ** 2)[:, 0]


# ------------------------------------------------------------------------------------------------------- centre / flip
def center_flip_fwd(x, center, flip):
    """differentiable restatement of dhaug_center_flip at x's dtype ((N,16,C)): x - x[:, :1], then the oracle's flip_lr"""
    y = x - x[:, :1] if center else x * 1.0
    if flip:
        sign = torch.ones(x.shape[-1], dtype=x.dtype, device=x.device)
        sign[0] = -1.0
        y = (y * sign)[:, FLIP_PERM]
    return y


def center_flip_adj(g, center, flip):
    """the transpose of center_flip_fwd by autograd (the map is linear: the point of linearisation does not matter)"""
    x = torch.zeros_like(g).requires_grad_(True)
    out, = torch.autograd.grad((center_flip_fwd(x, center, flip) * g).sum(), x)
    return out


# ------------------------------------------------------------------------------------------------------------ frame ops
def frame_diff_ref(x, R, in_w, w):
    """the oracle's _frame_diff on the first w columns of every frame"""
    rows = x.shape[0]
    return O._frame_diff(x.reshape(rows, R, in_w)[:, :, :w].reshape(rows, R * w), R, w)


def frame_diff_adj_ref(g, R, in_w, w):
    x = torch.zeros(g.shape[0], R * in_w, dtype=g.dtype, device=g.device, requires_grad=True)
    out, = torch.autograd.grad((frame_diff_ref(x, R, in_w, w) * g).sum(), x)
    return out


# ----------------------------------------------------------------------------------------------------------- reductions
def wm_depth(n):
    """fp32 additions on the longest path of weighted_means_kernel for an array of n elements, counted from the source for lane 0
    (it owns the most elements): `trips` serial adds into s0 by the four-way unrolled loop (one trip while j + 3 * 1024 < n,
    j += 4 * 1024), `tail` more by the remainder loop (j += 1024), 2 for (s0 + s1) + (s2 + s3), 6 for the wave butterfly, 16 for
    the serial sum over the 16 waves' partials, 1 for the division by n:  27 at n = 4 097, 74 at n = 196 613."""
    trips = 0 if n <= 3 * WM_THREADS else (n - 3 * WM_THREADS - 1) // ELEMS_PER_TRIP_WM + 1
    left = n - trips * ELEMS_PER_TRIP_WM
    tail = (left + WM_THREADS - 1) // WM_THREADS if left > 0 else 0
    return trips + tail + 2 + 6 + 16 + 1


def cs_depth(n, scaled=False):
    """the same count for one mean of dhaug_critic_scalars over n values: ceil(n / 16 384) serial adds per lane of stage 1, 6 (wave
    butterfly) + 2 ((r0 + r1) + (r2 + r3)); stage 2: 6 (butterfly over the 64 partials) + 1 (division); scaled: + 1 (lambda *)"""
    return (n + LOGITS_PER_PASS_CS - 1) // LOGITS_PER_PASS_CS + 6 + 2 + 6 + 1 + (1 if scaled else 0)


def gamma(k):
    """Higham's gamma_k = k u / (1 - k u): the relative error bound of a sum of depth k, relative to sum |x|"""
    return k * U32 / (1.0 - k * U32)
