"""Tensor-level wrappers of the C-ABI (no autograd here): allocate outputs with torch, pass raw device pointers and
the current HIP stream to libdhaug.so.  Every function requires CUDA(HIP) tensors and raises otherwise."""
import collections
import ctypes
import os

import torch

from . import _lib

_vp = ctypes.c_void_p
BF16 = torch.bfloat16


def _stream():
    """raw handle of torch's current stream (an int: argtypes c_void_p converts it; no ctypes object per call)"""
    return torch.cuda.current_stream().cuda_stream or None


def _p(t):
    """raw device pointer (int) or None"""
    return None if t is None else t.data_ptr()


def _dev(t, dtype, name):
    if not t.is_cuda:
        raise RuntimeError("dhaug op `%s` needs a GPU tensor (no CPU fallback exists)" % name)
    if t.dtype != dtype:
        t = t.to(dtype)
    if not t.is_contiguous():
        t = t.contiguous()
    if t.data_ptr() % 16:
        t = t.clone()
    return t


def _host3(x, n):
    """small host-side float arrays (camera parameters) -> ctypes float[n]"""
    if torch.is_tensor(x):
        x = x.detach().reshape(-1).cpu().tolist()
    x = [float(v) for v in (x.reshape(-1).tolist() if hasattr(x, "reshape") else x)]
    assert len(x) == n, (len(x), n)
    return (ctypes.c_float * n)(*x)


def ceil_to(v, m):
    return (v + m - 1) // m * m


# ---------------------------------------------------------------------------------------------- FK
def fk_forward(angles, bone_len, root, out_joints=16):
    a = _dev(angles, torch.float32, "fk_forward").reshape(-1, 37)
    b = _dev(bone_len, torch.float32, "fk_forward").reshape(-1, 15)
    r = None if root is None else _dev(root, torch.float32, "fk_forward").reshape(-1, 3)
    N = a.shape[0]
    assert b.shape[0] == N and (r is None or r.shape[0] == N), "FK inputs disagree on the number of poses"
    out = torch.empty((N, out_joints, 3), dtype=torch.float32, device=a.device)
    _lib.call("dhaug_fk_forward", _p(a), _p(b), _p(r), _p(out), N, out_joints, _stream())
    return out


def fk_backward(angles, bone_len, grad_out16):
    a = _dev(angles, torch.float32, "fk_backward").reshape(-1, 37)
    b = _dev(bone_len, torch.float32, "fk_backward").reshape(-1, 15)
    g = _dev(grad_out16, torch.float32, "fk_backward").reshape(-1, 48)
    N = a.shape[0]
    ga = torch.empty((N, 37), dtype=torch.float32, device=a.device)
    gb = torch.empty((N, 15), dtype=torch.float32, device=a.device)
    gr = torch.empty((N, 3), dtype=torch.float32, device=a.device)
    _lib.call("dhaug_fk_backward", _p(a), _p(b), _p(g), _p(ga), _p(gb), _p(gr), N, _stream())
    return ga, gb, gr


# ---------------------------------------------------------------------------------------------- IK
IK_DEAD_SLOTS = (4, 9, 22, 23, 28, 33)          # pinned to 0 by the generator (Fk_generator.py:136)
# the generator's joint limits per slot, degrees (kAngLo / kAngHi of csrc/dhaug_fk_math.h)
IK_GENERATOR_LO = [-110, -110, -110, -180, 0, -65, -65, -110, -180, 0] + [-180] * 12 + [0, 0] + \
                  [-155, -155, -100, 0, 0, -65, -65, -100, 0, 0] + [-180, -180, -180]
IK_GENERATOR_HI = [65, 65, 180, 0, 0, 110, 110, 180, 0, 0] + [180] * 12 + [0, 0] + \
                  [65, 65, 180, 180, 0, 155, 155, 180, 180, 0] + [180, 180, 180]
IkFit = collections.namedtuple("IkFit", "angles37 bone_len root residual")


def fk_jacobian(angles, bone_len):
    """(N,37) deg, (N,15) m -> (N,48,37): d joint coordinate / d angle slot, metres per degree (dhaug_fk_jacobian)."""
    a = _dev(angles, torch.float32, "fk_jacobian").reshape(-1, 37)
    b = _dev(bone_len, torch.float32, "fk_jacobian").reshape(-1, 15)
    N = a.shape[0]
    if b.shape[0] != N:
        raise ValueError("fk_jacobian: %d rows of angles, %d of bone lengths" % (N, b.shape[0]))
    J = torch.empty((N, 48, 37), dtype=torch.float32, device=a.device)
    _lib.call("dhaug_fk_jacobian", _p(a), _p(b), _p(J), N, _stream())
    return J


def _ik_shape(pose16, name):
    if not torch.is_tensor(pose16) or pose16.dim() < 2 or tuple(pose16.shape[-2:]) != (16, 3):
        raise ValueError("%s: poses must be a tensor that views as (..., 16, 3), got %s"
                         % (name, tuple(pose16.shape) if torch.is_tensor(pose16) else type(pose16).__name__))


def _ik_steps(iters, lambda0, name):
    if int(iters) < 1:
        raise ValueError("%s: iters must be at least 1, got %r" % (name, iters))
    if not float(lambda0) > 0.0:
        raise ValueError("%s: lambda0 must be positive, got %r" % (name, lambda0))


def _ik_limits(lo, hi, name):
    """the limits as two host lists of 37 (lo <= hi checked), and whether they are the caller's"""
    if lo is None and hi is None:
        return IK_GENERATOR_LO, IK_GENERATOR_HI, False
    if lo is None or hi is None:
        raise ValueError("%s: lo and hi come together" % name)
    hl = [float(v) for v in (lo.detach().reshape(-1).cpu().tolist() if torch.is_tensor(lo) else list(lo))]
    hh = [float(v) for v in (hi.detach().reshape(-1).cpu().tolist() if torch.is_tensor(hi) else list(hi))]
    if len(hl) != 37 or len(hh) != 37:
        raise ValueError("%s: limits have 37 entries each, got %d and %d" % (name, len(hl), len(hh)))
    bad = [i for i in range(37) if not hl[i] <= hh[i]]
    if bad:
        raise ValueError("%s: lo > hi at slot(s) %s" % (name, bad))
    return hl, hh, True


def _ik_init(init, rows, hl, hh, clamp_init, dev, name):
    if init is None:
        return None
    i = _dev(init, torch.float32, name).reshape(-1, 37)
    if i.shape[0] != rows:
        raise ValueError("%s: init has %d rows, expected %d" % (name, i.shape[0], rows))
    if not clamp_init:
        lo_t = torch.tensor(hl, dtype=torch.float32, device=dev)
        hi_t = torch.tensor(hh, dtype=torch.float32, device=dev)
        if bool(((i < lo_t) | (i > hi_t)).any()):
            raise ValueError("%s: init lies outside the limits (pass clamp_init=True to clamp it)" % name)
    return i


def _ik_outputs(T, dev):
    return (torch.empty((T, 37), dtype=torch.float32, device=dev), torch.empty((T, 15), dtype=torch.float32, device=dev),
            torch.empty((T, 3), dtype=torch.float32, device=dev), torch.empty((T,), dtype=torch.float32, device=dev))


def ik_fit(pose16, init=None, lo=None, hi=None, iters=20, lambda0=1e-3, clamp_init=False):
    """Poses (...,16,3) -> IkFit(angles37 (N,37) deg, bone_len (N,15), root (N,3), residual (N) m): `iters` damped
    least-squares steps per pose from `init` (N,37) or the T-pose, inside (lo, hi) or the generator's limits (dhaug_ik_fit).
    ValueError before any launch for a bad shape, lo > hi, iters < 1 or an init outside the limits (unless clamp_init)."""
    _ik_shape(pose16, "ik_fit")
    _ik_steps(iters, lambda0, "ik_fit")
    hl, hh, own = _ik_limits(lo, hi, "ik_fit")
    p = _dev(pose16, torch.float32, "ik_fit").reshape(-1, 48)
    N = p.shape[0]
    lim = torch.tensor([hl, hh], dtype=torch.float32, device=p.device) if own else None
    i = _ik_init(init, N, hl, hh, clamp_init, p.device, "ik_fit")
    ang, bl, root, res = _ik_outputs(N, p.device)
    _lib.call("dhaug_ik_fit", _p(p), _p(i), _p(None if lim is None else lim[0]), _p(None if lim is None else lim[1]), _p(ang),
              _p(bl), _p(root), _p(res), N, int(iters), float(lambda0), _stream())
    return IkFit(ang, bl, root, res)


IK_MAX_STAGES = 8                                # MAX_STAGES of csrc/dhaug_ik_math.h


def _joint_row(joints):
    return [1.0 if j in joints else 0.0 for j in range(16)]


# Coarse to fine, trunk outwards, 40 steps in all: hips and spine | + thorax, shoulders | + neck, knees, elbows | every joint.
# (weights16, iters) per stage; entry 0 of a row (the root, which has no residual) is not used.
IK_COARSE_TO_FINE = (
    (_joint_row({1, 4, 7}), 8),
    (_joint_row({1, 4, 7, 8, 10, 13}), 8),
    (_joint_row({1, 4, 7, 8, 10, 13, 9, 2, 5, 11, 14}), 8),
    (_joint_row(set(range(16))), 16),
)


def _ik_stages(stage_weights, stage_iters, name):
    """the schedule as a flat host list of S * 16 weights and a list of S step counts, checked as dhaug_ik_fit_staged checks it"""
    if torch.is_tensor(stage_weights):
        stage_weights = stage_weights.detach().cpu().tolist()
    if torch.is_tensor(stage_iters):
        stage_iters = stage_iters.detach().cpu().tolist()
    try:
        rows = [[float(v) for v in (r.detach().reshape(-1).cpu().tolist() if torch.is_tensor(r) else list(r))] for r in stage_weights]
        its = [int(v) for v in stage_iters]
    except TypeError:
        raise ValueError("%s: stage_weights is a sequence of rows of 16 weights, stage_iters a sequence of step counts" % name)
    S = len(rows)
    if not 1 <= S <= IK_MAX_STAGES:
        raise ValueError("%s: between 1 and %d stages, got %d" % (name, IK_MAX_STAGES, S))
    if len(its) != S:
        raise ValueError("%s: %d rows of weights, %d step counts" % (name, S, len(its)))
    if any(len(r) != 16 for r in rows):
        raise ValueError("%s: a stage has 16 weights (one per joint), got %s" % (name, [len(r) for r in rows]))
    if any(v < 1 for v in its):
        raise ValueError("%s: every stage runs at least 1 step, got %s" % (name, its))
    f32max = 3.4028234663852886e38
    if any(not (0.0 <= w and w * w <= f32max) for r in rows for w in r):
        raise ValueError("%s: weights are finite and not negative (their squares finite in fp32)" % name)
    if not any(w > 0.0 for w in rows[-1][1:]):
        raise ValueError("%s: the last stage needs a joint of weight above 0 (joints 1..15)" % name)
    return [w for r in rows for w in r], its


def ik_fit_staged(pose16, stage_weights, stage_iters, init=None, lo=None, hi=None, bone_len=None, lambda0=1e-3, clamp_init=False):
    """ik_fit in stages, each under a weight per joint on the residual (dhaug_ik_fit_staged): stage_weights S rows of 16 (w_j >= 0;
    0 leaves the joint out), stage_iters S step counts, S <= 8; a stage starts where the one before stopped, lambda back at
    lambda0.  bone_len (N,15) replaces the closed-form lengths (give it when a joint of weight 0 may be wrong).  `residual` is
    the largest distance over the joints of weight > 0 in the last stage.  ops.IK_COARSE_TO_FINE is the schedule for a start
    from the T-pose: ik_fit_staged(pose, *zip(*IK_COARSE_TO_FINE))."""
    _ik_shape(pose16, "ik_fit_staged")
    _ik_steps(1, lambda0, "ik_fit_staged")
    flat, its = _ik_stages(stage_weights, stage_iters, "ik_fit_staged")
    hl, hh, own = _ik_limits(lo, hi, "ik_fit_staged")
    p = _dev(pose16, torch.float32, "ik_fit_staged").reshape(-1, 48)
    N = p.shape[0]
    b = None
    if bone_len is not None:
        b = _dev(bone_len, torch.float32, "ik_fit_staged").reshape(-1, 15)
        if b.shape[0] != N:
            raise ValueError("ik_fit_staged: bone_len has %d rows, expected %d" % (b.shape[0], N))
    lim = torch.tensor([hl, hh], dtype=torch.float32, device=p.device) if own else None
    i = _ik_init(init, N, hl, hh, clamp_init, p.device, "ik_fit_staged")
    ang, bl, root, res = _ik_outputs(N, p.device)
    S = len(its)
    _lib.call("dhaug_ik_fit_staged", _p(p), _p(i), _p(None if lim is None else lim[0]), _p(None if lim is None else lim[1]), _p(b),
              (ctypes.c_float * (S * 16))(*flat), (ctypes.c_int * S)(*its), S, float(lambda0), _p(ang), _p(bl), _p(root), _p(res), N,
              _stream())
    return IkFit(ang, bl, root, res)


def ik_track(pose16, seq_offset, init=None, lo=None, hi=None, iters=8, lambda0=1e-3, clamp_init=False):
    """Concatenated sequences: pose16 (T,16,3), seq_offset S + 1 ascending frame indices from 0 to T (a host sequence or a
    tensor; checked on the host).  Frame 0 of sequence s starts from init[s] (S,37) or the T-pose, frame t from frame t - 1's
    solution (dhaug_ik_track).  Returns IkFit over the T frames."""
    _ik_shape(pose16, "ik_track")
    _ik_steps(iters, lambda0, "ik_track")
    hl, hh, own = _ik_limits(lo, hi, "ik_track")
    T = pose16.numel() // 48
    off = [int(v) for v in (seq_offset.detach().reshape(-1).cpu().tolist() if torch.is_tensor(seq_offset) else list(seq_offset))]
    if len(off) < 1 or off[0] != 0 or off[-1] != T or any(b <= a for a, b in zip(off, off[1:])):
        raise ValueError("ik_track: seq_offset must increase from 0 to the number of frames (%d), got %s%s"
                         % (T, off[:8], "..." if len(off) > 8 else ""))
    S = len(off) - 1
    p = _dev(pose16, torch.float32, "ik_track").reshape(-1, 48)
    lim = torch.tensor([hl, hh], dtype=torch.float32, device=p.device) if own else None
    i = _ik_init(init, S, hl, hh, clamp_init, p.device, "ik_track")
    off_t = torch.tensor(off, dtype=torch.int64, device=p.device)
    ang, bl, root, res = _ik_outputs(T, p.device)
    _lib.call("dhaug_ik_track", _p(p), _p(off_t), _p(i), _p(None if lim is None else lim[0]), _p(None if lim is None else lim[1]),
              _p(ang), _p(bl), _p(root), _p(res), S, int(iters), float(lambda0), _stream())
    return IkFit(ang, bl, root, res)


def gen_tail_forward(head, bone_len, scaler, use_preangle=True, want_angles=False):
    h = _dev(head, torch.float32, "gen_tail_forward").reshape(-1, 35)
    b = _dev(bone_len, torch.float32, "gen_tail_forward").reshape(-1, 15)
    s = None if scaler is None else _dev(scaler, torch.float32, "gen_tail_forward").reshape(-1, 8)
    N = h.shape[0]
    assert b.shape[0] == N and (s is None or s.shape[0] == N)
    fake = torch.empty((N, 16, 3), dtype=torch.float32, device=h.device)
    ang = torch.empty((N, 37), dtype=torch.float32, device=h.device) if want_angles else None
    _lib.call("dhaug_gen_tail_forward", _p(h), _p(b), _p(s), _p(fake), _p(ang), N, int(bool(use_preangle)), _stream())
    return fake, ang


def gen_tail_forward_critics(head, bone_len, scaler, use_preangle=True, camera=None, rng=None, want_scaler=False,
                             want_critic_inputs=True, inputs_bf16=False):
    """generator tail + what the critics consume in one launch: (fake (N,16,3), centered (N,48), kcs bf16 (N,32),
    proj2d (N,16,2) | None).  camera = (quat[4], trans[3], cam9[9]) host sequences.  rng = (seed, offset): draw the
    bone-length jitter in the kernel (scaler must be None); want_scaler appends the (N,8) draw to the result;
    want_critic_inputs=False skips the centred pose and the KCS operand (plain sampling with the in-kernel jitter);
    inputs_bf16: the centred pose and the projection leave as bf16 (the rounding the critics apply on load anyway)."""
    h = _dev(head, torch.float32, "gen_tail_forward_critics").reshape(-1, 35)
    b = _dev(bone_len, torch.float32, "gen_tail_forward_critics").reshape(-1, 15)
    s = None if scaler is None else _dev(scaler, torch.float32, "gen_tail_forward_critics").reshape(-1, 8)
    N = h.shape[0]
    assert b.shape[0] == N and (s is None or s.shape[0] == N)
    fake = torch.empty((N, 16, 3), dtype=torch.float32, device=h.device)
    idt = BF16 if inputs_bf16 else torch.float32
    xc = torch.empty((N, 48), dtype=idt, device=h.device) if want_critic_inputs else None
    kcs = torch.empty((N, 32), dtype=BF16, device=h.device) if want_critic_inputs else None
    p2 = q = t = c = None
    if camera is not None:
        p2 = torch.empty((N, 16, 2), dtype=idt, device=h.device)
        q, t, c = _host3(camera[0], 4), _host3(camera[1], 3), _host3(camera[2], 9)
    so = torch.empty((N, 8), dtype=torch.float32, device=h.device) if (rng is not None and want_scaler) else None
    _lib.call("dhaug_gen_tail_forward_critics", _p(h), _p(b), _p(s), _p(fake), _p(xc), _p(kcs), q, t, c, _p(p2),
              int(rng is not None), 0 if rng is None else int(rng[0]) & (2 ** 64 - 1), 0 if rng is None else int(rng[1]), _p(so),
              N, int(bool(use_preangle)), int(bool(inputs_bf16)), _stream())
    if want_scaler:
        return fake, xc, kcs, p2, so
    return fake, xc, kcs, p2


def gen_tail_backward(head, bone_len, scaler, grad_fake16, use_preangle=True):
    h = _dev(head, torch.float32, "gen_tail_backward").reshape(-1, 35)
    b = _dev(bone_len, torch.float32, "gen_tail_backward").reshape(-1, 15)
    s = None if scaler is None else _dev(scaler, torch.float32, "gen_tail_backward").reshape(-1, 8)
    g = _dev(grad_fake16, torch.float32, "gen_tail_backward").reshape(-1, 48)
    N = h.shape[0]
    gh = torch.empty((N, 35), dtype=torch.float32, device=h.device)
    _lib.call("dhaug_gen_tail_backward", _p(h), _p(b), _p(s), _p(g), _p(gh), N, int(bool(use_preangle)), _stream())
    return gh


# ------------------------------------------------------------------------------------- pose features
def bone_length(pose16):
    x = _dev(pose16, torch.float32, "bone_length").reshape(-1, 48)
    out = torch.empty((x.shape[0], 15), dtype=torch.float32, device=x.device)
    _lib.call("dhaug_bone_length", _p(x), _p(out), x.shape[0], _stream())
    return out


def kcs_forward(pose16, with_lengths=True, f32=True, bf16_ld=0):
    x = _dev(pose16, torch.float32, "kcs_forward").reshape(-1, 48)
    N, W = x.shape[0], (30 if with_lengths else 15)
    of = torch.empty((N, W), dtype=torch.float32, device=x.device) if f32 else None
    ob = torch.empty((N, bf16_ld), dtype=BF16, device=x.device) if bf16_ld else None
    _lib.call("dhaug_kcs_forward", _p(x), _p(of), _p(ob), bf16_ld, N, int(with_lengths), _stream())
    return of, ob


def center_kcs_forward(pose16, bf16_ld=32, with_lengths=True):
    """root-relative pose (N,48) fp32 and the bf16 KCS operand of the 3D critic in one pass over the pose"""
    x = _dev(pose16, torch.float32, "center_kcs_forward").reshape(-1, 48)
    N = x.shape[0]
    xc = torch.empty((N, 48), dtype=torch.float32, device=x.device)
    ob = torch.empty((N, bf16_ld), dtype=BF16, device=x.device)
    _lib.call("dhaug_center_kcs_forward", _p(x), _p(xc), _p(ob), bf16_ld, N, int(with_lengths), _stream())
    return xc, ob


def kcs_backward(pose16, grad_feat, with_lengths=True):
    x = _dev(pose16, torch.float32, "kcs_backward").reshape(-1, 48)
    g = _dev(grad_feat, torch.float32, "kcs_backward").reshape(x.shape[0], 30 if with_lengths else 15)
    out = torch.empty((x.shape[0], 48), dtype=torch.float32, device=x.device)
    _lib.call("dhaug_kcs_backward", _p(x), _p(g), _p(out), x.shape[0], int(with_lengths), _stream())
    return out


def kcs_jvp(pose16, tangent, with_lengths=True):
    x = _dev(pose16, torch.float32, "kcs_jvp").reshape(-1, 48)
    t = _dev(tangent, torch.float32, "kcs_jvp").reshape(-1, 48)
    out = torch.empty((x.shape[0], 30 if with_lengths else 15), dtype=torch.float32, device=x.device)
    _lib.call("dhaug_kcs_jvp", _p(x), _p(t), _p(out), x.shape[0], int(with_lengths), _stream())
    return out


# -------------------------------------------------------------------------------------------- camera
def world_to_camera_project(pose16, quat, trans, cam9, want3d=True, want2d=True):
    x = _dev(pose16, torch.float32, "world_to_camera_project").reshape(-1, 48)
    N = x.shape[0]
    c3 = torch.empty((N, 16, 3), dtype=torch.float32, device=x.device) if want3d else None
    p2 = torch.empty((N, 16, 2), dtype=torch.float32, device=x.device) if want2d else None
    _lib.call("dhaug_world_to_camera_project", _p(x), _host3(quat, 4), _host3(trans, 3),
              None if cam9 is None else _host3(cam9, 9), _p(c3), _p(p2), N, _stream())
    return c3, p2


def world_to_camera_project_backward(pose16, quat, trans, cam9, grad3d, grad2d):
    x = _dev(pose16, torch.float32, "w2c_backward").reshape(-1, 48)
    g3 = None if grad3d is None else _dev(grad3d, torch.float32, "w2c_backward").reshape(-1, 48)
    g2 = None if grad2d is None else _dev(grad2d, torch.float32, "w2c_backward").reshape(-1, 32)
    out = torch.empty((x.shape[0], 16, 3), dtype=torch.float32, device=x.device)
    _lib.call("dhaug_world_to_camera_project_backward", _p(x), _host3(quat, 4), _host3(trans, 3),
              None if cam9 is None else _host3(cam9, 9), _p(g3), _p(g2), _p(out), x.shape[0], _stream())
    return out


def camera_to_world(cam3d, quat, trans):
    x = _dev(cam3d, torch.float32, "camera_to_world").reshape(-1, 48)
    q = _dev(quat, torch.float32, "camera_to_world").reshape(-1, 4)
    t = _dev(trans, torch.float32, "camera_to_world").reshape(-1, 3)
    assert q.shape[0] == x.shape[0] and t.shape[0] == x.shape[0]
    out = torch.empty((x.shape[0], 16, 3), dtype=torch.float32, device=x.device)
    _lib.call("dhaug_camera_to_world", _p(x), _p(q), _p(t), _p(out), x.shape[0], _stream())
    return out


def bone_length_swap(pose16, new_len):
    x = _dev(pose16, torch.float32, "bone_length_swap").reshape(-1, 48)
    l = _dev(new_len, torch.float32, "bone_length_swap").reshape(-1, 15)
    assert l.shape[0] == x.shape[0]
    out = torch.empty((x.shape[0], 16, 3), dtype=torch.float32, device=x.device)
    _lib.call("dhaug_bone_length_swap", _p(x), _p(l), _p(out), x.shape[0], _stream())
    return out


def project_to_2d(cam3d, cam9):
    x = _dev(cam3d, torch.float32, "project_to_2d").reshape(-1, 48)
    c = _dev(cam9, torch.float32, "project_to_2d")[:, :9].contiguous()
    assert c.shape[0] == x.shape[0]
    out = torch.empty((x.shape[0], 16, 2), dtype=torch.float32, device=x.device)
    _lib.call("dhaug_project_to_2d", _p(x), _p(c), _p(out), x.shape[0], _stream())
    return out


def clip_gather(seq3d, seq2d, cams, seq_offset, seq_len, records, frames, pad, causal_shift=0, perm3d=None, perm2d=None,
                out3d=None, out2d=None, out_cam=None):
    """clips of the video loader (dhaug_clip_gather): seq3d (T,16,3) or None, seq2d (T,16,2), cams (S,cam_w) or None,
    seq_offset (S,) int64, seq_len (S,) int32, records (nrec,4) int32 -> (out_cam, out3d, out2d) as (nrec, cam_w),
    (nrec, frames, 16, 3), (nrec, frames, 16, 2); None where the input is None.  perm3d / perm2d: host sequences of 16
    joint indices (None = identity).  out*: optional preallocated outputs of those shapes."""
    s2 = _dev(seq2d, torch.float32, "clip_gather").reshape(-1, 32)
    s3 = None if seq3d is None else _dev(seq3d, torch.float32, "clip_gather").reshape(-1, 48)
    c = None if cams is None else _dev(cams, torch.float32, "clip_gather")
    off = _dev(seq_offset, torch.int64, "clip_gather")
    ln = _dev(seq_len, torch.int32, "clip_gather")
    rec = _dev(records, torch.int32, "clip_gather").reshape(-1, 4)
    n, dev = rec.shape[0], s2.device
    cam_w = 0 if c is None else c.reshape(c.shape[0], -1).shape[1]

    def out(t, shape):
        if t is None:
            return torch.empty(shape, dtype=torch.float32, device=dev)
        assert t.dtype == torch.float32 and t.is_cuda and t.is_contiguous() and tuple(t.shape) == shape, "clip_gather output"
        return t

    o2 = out(out2d, (n, frames, 16, 2))
    o3 = None if s3 is None else out(out3d, (n, frames, 16, 3))
    oc = None if c is None else out(out_cam, (n, cam_w))
    perm = lambda p: None if p is None else (ctypes.c_int8 * 16)(*[int(v) for v in p])
    _lib.call("dhaug_clip_gather", _p(s3), _p(s2), _p(c), cam_w, _p(off), _p(ln), _p(rec), n, int(frames), int(pad),
              int(causal_shift), perm(perm3d), perm(perm2d), _p(o3), _p(o2), _p(oc), _stream())
    return oc, o3, o2


def _perm8(p):
    return None if p is None else (ctypes.c_int8 * 16)(*[int(v) for v in p])


def _clip_inputs(seq3d, seq2d, seq_offset, seq_len, records, name):
    s2 = None if seq2d is None else _dev(seq2d, torch.float32, name).reshape(-1, 32)
    s3 = None if seq3d is None else _dev(seq3d, torch.float32, name).reshape(-1, 48)
    return (s3, s2, _dev(seq_offset, torch.int64, name), _dev(seq_len, torch.int32, name),
            _dev(records, torch.int32, name).reshape(-1, 4))


def _clip_out(t, shape, dev, name):
    if t is None:
        return torch.empty(shape, dtype=torch.float32, device=dev)
    if not (t.dtype == torch.float32 and t.is_cuda and t.is_contiguous() and tuple(t.shape) == shape):
        raise ValueError("%s: a preallocated output must be a contiguous fp32 device tensor of shape %s" % (name, shape))
    return t


def clip_gather_windows(seq3d, seq2d, cams, seq_offset, seq_len, records, frames3, shift3, frames2, shift2, perm3d=None,
                        perm2d=None, out3d=None, out2d=None, out_cam=None):
    """clip_gather with a window of its own for the 3D and the 2D frames (dhaug_clip_gather_windows): output frame f of record
    (seq, start, end, flip) is frame clamp(start - shift + f, 0, len - 1) of the sequence.  Arguments as clip_gather; returns
    (out_cam (nrec, cam_w), out3d (nrec, frames3, 16, 3), out2d (nrec, frames2, 16, 2)), None where the input is None."""
    frames3, shift3, frames2, shift2 = int(frames3), int(shift3), int(frames2), int(shift2)
    if frames3 < 1 or frames2 < 1:
        raise ValueError("clip_gather_windows: frames3 and frames2 must be >= 1, got %d and %d" % (frames3, frames2))
    s3, s2, off, ln, rec = _clip_inputs(seq3d, seq2d, seq_offset, seq_len, records, "clip_gather_windows")
    c = None if cams is None else _dev(cams, torch.float32, "clip_gather_windows")
    n, dev = rec.shape[0], s2.device
    cam_w = 0 if c is None else c.reshape(c.shape[0], -1).shape[1]
    o2 = _clip_out(out2d, (n, frames2, 16, 2), dev, "clip_gather_windows")
    o3 = None if s3 is None else _clip_out(out3d, (n, frames3, 16, 3), dev, "clip_gather_windows")
    oc = None if c is None else _clip_out(out_cam, (n, cam_w), dev, "clip_gather_windows")
    _lib.call("dhaug_clip_gather_windows", _p(s3), _p(s2), _p(c), cam_w, _p(off), _p(ln), _p(rec), n, frames3, shift3, frames2,
              shift2, _perm8(perm3d), _perm8(perm2d), _p(o3), _p(o2), _p(oc), _stream())
    return oc, o3, o2


def clip_pair_batch(seq3d, seq2d, seq_offset, seq_len, records, frames3, shift3, frames2, shift2, perm3d=None, perm2d=None,
                    flip=False, playback=False, out=None):
    """pair_batch of the clips clip_gather_windows would write, in one launch from the resident sequences
    (dhaug_clip_pair_batch).  Returns pair_batch's dict: tgt (nrec, frames3, 16, 3) root-centred, inp (nrec, frames2, 16, 2);
    flip: tgt_flip, inp_flip; playback: inp_back (and inp_flip_back with flip).  out: optional dict of preallocated outputs
    under those names (the others are allocated)."""
    frames3, shift3, frames2, shift2 = int(frames3), int(shift3), int(frames2), int(shift2)
    if frames3 < 1 or frames2 < 1:
        raise ValueError("clip_pair_batch: frames3 and frames2 must be >= 1, got %d and %d" % (frames3, frames2))
    if seq3d is None or seq2d is None:
        raise ValueError("clip_pair_batch: a training batch needs the 3D and the 2D sequences")
    s3, s2, off, ln, rec = _clip_inputs(seq3d, seq2d, seq_offset, seq_len, records, "clip_pair_batch")
    n, dev = rec.shape[0], s2.device
    shapes = dict(tgt=(n, frames3, 16, 3), inp=(n, frames2, 16, 2))
    if flip:
        shapes.update(tgt_flip=shapes["tgt"], inp_flip=shapes["inp"])
    if playback:
        shapes.update(inp_back=shapes["inp"])
        if flip:
            shapes.update(inp_flip_back=shapes["inp"])
    given = {} if out is None else out
    if set(given) - set(shapes):
        raise ValueError("clip_pair_batch: outputs %s are not produced with flip=%s playback=%s"
                         % (sorted(set(given) - set(shapes)), bool(flip), bool(playback)))
    res = {k: _clip_out(given.get(k), shape, dev, "clip_pair_batch") for k, shape in shapes.items()}
    g = lambda k: _p(res.get(k))
    _lib.call("dhaug_clip_pair_batch", _p(s3), _p(s2), _p(off), _p(ln), _p(rec), n, frames3, shift3, frames2, shift2,
              _perm8(perm3d), _perm8(perm2d), int(bool(flip)), int(bool(playback)), g("tgt"), g("inp"), g("tgt_flip"),
              g("inp_flip"), g("inp_back"), g("inp_flip_back"), _stream())
    return res


def eval_totals(device=None):
    """a zeroed device totals record of pose_metrics (struct dhaug_eval_totals as int64 words: sum_err and sum_pmpjpe are
    fp64 bit patterns, then poses and tp[32])"""
    return torch.zeros(_lib.EVAL_TOTALS_WORDS, dtype=torch.int64, device=device if device is not None else "cuda")


def pose_metrics(pred, target, center=False, thresholds=(), multiplicity=None, per_pose=False, totals=None):
    """evaluation metrics of (P, 16, 3) poses (dhaug_pose_metrics): per-joint error, PCK counts and P-MPJPE.
    thresholds: up to 32 host floats in mm (compared with fl32(error * 1000)); multiplicity: 16 host ints (joint weights of
    the PCK counts, None = 1 each); totals: a record of eval_totals() accumulated into (stream order, no host read).
    Returns (mpjpe, pmpjpe) as fp32 (P,) device tensors when per_pose, else (None, None)."""
    if tuple(pred.shape) != tuple(target.shape):
        raise ValueError("pose_metrics: pred %s and target %s differ in shape" % (tuple(pred.shape), tuple(target.shape)))
    if pred.dim() < 2 or tuple(pred.shape[-2:]) != (16, 3):
        raise ValueError("pose_metrics: poses must be (..., 16, 3), got %s" % (tuple(pred.shape),))
    thr = [float(t) for t in thresholds]
    if len(thr) > _lib.EVAL_MAX_THRESHOLDS:
        raise ValueError("pose_metrics: at most %d thresholds, got %d" % (_lib.EVAL_MAX_THRESHOLDS, len(thr)))
    if totals is None and not per_pose:
        raise ValueError("pose_metrics: nothing to compute (no totals and per_pose=False)")
    y = _dev(pred, torch.float32, "pose_metrics").reshape(-1, 48)
    x = _dev(target, torch.float32, "pose_metrics").reshape(-1, 48)
    P, dev = y.shape[0], y.device
    m = None
    if multiplicity is not None:
        m = [int(v) for v in multiplicity]
        if len(m) != 16 or any(v < 0 or v > _lib.EVAL_MAX_MULTIPLICITY for v in m):
            raise ValueError("pose_metrics: multiplicity must be 16 ints in [0, %d]" % _lib.EVAL_MAX_MULTIPLICITY)
        m = (ctypes.c_int32 * 16)(*m)
    ws = None
    if totals is not None:
        assert totals.is_cuda and totals.dtype == torch.int64 and totals.numel() == _lib.EVAL_TOTALS_WORDS \
            and totals.is_contiguous(), "pose_metrics: totals must come from eval_totals()"
        ws = torch.empty(_lib.EVAL_WORKSPACE_BYTES // 8, dtype=torch.int64, device=dev)
    mp = torch.empty(P, dtype=torch.float32, device=dev) if per_pose else None
    pp = torch.empty(P, dtype=torch.float32, device=dev) if per_pose else None
    _lib.call("dhaug_pose_metrics", _p(y), _p(x), P, int(bool(center)), (ctypes.c_double * max(1, len(thr)))(*thr),
              len(thr), m, _p(mp), _p(pp), _p(totals), _p(ws), _stream())
    return mp, pp


def _f64_sums(t, n, name, what):
    assert t.is_cuda and t.dtype == torch.float64 and t.numel() == n and t.is_contiguous(), \
        "%s: %s must be a contiguous fp64 device tensor of %d elements" % (name, what, n)
    return t


def pose_column_errors(pred, target, center=False, col_sums=None, vel_sum=None):
    """per-column sums of the joint error and the velocity-error sum of (rows, ..., 3) joints (dhaug_pose_column_errors): the
    first axis is the rows, the axes between it and the last one are flattened into the columns.  col_sums: fp64 (cols,)
    device tensor, += the sum over the rows of |pred - target| per column; vel_sum: fp64 (1,) device tensor, += the sum over
    consecutive row pairs and columns of |diff(pred) - diff(target)|.  Both are accumulated into (stream order, no host read);
    at least one must be given.  center: each group of 16 columns is root-centred first.  Returns (col_sums, vel_sum)."""
    name = "pose_column_errors"
    if tuple(pred.shape) != tuple(target.shape):
        raise ValueError("%s: pred %s and target %s differ in shape" % (name, tuple(pred.shape), tuple(target.shape)))
    if pred.dim() < 2 or pred.shape[-1] != 3:
        raise ValueError("%s: joints must be (rows, ..., 3), got %s" % (name, tuple(pred.shape)))
    if col_sums is None and vel_sum is None:
        raise ValueError("%s: nothing to compute (no col_sums and no vel_sum)" % name)
    rows, cols = pred.shape[0], 1
    for d in pred.shape[1:-1]:
        cols *= d
    if cols % 4 or cols > _lib.COLERR_MAX_COLS or (center and cols % 16):
        raise ValueError("%s: %d columns: need a multiple of %d, at most %d" % (name, cols, 16 if center else 4, _lib.COLERR_MAX_COLS))
    y = _dev(pred, torch.float32, name)
    x = _dev(target, torch.float32, name)
    if col_sums is not None:
        _f64_sums(col_sums, cols, name, "col_sums")
    if vel_sum is not None:
        _f64_sums(vel_sum, 1, name, "vel_sum")
    ws = torch.empty(_lib.COLERR_WORKSPACE_BYTES // 8, dtype=torch.float64, device=y.device)
    _lib.call("dhaug_pose_column_errors", _p(y), _p(x), rows, cols, int(bool(center)), _p(col_sums), _p(vel_sum), _p(ws), _stream())
    return col_sums, vel_sum


def pose_scaled_errors(pred, target, center=False, w=None, sums=None):
    """the N-MPJPE and weighted error sums of (..., 16, 3) poses (dhaug_pose_scaled_errors).  sums: fp64 (2,) device tensor
    accumulated into (a zeroed one is made when None): sums[0] += the sum of |s pred - target| over all joints, s the pose's
    least-squares scale; sums[1] += the sum of w |pred - target|, w fp32 with one value per pose (P elements) or per joint
    (16 P elements), untouched without w.  Returns sums."""
    name = "pose_scaled_errors"
    if tuple(pred.shape) != tuple(target.shape):
        raise ValueError("%s: pred %s and target %s differ in shape" % (name, tuple(pred.shape), tuple(target.shape)))
    if pred.dim() < 2 or tuple(pred.shape[-2:]) != (16, 3):
        raise ValueError("%s: poses must be (..., 16, 3), got %s" % (name, tuple(pred.shape)))
    P = pred.numel() // 48
    if w is not None and w.numel() not in (P, 16 * P):
        raise ValueError("%s: w must hold one value per pose (%d) or per joint (%d), got %s" % (name, P, 16 * P, tuple(w.shape)))
    y = _dev(pred, torch.float32, name)
    x = _dev(target, torch.float32, name)
    per_joint = w is not None and P > 0 and w.numel() == 16 * P
    wd = None if w is None else _dev(w, torch.float32, name)
    if sums is None:
        sums = torch.zeros(2, dtype=torch.float64, device=y.device)
    _f64_sums(sums, 2, name, "sums")
    ws = torch.empty(_lib.SCALEDERR_WORKSPACE_BYTES // 8, dtype=torch.float64, device=y.device)
    _lib.call("dhaug_pose_scaled_errors", _p(y), _p(x), P, int(bool(center)), _p(wd), int(per_joint), _p(sums), _p(ws), _stream())
    return sums


# ---------------------------------------------------------------------------------------------- DOF angle distributions
def dof_record(D=37, device=None):
    """a fresh record of dof_histogram for D slots: _lib.dof_record_offsets(D)['words'] int64 words (the fp64 fields are bit
    patterns: view(torch.float64)), zeros with min = +inf and max = -inf"""
    D = int(D)
    if not 1 <= D <= _lib.DOF_MAX_SLOTS:
        raise ValueError("dof_record: D must be in 1..%d, got %r" % (_lib.DOF_MAX_SLOTS, D))
    off = _lib.dof_record_offsets(D)
    rec = torch.zeros(off["words"], dtype=torch.int64, device=device if device is not None else "cuda")
    f = rec.view(torch.float64)
    f[off["min"]:off["min"] + D] = float("inf")
    f[off["max"]:off["max"] + D] = float("-inf")
    return rec


def _dof_rows(angles, name):
    """the angle table as fp32 (rows, D) with unit column stride (a row pitch >= D is passed on as it is: no copy)"""
    if not torch.is_tensor(angles) or angles.dim() != 2:
        raise ValueError("%s: angles must be a (rows, D) tensor, got %s"
                         % (name, tuple(angles.shape) if torch.is_tensor(angles) else type(angles).__name__))
    rows, D = angles.shape
    if not 1 <= D <= _lib.DOF_MAX_SLOTS:
        raise ValueError("%s: D must be in 1..%d, got %d" % (name, _lib.DOF_MAX_SLOTS, D))
    a = angles if angles.dtype == torch.float32 else angles.float()
    if rows > 1 and (a.stride(1) != 1 or a.stride(0) < D):
        a = a.contiguous()
    elif rows <= 1 and D > 1 and a.stride(1) != 1:
        a = a.contiguous()
    return a, rows, D, (a.stride(0) if rows > 1 else D)


def _dof_residual(residual, max_residual, rows, name):
    if residual is None:
        if max_residual is not None:
            raise ValueError("%s: max_residual goes with a residual" % name)
        return None, 0.0
    if max_residual is None:
        raise ValueError("%s: a residual needs max_residual" % name)
    if not torch.is_tensor(residual) or residual.numel() != rows:
        raise ValueError("%s: residual must hold one value per row (%d)" % (name, rows))
    r = residual.reshape(-1)
    return (r if r.dtype == torch.float32 else r.float()).contiguous(), float(max_residual)


def _dof_on_device(name, *tensors):
    """every ValueError of a DOF entry comes before this check, so the refusals can be tested without a GPU"""
    if any(t is not None and not t.is_cuda for t in tensors):
        raise RuntimeError("dhaug op `%s` needs GPU tensors (no CPU fallback exists)" % name)


def dof_histogram(angles, record, residual=None, max_residual=None, lo=None, hi=None, tol=0.0):
    """record += the per-slot one-degree histograms (bin = int(angle) + 180 of 361), NaN / outside / at-limit counts, exact
    min / max and fp64 sums of angles (rows, D) fp32 (dhaug_dof_histogram; a row-strided view is read in place).  record comes
    from dof_record(D).  residual (rows) with max_residual: rows whose residual is larger, or NaN, are left out and counted in
    `skipped`.  lo / hi: (D,) device tensors (both or neither) for at_lo += a <= fl32(lo + tol), at_hi += a >= fl32(hi - tol).
    Enqueues two launches on the current stream; no host read.  ValueError before any launch for a bad argument."""
    name = "dof_histogram"
    a, rows, D, pitch = _dof_rows(angles, name)
    words = _lib.dof_record_offsets(D)["words"]
    if not (torch.is_tensor(record) and record.dtype == torch.int64 and record.numel() == words and record.is_contiguous()):
        raise ValueError("%s: record must come from dof_record(%d) (%d int64 words)" % (name, D, words))
    if (lo is None) != (hi is None):
        raise ValueError("%s: lo and hi come together" % name)
    if lo is not None:
        if not (torch.is_tensor(lo) and torch.is_tensor(hi) and lo.numel() == D and hi.numel() == D):
            raise ValueError("%s: lo and hi are tensors of %d entries each" % (name, D))
        lo, hi = lo.reshape(-1).float().contiguous(), hi.reshape(-1).float().contiguous()
    if not float(tol) >= 0.0:
        raise ValueError("%s: tol must not be negative, got %r" % (name, tol))
    res, mr = _dof_residual(residual, max_residual, rows, name)
    _dof_on_device(name, a, record, res, lo, hi)
    ws = torch.empty(_lib.DOF_WORKSPACE_BYTES // 8, dtype=torch.float64, device=a.device)
    _lib.call("dhaug_dof_histogram", _p(a), rows, D, pitch, _p(res), mr, _p(lo), _p(hi), float(tol), _p(record), _p(ws), _stream())
    return record


def dof_pairs(pairs, D, name="dof_pair_histogram"):
    """slot pairs as a list of (i, j) ints, checked as dhaug_dof_pair_histogram checks them"""
    try:
        out = [(int(i), int(j)) for i, j in pairs]
    except (TypeError, ValueError):
        raise ValueError("%s: pairs is a sequence of (i, j) slot pairs" % name)
    if len(out) > _lib.DOF_MAX_PAIRS:
        raise ValueError("%s: at most %d pairs per call, got %d" % (name, _lib.DOF_MAX_PAIRS, len(out)))
    bad = [p for p in out if not (0 <= p[0] < D and 0 <= p[1] < D)]
    if bad:
        raise ValueError("%s: slot(s) outside [0, %d) in %s" % (name, D, bad))
    return out


def dof_pair_histogram(angles, pairs, table, residual=None, max_residual=None):
    """table[p][bin(a_i)][bin(a_j)] += 1 over the rows of angles (rows, D) for the slot pairs p = (i, j), at most 4 per call
    (dhaug_dof_pair_histogram).  table: int64 (len(pairs), 361, 361) on the device, accumulated into.  Same binning and skip
    rule as dof_histogram; a row with a NaN in either slot of a pair is left out of that pair."""
    name = "dof_pair_histogram"
    a, rows, D, pitch = _dof_rows(angles, name)
    pr = dof_pairs(pairs, D, name)
    n = len(pr)
    if not (torch.is_tensor(table) and table.dtype == torch.int64 and table.is_contiguous()
            and tuple(table.shape) == (n, _lib.DOF_BINS, _lib.DOF_BINS)):
        raise ValueError("%s: table must be a contiguous int64 tensor of shape (%d, %d, %d)"
                         % (name, n, _lib.DOF_BINS, _lib.DOF_BINS))
    res, mr = _dof_residual(residual, max_residual, rows, name)
    _dof_on_device(name, a, table, res)
    if n == 0:
        return table
    flat = [v for p in pr for v in p]
    _lib.call("dhaug_dof_pair_histogram", _p(a), rows, D, pitch, _p(res), mr, (ctypes.c_int * (2 * n))(*flat), n, _p(table),
              _stream())
    return table


def center_flip(x, center, flip, adjoint=False):
    C = x.shape[-1]
    v = _dev(x, torch.float32, "center_flip").reshape(-1, 16 * C)
    out = torch.empty_like(v)
    _lib.call("dhaug_center_flip_backward" if adjoint else "dhaug_center_flip", _p(v), _p(out), v.shape[0], C,
              int(bool(center)), int(bool(flip)), _stream())
    return out.reshape(-1, 16, C)


# ---------------------------------------------------------------------------------------------- posenet training
def posetrain_workspace(device=None):
    """the partials' workspace of pose_mse / pose_mpjpe / grad_sumsq / adam_clip_step (one call chain at a time per workspace)"""
    return torch.empty(_lib.POSETRAIN_WORKSPACE_BYTES // 8, dtype=torch.int64, device=device if device is not None else "cuda")


def loss_meters(count=1, device=None):
    """count zeroed device meter records (struct dhaug_loss_meter as int64 words: sum_loss_x_poses as fp64 bits, poses, steps)"""
    return torch.zeros((count, _lib.LOSS_METER_WORDS), dtype=torch.int64, device=device if device is not None else "cuda")


def pair_batch(p3, p2, idx=None, n=None, flip=False, playback=False):
    """the tensors of one posenet training iteration in one launch (dhaug_pair_batch).  p3 (M, [F3,] 16, 3), p2 (M, [F2,] 16, 2);
    idx: int64 device indices into the M rows (None: rows 0..n-1, n defaulting to M).  Returns a dict: tgt (n,F3,16,3)
    root-centred, inp (n,F2,16,2); flip: tgt_flip, inp_flip; playback: inp_back (and inp_flip_back with flip)."""
    if p3.dim() not in (3, 4) or tuple(p3.shape[-2:]) != (16, 3):
        raise ValueError("pair_batch: p3 must be (M, 16, 3) or (M, F, 16, 3), got %s" % (tuple(p3.shape),))
    if p2.dim() not in (3, 4) or tuple(p2.shape[-2:]) != (16, 2):
        raise ValueError("pair_batch: p2 must be (M, 16, 2) or (M, F, 16, 2), got %s" % (tuple(p2.shape),))
    M = p3.shape[0]
    if p2.shape[0] != M:
        raise ValueError("pair_batch: p3 has %d rows, p2 %d" % (M, p2.shape[0]))
    F3 = p3.shape[1] if p3.dim() == 4 else 1
    F2 = p2.shape[1] if p2.dim() == 4 else 1
    if idx is not None:
        if idx.dim() != 1 or idx.dtype != torch.int64:
            raise ValueError("pair_batch: idx must be a 1-D int64 tensor")
        if n is not None and n != idx.shape[0]:
            raise ValueError("pair_batch: n = %d but idx holds %d indices" % (n, idx.shape[0]))
        n = idx.shape[0]
    else:
        n = M if n is None else int(n)
        if n < 0 or n > M:
            raise ValueError("pair_batch: n = %d outside 0..%d" % (n, M))
    if F3 < 1 or F2 < 1 or n * max(F3, F2) >= (1 << 31) // 48:
        raise ValueError("pair_batch: n * frames must be in [0, 2^31 / 48)")
    x3 = _dev(p3, torch.float32, "pair_batch")
    x2 = _dev(p2, torch.float32, "pair_batch")
    ix = None if idx is None else _dev(idx, torch.int64, "pair_batch")
    dev = x3.device
    new = lambda F, C: torch.empty((n, F, 16, C), dtype=torch.float32, device=dev)
    out = dict(tgt=new(F3, 3), inp=new(F2, 2))
    if flip:
        out.update(tgt_flip=new(F3, 3), inp_flip=new(F2, 2))
    if playback:
        out.update(inp_back=new(F2, 2))
        if flip:
            out.update(inp_flip_back=new(F2, 2))
    g = lambda k: _p(out.get(k))
    _lib.call("dhaug_pair_batch", _p(x3), _p(x2), M, F3, F2, _p(ix), n, int(bool(flip)), int(bool(playback)), g("tgt"), g("inp"),
              g("tgt_flip"), g("inp_flip"), g("inp_back"), g("inp_flip_back"), _stream())
    return out


def pose_mse(pred, target, poses, meter=None, workspace=None, loss=None):
    """nn.MSELoss(reduction='mean') forward + backward (dhaug_pose_mse): returns (loss, grad), loss a 1-element fp32 device
    tensor (or the one given), grad = d loss / d pred in pred's shape.  meter: one record of loss_meters(), accumulated into
    (AverageMeter.update(loss, poses) on the device)."""
    if tuple(pred.shape) != tuple(target.shape):
        raise ValueError("pose_mse: pred %s and target %s differ in shape" % (tuple(pred.shape), tuple(target.shape)))
    if int(poses) < 0:
        raise ValueError("pose_mse: poses must be >= 0")
    y = _dev(pred.detach(), torch.float32, "pose_mse")
    x = _dev(target, torch.float32, "pose_mse")
    dev = y.device
    if meter is not None:
        assert meter.is_cuda and meter.dtype == torch.int64 and meter.numel() == _lib.LOSS_METER_WORDS and meter.is_contiguous(), \
            "pose_mse: meter must be one record of loss_meters()"
    ws = workspace if workspace is not None else posetrain_workspace(dev)
    grad = torch.empty_like(y)
    if loss is None:
        loss = torch.empty(1, dtype=torch.float32, device=dev)
    assert loss.is_cuda and loss.dtype == torch.float32 and loss.numel() == 1
    _lib.call("dhaug_pose_mse", _p(y), _p(x), y.numel(), int(poses), _p(grad), _p(loss), _p(meter), _p(ws), _stream())
    return loss, grad


def pose_mpjpe(pred, target, poses, meter=None, workspace=None, loss=None):
    """mpjpe = mean(norm(pred - target, dim=-1)) forward + backward (dhaug_pose_mpjpe) over (..., 3) rows: returns (loss, grad)
    with pose_mse's conventions -- loss a 1-element fp32 device tensor (or the one given), grad = d loss / d pred in pred's
    shape (exactly 0 for a joint at distance 0), meter one record of loss_meters()."""
    if tuple(pred.shape) != tuple(target.shape):
        raise ValueError("pose_mpjpe: pred %s and target %s differ in shape" % (tuple(pred.shape), tuple(target.shape)))
    if pred.dim() < 1 or pred.shape[-1] != 3:
        raise ValueError("pose_mpjpe: the last dimension must be 3, got %s" % (tuple(pred.shape),))
    if int(poses) < 0:
        raise ValueError("pose_mpjpe: poses must be >= 0")
    y = _dev(pred.detach(), torch.float32, "pose_mpjpe")
    x = _dev(target.detach(), torch.float32, "pose_mpjpe")
    dev = y.device
    if meter is not None:
        assert meter.is_cuda and meter.dtype == torch.int64 and meter.numel() == _lib.LOSS_METER_WORDS and meter.is_contiguous(), \
            "pose_mpjpe: meter must be one record of loss_meters()"
    ws = workspace if workspace is not None else posetrain_workspace(dev)
    grad = torch.empty_like(y)
    if loss is None:
        loss = torch.empty(1, dtype=torch.float32, device=dev)
    assert loss.is_cuda and loss.dtype == torch.float32 and loss.numel() == 1
    _lib.call("dhaug_pose_mpjpe", _p(y), _p(x), y.numel() // 3, int(poses), _p(grad), _p(loss), _p(meter), _p(ws), _stream())
    return loss, grad


def _pose_criterion(name, pred, target, poses, meter, workspace, loss):
    """the checks and outputs pose_nmpjpe and pose_wmpjpe share: (y, x, P, grad, loss, workspace)"""
    if tuple(pred.shape) != tuple(target.shape):
        raise ValueError("%s: pred %s and target %s differ in shape" % (name, tuple(pred.shape), tuple(target.shape)))
    if pred.dim() < 2 or tuple(pred.shape[-2:]) != (16, 3):
        raise ValueError("%s: poses must be (..., 16, 3), got %s" % (name, tuple(pred.shape)))
    if int(poses) < 0:
        raise ValueError("%s: poses must be >= 0" % name)
    y = _dev(pred.detach(), torch.float32, name)
    x = _dev(target.detach(), torch.float32, name)
    dev = y.device
    if meter is not None:
        assert meter.is_cuda and meter.dtype == torch.int64 and meter.numel() == _lib.LOSS_METER_WORDS and meter.is_contiguous(), \
            "%s: meter must be one record of loss_meters()" % name
    ws = workspace if workspace is not None else posetrain_workspace(dev)
    grad = torch.empty_like(y)
    if loss is None:
        loss = torch.empty(1, dtype=torch.float32, device=dev)
    assert loss.is_cuda and loss.dtype == torch.float32 and loss.numel() == 1
    return y, x, y.numel() // 48, grad, loss, ws


def pose_nmpjpe(pred, target, poses, meter=None, workspace=None, loss=None):
    """n_mpjpe forward + backward (dhaug_pose_nmpjpe) over (..., 16, 3) poses, each scaled by its own least-squares scale: returns
    (loss, grad) with pose_mpjpe's conventions.  `poses` is what the meter counts (the batch size), not the number of (16, 3)
    poses, which follows from the shape.  An all-zero predicted pose gives a NaN loss and NaN for that pose's gradient."""
    y, x, P, grad, loss, ws = _pose_criterion("pose_nmpjpe", pred, target, poses, meter, workspace, loss)
    _lib.call("dhaug_pose_nmpjpe", _p(y), _p(x), P, int(poses), _p(grad), _p(loss), _p(meter), _p(ws), _stream())
    return loss, grad


def wmpjpe_mode(w_shape, joint_shape):
    """the w_mode of dhaug_pose_wmpjpe from w's shape against pred.shape[:-1]: per pose for (..., 1), per pose and joint for the
    full shape, shared for (16,) -- the first that fits; None for any other shape"""
    w_shape, joint_shape = tuple(w_shape), tuple(joint_shape)
    if w_shape == joint_shape[:-1] + (1,):
        return _lib.WMPJPE_PER_POSE
    if w_shape == joint_shape:
        return _lib.WMPJPE_PER_JOINT
    if w_shape == (16,):
        return _lib.WMPJPE_SHARED
    return None


def pose_wmpjpe(pred, target, w, poses, meter=None, workspace=None, loss=None):
    """mean(w * norm(pred - target, dim=-1)) forward + backward (dhaug_pose_wmpjpe) over (..., 16, 3) poses: returns (loss, grad)
    with pose_mpjpe's conventions.  w: an fp32 device tensor of shape pred.shape[:-2] + (1,) (one weight per pose),
    pred.shape[:-1] (per pose and joint) or (16,) (per joint, shared by all poses and read in place); any sign."""
    name = "pose_wmpjpe"
    y, x, P, grad, loss, ws = _pose_criterion(name, pred, target, poses, meter, workspace, loss)
    mode = wmpjpe_mode(w.shape, pred.shape[:-1])
    if mode is None:
        raise ValueError("%s: w %s must be %s, %s or (16,)" % (name, tuple(w.shape), tuple(pred.shape[:-2]) + (1,),
                                                              tuple(pred.shape[:-1])))
    wd = _dev(w.detach(), torch.float32, name)
    _lib.call("dhaug_pose_wmpjpe", _p(y), _p(x), P, _p(wd), mode, int(poses), _p(grad), _p(loss), _p(meter), _p(ws), _stream())
    return loss, grad


def pose_byjoint_backward(pred, target, cot):
    """the backward of mpjpe_byjoint (dhaug_pose_byjoint_backward) for (rows, ..., 3) joints: cot holds one value per entry of
    pred.shape[1:-1]; returns grad[r, c] = cot[c] (pred - target) / (|pred - target| rows) in pred's shape, 0 at distance 0"""
    name = "pose_byjoint_backward"
    if tuple(pred.shape) != tuple(target.shape):
        raise ValueError("%s: pred %s and target %s differ in shape" % (name, tuple(pred.shape), tuple(target.shape)))
    if pred.dim() < 2 or pred.shape[-1] != 3:
        raise ValueError("%s: joints must be (rows, ..., 3), got %s" % (name, tuple(pred.shape)))
    rows, cols = pred.shape[0], 1
    for d in pred.shape[1:-1]:
        cols *= d
    if cot.numel() != cols:
        raise ValueError("%s: cot %s must hold one value per column (%d)" % (name, tuple(cot.shape), cols))
    y = _dev(pred.detach(), torch.float32, name)
    x = _dev(target.detach(), torch.float32, name)
    c = _dev(cot.detach(), torch.float32, name)
    grad = torch.empty_like(y)
    _lib.call("dhaug_pose_byjoint_backward", _p(y), _p(x), rows, cols, _p(c), _p(grad), _stream())
    return grad


def _flat_f32(t, name, what):
    if t.dim() != 1:
        raise ValueError("%s: %s must be a flat vector, got %s" % (name, what, tuple(t.shape)))
    if not t.is_cuda:
        raise RuntimeError("dhaug op `%s` needs a GPU tensor (no CPU fallback exists)" % name)
    assert t.dtype == torch.float32 and t.is_contiguous(), "%s: %s must be contiguous fp32" % (name, what)
    return t


def grad_sumsq(grad, grad_scale=1.0, workspace=None, step_counter=None):
    """per-workgroup partial sums of (grad * grad_scale)^2 into workspace (dhaug_grad_sumsq); step_counter (int32 device tensor)
    is advanced by one in the same launch.  Returns the workspace (adam_clip_step reads it)."""
    g = _flat_f32(grad, "grad_sumsq", "grad")
    ws = workspace if workspace is not None else posetrain_workspace(g.device)
    assert step_counter is None or step_counter.dtype == torch.int32
    _lib.call("dhaug_grad_sumsq", _p(g), g.numel(), float(grad_scale), _p(ws), _p(step_counter), _stream())
    return ws


def u64_add(cell, value):
    """*cell += value on one element of an int64 device tensor read as uint64 (dhaug_u64_add, one launch in stream order)"""
    if not cell.is_cuda:
        raise RuntimeError("dhaug op `u64_add` needs a GPU tensor (no CPU fallback exists)")
    if cell.dtype != torch.int64 or cell.numel() != 1:
        raise ValueError("u64_add: cell must be one int64 element, got %s %s" % (cell.dtype, tuple(cell.shape)))
    _lib.call("dhaug_u64_add", _p(cell), int(value) & 0xFFFFFFFFFFFFFFFF, _stream())
    return cell


def adam_clip_step(param, grad, exp_avg, exp_avg_sq, step_dev, workspace, max_norm, lr=1e-3, betas=(0.9, 0.999), eps=1e-8,
                   grad_scale=1.0, norm_out=None):
    """clip_grad_norm_(max_norm) + Adam.step() from the partials of grad_sumsq(grad, grad_scale, workspace) (dhaug_adam_clip_step);
    *step_dev is the step count (already advanced).  lr: a number, or a 1-element fp32 device tensor that the launch reads when it
    runs (dhaug_adam_clip_step_lr: a captured launch follows the schedule).  Returns the gradient norm as a 1-element fp32 device
    tensor."""
    n = param.numel()
    vectors = ((param, "param"), (grad, "grad"), (exp_avg, "exp_avg"), (exp_avg_sq, "exp_avg_sq"))
    for t, what in vectors:
        if t.dim() != 1 or t.numel() != n:
            raise ValueError("adam_clip_step: %s must be a flat vector of %d elements, got %s" % (what, n, tuple(t.shape)))
    max_norm = float(max_norm)
    if not max_norm > 0.0:
        raise ValueError("adam_clip_step: max_norm must be > 0, got %r" % max_norm)
    for t, what in vectors:
        _flat_f32(t, "adam_clip_step", what)
    assert step_dev.dtype == torch.int32
    if norm_out is None:
        norm_out = torch.empty(1, dtype=torch.float32, device=param.device)
    if torch.is_tensor(lr):
        if not (lr.is_cuda and lr.dtype == torch.float32 and lr.numel() == 1):
            raise ValueError("adam_clip_step: a tensor lr must be one fp32 device element, got %s %s" % (lr.dtype, tuple(lr.shape)))
        _lib.call("dhaug_adam_clip_step_lr", _p(param), _p(grad), _p(exp_avg), _p(exp_avg_sq), n, _p(lr), betas[0], betas[1], eps,
                  _p(step_dev), float(grad_scale), max_norm, _p(workspace), _p(norm_out), _stream())
        return norm_out
    _lib.call("dhaug_adam_clip_step", _p(param), _p(grad), _p(exp_avg), _p(exp_avg_sq), n, float(lr), betas[0], betas[1], eps,
              _p(step_dev), float(grad_scale), max_norm, _p(workspace), _p(norm_out), _stream())
    return norm_out


# ---------------------------------------------------------------------------------------------- GEMM
def cast_pad_bf16(src, pad_cols=None, out=None):
    """fp32 (rows, cols) -> bf16 (rows, pad_cols), zero-padded; out: write into these rows of a larger buffer"""
    s = _dev(src, torch.float32, "cast_pad_bf16")
    s = s.reshape(-1, s.shape[-1])
    rows, cols = s.shape
    pad_cols = ceil_to(cols, 16) if pad_cols is None else pad_cols
    dst = torch.empty((rows, pad_cols), dtype=BF16, device=s.device) if out is None else out
    assert dst.dtype == BF16 and dst.shape == (rows, pad_cols) and dst.stride(1) == 1
    _lib.call("dhaug_cast_pad_bf16", _p(s), cols, _p(dst), dst.stride(0), rows, cols, pad_cols, _stream())
    return dst


def cast_transpose_bf16(src, pad_cols=None):
    s = _dev(src, torch.float32, "cast_transpose_bf16")
    rows, cols = s.shape
    pad_cols = ceil_to(rows, 16) if pad_cols is None else pad_cols
    dst = torch.empty((cols, pad_cols), dtype=BF16, device=s.device)
    _lib.call("dhaug_cast_transpose_bf16", _p(s), cols, _p(dst), pad_cols, rows, cols, pad_cols, _stream())
    return dst


def split_bf16(src, mode, terms, pad_cols=None):
    """fp32 (rows, cols) -> bf16 (rows, terms*pad): see dhaug_split_bf16 (mode 0 activation side, 1 weight side)."""
    if src.is_cuda and src.dtype == torch.float32 and src.dim() == 2 and src.stride(1) == 1 and src.stride(0) >= src.shape[1]:
        # a column block of a wider buffer is read where it lies (no contiguous copy, no realignment: the kernel's vector
        # path tests the base address and the row pitch itself and falls back to element loads)
        s, ld = src, src.stride(0)
    else:
        s = _dev(src, torch.float32, "split_bf16")
        s = s.reshape(-1, s.shape[-1])
        ld = s.shape[1]
    rows, cols = s.shape
    pad_cols = ceil_to(cols, 16) if pad_cols is None else pad_cols
    dst = torch.empty((rows, (3 if mode == 2 else terms) * pad_cols), dtype=BF16, device=s.device)
    _lib.call("dhaug_split_bf16", _p(s), ld, _p(dst), rows, cols, pad_cols, mode, terms, _stream())
    return dst


def gemm_planes_ok(N, kp, bias=None, res_f32=None, dmask_f32=None, out=None, six=False):
    """shapes dhaug_gemm_bf16x6_planes takes (the ping-pong tiles; a power-of-two piece width, or -- six: the ordinary six-segment operand,
    x_order 2 -- any width with 6 kp >= 128)"""
    al = lambda t: t is None or (t.data_ptr() % 16 == 0)
    row = lambda t: t is None or (t.stride(1) == 1 and t.stride(0) % 4 == 0)
    wide = (6 * kp >= 128 and kp % 8 == 0) if six else (kp >= 64 and (kp & (kp - 1)) == 0)
    return (N % 8 == 0 and wide and al(bias) and al(res_f32) and al(dmask_f32) and al(out) and row(res_f32) and row(dmask_f32) and row(out))


def gemm_nt_planes(A3, B6, N, kp, bias=None, res_f32=None, act=0, slope=0.0, dmask_f32=None, dmask_act=0, dmask_slope=0.0, out=None, x_order=0,
                   planes_out=False):
    """fp32 (M, N) = act(x W^T + bias + res_f32), masked by dmask_f32, in the bf16x6 arithmetic with the activation side as planes:
    A3 = split_bf16(x, 2, 6, kp) = [hi|mid|lo], B6 = split_bf16(W, 1, 6, kp) (dhaug_gemm_bf16x6_planes: bit-identical to gemm_nt on the
    mode 0 split); x_order 1: the planes stand for the mode 1 operand, B6 = split_bf16(W, 0, 6, kp)."""
    assert A3.dtype == BF16 and B6.dtype == BF16 and A3.is_cuda and B6.is_cuda and A3.stride(1) == 1 and B6.stride(1) == 1
    M = A3.shape[0]
    if out is None:
        out = torch.empty((M, N), dtype=torch.float32, device=A3.device)
    assert out.dtype == torch.float32 and out.stride(1) == 1 and out.shape[0] == M
    if bias is not None:
        bias = _dev(bias, torch.float32, "gemm_nt_planes")
    # planes_out: the result once more as split_bf16(out, 2, 6, N) would make it (N a multiple of 8), written by the GEMM's epilogue
    cp = torch.empty((M, 3 * N), dtype=BF16, device=A3.device) if planes_out else None
    _lib.call("dhaug_gemm_bf16x6_planes", _p(A3), A3.stride(0), _p(B6), B6.stride(0), _p(bias), _p(res_f32),
              0 if res_f32 is None else res_f32.stride(0), _p(dmask_f32), 0 if dmask_f32 is None else dmask_f32.stride(0), int(dmask_act),
              float(dmask_slope), _p(out), out.stride(0), _p(cp), 0 if cp is None else cp.stride(0), M, N, kp, int(x_order), act, float(slope),
              _stream())
    return (out, cp) if planes_out else out


def split_f16(src, mode, pad_cols=None):
    """fp32 (rows, cols) -> (rows, 3 * pad_cols) IEEE-half pieces of x = hi + lo: mode 0 [hi|hi|lo] (activation side), mode 1 [hi|lo|hi]
    (weight side) -- the operands of gemm_nt_f16x3.  |x| < 65 504."""
    s = _dev(src, torch.float32, "split_f16") if src.is_contiguous() or not (src.dim() == 2 and src.stride(1) == 1) else src
    assert s.dtype == torch.float32 and s.is_cuda and s.dim() == 2 and s.stride(1) == 1
    rows, cols = s.shape
    pad_cols = ceil_to(cols, 16) if pad_cols is None else pad_cols
    dst = torch.empty((rows, (2 if mode == 2 else 3) * pad_cols), dtype=torch.float16, device=s.device)
    _lib.call("dhaug_split_f16", _p(s), s.stride(0), _p(dst), rows, cols, pad_cols, mode, _stream())
    return dst


def gemm_nt_f16x3_planes(A, B, N, kp, a_planes, bias=None, res_f32=None, act=0, slope=0.0, planes_kp=0, out=None):
    """gemm_nt_f16x3 with the split left out of a chain of layers (dhaug_gemm_f16x3_planes): A = split_f16(x, 2, kp) = [hi|lo] (a_planes;
    kp = 64 * 2^j) or the mode 0 operand; B = split_f16(W, 1, kp); planes_kp > 0: returns (out, planes) with planes = split_f16(out, 2,
    planes_kp) written by the GEMM's epilogue."""
    assert A.dtype == torch.float16 and B.dtype == torch.float16 and A.is_cuda and B.is_cuda and A.stride(1) == 1
    M = A.shape[0]
    if out is None:
        out = torch.empty((M, N), dtype=torch.float32, device=A.device)
    assert out.dtype == torch.float32 and out.shape == (M, N) and out.stride(1) == 1      # (may be a column block of a wider buffer)
    cp = torch.empty((M, 2 * planes_kp), dtype=torch.float16, device=A.device) if planes_kp else None
    if bias is not None:
        bias = _dev(bias, torch.float32, "gemm_nt_f16x3_planes")
    _lib.call("dhaug_gemm_f16x3_planes", _p(A), A.stride(0), int(bool(a_planes)), _p(B), B.stride(0), _p(bias), _p(res_f32),
              0 if res_f32 is None else res_f32.stride(0), _p(out), out.stride(0), _p(cp), 0 if cp is None else cp.stride(0), int(planes_kp), M, N, kp,
              act, float(slope), _stream())
    return (out, cp) if planes_kp else out


def gemm_f16x3_ok(N, K3, bias=None, res_f32=None):
    """shapes dhaug_gemm_f16x3 takes (the ping-pong tiles: csrc/dhaug_gemm_p8.hip)"""
    al = lambda t: t is None or (t.data_ptr() % 16 == 0)
    return (N % 8 == 0 and K3 >= 128 and K3 % 16 == 0 and al(bias) and al(res_f32)
            and (res_f32 is None or (res_f32.stride(1) == 1 and res_f32.stride(0) % 4 == 0)))


def gemm_nt_f16x3(A, B, N, K3, bias=None, res_f32=None, act=0, slope=0.0, out=None):
    """fp32 (M, N) = act(A B^T + bias + res_f32) on IEEE-half operands: A = split_f16(x, 0), B = split_f16(W, 1), K3 = 3 * padded width
    (dhaug_gemm_f16x3: the "f16x3" arithmetic as a layer GEMM)."""
    assert A.dtype == torch.float16 and B.dtype == torch.float16 and A.is_cuda and B.is_cuda
    M = A.shape[0]
    if out is None:
        out = torch.empty((M, N), dtype=torch.float32, device=A.device)
    assert out.dtype == torch.float32 and out.stride(1) == 1 and out.shape[0] == M
    if bias is not None:
        bias = _dev(bias, torch.float32, "gemm_nt_f16x3")
    _lib.call("dhaug_gemm_f16x3", _p(A), A.stride(0), _p(B), B.stride(0), _p(bias), _p(res_f32), 0 if res_f32 is None else res_f32.stride(0),
              _p(out), out.stride(0), M, N, K3, act, float(slope), _stream())
    return out


def gemm_nt(A, B, N, K, bias=None, res_bf16=None, res_f32=None, act=0, slope=0.0, out_bf16=False, n_pad=0,
            out_f32=False, lda=None, ldb=None, c_bf16=None, c_f32=None):
    """C[M,N] = act(A[M,K] B[N,K]^T + bias + residual).  A, B bf16 (row strides lda/ldb default to their widths).
    Returns (c_bf16 (M, max(n_pad, ceil8(N))) | None, c_f32 (M,N) | None).  c_bf16 / c_f32: write into these (row-strided
    views allowed: a column block of a wider buffer) instead of allocating; columns [N, n_pad) of c_bf16 are zeroed."""
    assert A.dtype == BF16 and B.dtype == BF16 and A.is_cuda and B.is_cuda
    M = A.shape[0]
    lda = A.stride(0) if lda is None else lda
    ldb = B.stride(0) if ldb is None else ldb
    cb, cf = c_bf16, c_f32
    ldcb = 0
    if cb is not None:
        assert cb.dtype == BF16 and cb.stride(1) == 1 and cb.shape[0] == M
        ldcb, n_pad = cb.stride(0), min(max(n_pad, N), cb.shape[1])       # never past the view's own columns
    elif out_bf16:
        ldcb = max(n_pad, ceil_to(N, 8))
        cb = torch.empty((M, ldcb), dtype=BF16, device=A.device)
        n_pad = ldcb
    if cf is not None:
        assert cf.dtype == torch.float32 and cf.stride(1) == 1 and cf.shape[0] == M
    elif out_f32:
        cf = torch.empty((M, N), dtype=torch.float32, device=A.device)
    if bias is not None:
        bias = _dev(bias, torch.float32, "gemm_nt")
    _lib.call("dhaug_gemm_bf16", _p(A), lda, _p(B), ldb, _p(bias), _p(res_bf16),
              0 if res_bf16 is None else res_bf16.stride(0), _p(res_f32), 0 if res_f32 is None else res_f32.stride(0),
              _p(cb), ldcb, n_pad, _p(cf), N if cf is None else cf.stride(0), M, N, K, act, float(slope), _stream())
    return cb, cf


def gemm_nt_dmask(A, B, N, K, dmask, dmask_act, dmask_slope=0.0, res_bf16=None, out=None):
    """(A[M,K] B[N,K]^T + res) * act'(dmask): input gradient of a layer + activation backward of its producer in one launch;
    bf16 (M, ceil16 N) with zero pad columns, or `out` (a row-strided view: no columns beyond its own are touched)."""
    assert A.dtype == BF16 and B.dtype == BF16 and dmask.dtype == BF16
    M = A.shape[0]
    if out is None:
        out = torch.empty((M, ceil_to(N, 16)), dtype=BF16, device=A.device)
    assert out.dtype == BF16 and out.stride(1) == 1 and out.shape[0] == M and out.shape[1] >= N
    cols = getattr(dmask, "_dhaug_bits_cols", None)
    if (cols is not None and N == 256 * len(cols) and len(cols) <= 2 and K in (16, 32, 48, 64, 112, 128, 256) and res_bf16 is None
            and dmask_act != 0 and M > 0 and A.stride(0) % 8 == 0 and out.stride(0) % 8 == 0):
        # a wide output whose 256-column blocks carry their own sign bits (the cotangent of the 3D critic's concatenation)
        assert all(c.device == A.device for c in cols), "sign bits must live on the operands' device"
        _lib.call("dhaug_gemm_bf16_dbits_wide", _p(A), A.stride(0), _p(B), B.stride(0), _p(cols[0]), _p(cols[1]) if len(cols) > 1 else 0,
                  dmask_act, float(dmask_slope), _p(out), out.stride(0), M, N, K, _stream())
        return out
    bits = getattr(dmask, "_dhaug_bits", None)
    assert bits is None or bits.device == A.device, "sign bits must live on the operands' device"
    if (bits is not None and N == 256 and K in (16, 32, 48, 64, 112, 128) and res_bf16 is None and dmask_act != 0
            and M > 0 and M % 32 == 0 and A.stride(0) % 8 == 0 and out.stride(0) % 8 == 0):
        # a 256-wide layer behind a NARROW one (the tangent through a branch's first layer): the same mask bits, K < 256
        _lib.call("dhaug_gemm_bf16_dbits_wide", _p(A), A.stride(0), _p(B), B.stride(0), _p(bits), 0, dmask_act, float(dmask_slope),
                  _p(out), out.stride(0), M, N, K, _stream())
        return out
    if (bits is not None and N == 256 and K == 256 and M % 32 == 0 and M > 0 and dmask_act != 0
            and A.stride(0) % 8 == 0 and out.stride(0) % 8 == 0):
        # the mask as the sign-bit array its forward-with-save layer left beside the image: 32 bytes per row instead of 512
        _lib.call("dhaug_gemm_bf16_dbits", _p(A), A.stride(0), _p(B), B.stride(0), _p(res_bf16),
                  0 if res_bf16 is None else res_bf16.stride(0), _p(bits), dmask_act, float(dmask_slope), _p(out), out.stride(0), M,
                  _stream())
        return out
    _lib.call("dhaug_gemm_bf16_dmask_pad", _p(A), A.stride(0), _p(B), B.stride(0), _p(res_bf16),
              0 if res_bf16 is None else res_bf16.stride(0), _p(dmask), dmask.stride(0), dmask_act, float(dmask_slope),
              _p(out), out.stride(0), min(out.shape[1], ceil_to(N, 16)), M, N, K, _stream())
    return out


NT_GROUP_MAX = 8
# the top of a branch critic (merge layer, merge block, logit layer) as one launch per sweep (dhaug_critic_top_*): DHAUG_NO_TOP_FUSED=1
# runs the separate launches
TOP_FUSED = os.environ.get("DHAUG_NO_TOP_FUSED") is None


def gemm_nt_group(members):
    """Up to NT_GROUP_MAX independent GEMMs of one shape as ONE launch (dhaug_gemm_bf16_group).  members: dicts with A, B (bf16
    operands), N, K and optionally bias, res_bf16, act, slope, dmask, dmask_act, dmask_slope, out (bf16 (M, >= N) view), n_pad.
    Each computes act(A B^T + bias + res) * dmask_act'(dmask) like gemm_nt / gemm_nt_dmask; returns the outputs."""
    assert 1 <= len(members) <= NT_GROUP_MAX
    arr = (_lib.GemmDesc * len(members))()
    outs, keep = [], []
    for d, m in zip(arr, members):
        A, B, N, K = m["A"], m["B"], m["N"], m["K"]
        assert A.dtype == BF16 and B.dtype == BF16
        M = A.shape[0]
        out = m.get("out")
        n_pad = m.get("n_pad", ceil_to(N, 16))
        if out is None:
            out = torch.empty((M, max(n_pad, ceil_to(N, 8))), dtype=BF16, device=A.device)
        assert out.dtype == BF16 and out.stride(1) == 1 and out.shape[0] == M
        n_pad = min(max(n_pad, N), out.shape[1])
        res, dm, bias = m.get("res_bf16"), m.get("dmask"), m.get("bias")
        d.A, d.lda, d.B, d.ldb = _p(A), A.stride(0), _p(B), B.stride(0)
        d.bias = _p(bias)
        d.residual, d.ld_res = _p(res), 0 if res is None else res.stride(0)
        d.residual_f32, d.ld_res_f32 = None, 0
        d.c_bf16, d.ldc_bf16, d.n_pad_zero = _p(out), out.stride(0), n_pad
        d.c_f32, d.ldc_f32 = None, 0
        d.M, d.N, d.K = M, N, K
        d.act, d.slope = int(m.get("act", 0)), float(m.get("slope", 0.0))
        d.dmask, d.ld_dmask = _p(dm), 0 if dm is None else dm.stride(0)
        d.dmask_act, d.dmask_slope = int(m.get("dmask_act", 0)) if dm is not None else 0, float(m.get("dmask_slope", 0.0))
        outs.append(out)
        keep.append((A, B, res, dm, bias))
    _lib.call("dhaug_gemm_bf16_group", arr, len(members), _stream())
    return outs


def gemm_nt_dmask_f32(A, B, N, K, dmask, dmask_act, dmask_slope=0.0, res_f32=None, out=None):
    """(A[M,K] B[N,K]^T + res) * act'(dmask) in the split-operand arithmetic: fp32 result / residual / mask (M, N), A and B the
    operands split_bf16 makes (K = terms * padded width)."""
    assert A.dtype == BF16 and B.dtype == BF16 and dmask.dtype == torch.float32 and dmask.stride(1) == 1
    M = A.shape[0]
    if out is None:
        out = torch.empty((M, N), dtype=torch.float32, device=A.device)
    assert out.dtype == torch.float32 and out.stride(1) == 1 and out.shape[0] == M and out.shape[1] >= N
    assert res_f32 is None or (res_f32.dtype == torch.float32 and res_f32.stride(1) == 1)
    _lib.call("dhaug_gemm_bf16_dmask_f32", _p(A), A.stride(0), _p(B), B.stride(0), _p(res_f32), 0 if res_f32 is None else res_f32.stride(0),
              _p(dmask), dmask.stride(0), dmask_act, float(dmask_slope), _p(out), out.stride(0), M, N, K, _stream())
    return out


BLOCK2 = os.environ.get("DHAUG_NO_BLOCK2") is None        # the two layers of a residual block's backward / tangent step in one launch


def block2_ok(x, mask1, mask2, M):
    """can dhaug_gemm_block2_bf16 take this pair of 256 -> 256 layers?  (bf16 rows, whole 32-row tiles, both masks as sign bits)"""
    return (BLOCK2 and M > 0 and M % 32 == 0 and x.dtype == BF16 and x.shape[1] >= 256 and x.stride(0) % 8 == 0
            and getattr(mask1, "_dhaug_bits", None) is not None and getattr(mask2, "_dhaug_bits", None) is not None)


def gemm_block2(x, B1, B2, mask1, mask2, act, slope=0.0, out1=None, out2=None):
    """y1 = (x B1^T) * act'(mask1); y2 = (y1 B2^T + x) * act'(mask2) -- x, y1, y2 bf16 (M, >= 256); B1, B2 bf16 (256, >= 256);
    the masks by their sign-bit arrays.  Returns (y1, y2)."""
    M = x.shape[0]
    if out1 is None:
        out1 = torch.empty((M, 256), dtype=BF16, device=x.device)
    if out2 is None:
        out2 = torch.empty((M, 256), dtype=BF16, device=x.device)
    assert out1.dtype == BF16 and out2.dtype == BF16 and out1.shape[0] == M and out2.shape[0] == M
    assert mask1._dhaug_bits.device == x.device and mask2._dhaug_bits.device == x.device, "sign bits must live on the operands' device"
    _lib.call("dhaug_gemm_block2_bf16", _p(x), x.stride(0), _p(B1), B1.stride(0), _p(B2), B2.stride(0), _p(mask1._dhaug_bits),
              _p(mask2._dhaug_bits), act, float(slope), _p(out1), out1.stride(0), _p(out2), out2.stride(0), M, _stream())
    return out1, out2


def gemm_block2_stack(x, blocks, act, slope=0.0):
    """a chain of gemm_block2 steps in one launch: blocks = [(B1, B2, mask1, mask2, out1 | None, out2 | None)], block i + 1 takes
    block i's y2 as its x.  Returns [(y1, y2)]."""
    M = x.shape[0]
    assert 1 <= len(blocks) <= _lib.BLOCK2_MAX and x.dtype == BF16
    arr = (_lib.Block2 * len(blocks))()
    outs = []
    for d, (B1, B2, mask1, mask2, out1, out2) in zip(arr, blocks):
        if out1 is None:
            out1 = torch.empty((M, 256), dtype=BF16, device=x.device)
        if out2 is None:
            out2 = torch.empty((M, 256), dtype=BF16, device=x.device)
        assert out1.dtype == BF16 and out2.dtype == BF16 and out1.shape[0] == M and out2.shape[0] == M
        assert mask1._dhaug_bits.device == x.device and mask2._dhaug_bits.device == x.device, "sign bits must live on the operands' device"
        d.W1, d.ldw1, d.W2, d.ldw2 = _p(B1), B1.stride(0), _p(B2), B2.stride(0)
        d.bits1, d.bits2 = _p(mask1._dhaug_bits), _p(mask2._dhaug_bits)
        d.Y1, d.ldy1, d.Y2, d.ldy2 = _p(out1), out1.stride(0), _p(out2), out2.stride(0)
        outs.append((out1, out2))
    _lib.call("dhaug_gemm_block2_stack_bf16", _p(x), x.stride(0), arr, len(blocks), act, float(slope), M, _stream())
    return outs


def tail_rows(t, r0):
    """t[r0:], keeping the sign-bit array of a saved activation attached (rows r0.. start at a 32-row tile)"""
    v = t[r0:]
    bits = getattr(t, "_dhaug_bits", None)
    if bits is not None and r0 % 32 == 0:
        v._dhaug_bits = bits[(r0 // 32) * 256:]
    return v


TN256 = os.environ.get("DHAUG_NO_TN256") is None
_TN_WS = {}


def _tn_group_workspace(dev):
    """DHAUG_TN_GROUP_WORKSPACE_FLOATS fp32 values per device: the per-workgroup partial results of dhaug_gemm_tn_group_bf16
    (any content; calls are ordered on the stream)"""
    if torch.cuda.is_current_stream_capturing():
        # inside a hipGraph capture the buffer must belong to THAT graph's pool (a cached one would be memory of whichever
        # capture came first, gone with it): the pool hands the same block out again after each use
        return torch.empty(_lib.TN_GROUP_WORKSPACE_FLOATS, dtype=torch.float32, device=dev)
    k = (dev.type, dev.index, torch.cuda.current_stream().cuda_stream)      # (per stream: concurrent critic steps)
    if k not in _TN_WS:
        _TN_WS[k] = torch.empty(_lib.TN_GROUP_WORKSPACE_FLOATS, dtype=torch.float32, device=dev)
    return _TN_WS[k]


class workgroup_cap:
    """with workgroup_cap(n): the persistent launches issued inside take at most n workgroups (dhaug_set_workgroup_cap)"""

    def __init__(self, n):
        self.n = int(n)

    def __enter__(self):
        self.old = _lib.lib().dhaug_set_workgroup_cap(self.n) if self.n else None
        return self

    def __exit__(self, *exc):
        if self.old is not None:
            _lib.lib().dhaug_set_workgroup_cap(self.old)


class nan_propagation:
    """with nan_propagation(True): the fused INFERENCE programs launched inside apply ReLU as max(v, v * 0) -- a NaN / inf input
    row reaches its logit, NaN weights reach every logit, as in the reference (dhaug_set_nan_propagation; process-wide default:
    DHAUG_NAN_PROPAGATION=1 in the environment).  The training iterations (gan_iteration, video_gan_iteration) always run inside it.
    The flag is a process-wide value read when a kernel is LAUNCHED: a hipGraph keeps the setting it was CAPTURED with, so wrapping
    the replay of an already captured graph changes nothing -- wrap the capture (or the function that is captured)."""

    def __init__(self, on=True):
        self.on = int(bool(on))

    def __enter__(self):
        self.old = _lib.lib().dhaug_set_nan_propagation(self.on)
        return self

    def __exit__(self, *exc):
        _lib.lib().dhaug_set_nan_propagation(self.old)


def tn_group_ok(M, N1, N2, colsum_rows):
    """shapes dhaug_gemm_tn_group_bf16 takes (and where it pays: a long batch)"""
    return M >= 1024 and M % 32 == 0 and colsum_rows % 32 == 0 and 1 <= N1 <= 256 and 1 <= N2 <= 256


TN_WIDE_MIN_BLOCKS = int(os.environ.get("DHAUG_TN_WIDE_MIN_BLOCKS", "128"))


# one weight gradient of gemm_tn_group: out[N1,N2] (+)= A[M,N1]^T B[M,N2], colsum[N1] (+)= column sums of A over rows [0, colsum_rows);
# M, lda, ldb default to A's rows and the operands' row pitches; planes_a / planes_b: A / B as the three planes of a split operand (dhaug_tn_layer)
TnItem = collections.namedtuple("TnItem", "A B N1 N2 out colsum colsum_rows accumulate M lda ldb planes_a planes_b",
                                defaults=(None, 0, True, None, None, None, 0, 0))


def gemm_tn_group(items, max_workgroups=0):
    """items: TnItems (or plain tuples of their leading fields) -- the weight gradients C_i (+)= A_i^T B_i of several layers in
    one launch (+ one that sums the partial results).
    max_workgroups: leave CUs to kernels running beside this launch (0: one workgroup per CU)."""
    # layers wider than 256: whole ("wide": one workgroup per 256 x 256 block, which adds into the gradient slot itself) where the
    # chunk they travel in has blocks enough to fill the card without splitting any over the batch; as 256 x 256 blocks, each an
    # item of its own, otherwise (a long batch of few wide layers: the blocks are split over the batch and summed)
    nblk = lambda it: ((it.N1 + 255) // 256) * ((it.N2 + 255) // 256)
    items = [it if type(it) is TnItem else TnItem(*it) for it in items]
    if any(nblk(it) > 1 for it in items):
        flat = []
        for i0 in range(0, len(items), _lib.TN_GROUP_MAX):
            chunk = items[i0:i0 + _lib.TN_GROUP_MAX]
            if sum(nblk(it) for it in chunk) >= TN_WIDE_MIN_BLOCKS:
                flat.extend(chunk)
                continue
            for it in chunk:
                assert (it.planes_a == 0 and it.planes_b == 0) or (it.N1 <= 256 and it.N2 <= 256), "a wide layer's operands as planes: not built"
                for n0 in range(0, it.N1, 256):
                    for k0 in range(0, it.N2, 256):
                        c = it.colsum[n0:] if (it.colsum is not None and k0 == 0) else None
                        flat.append(it._replace(A=it.A[:, n0:], B=it.B[:, k0:], N1=min(256, it.N1 - n0), N2=min(256, it.N2 - k0),
                                                out=it.out[n0:, k0:], colsum=c, colsum_rows=it.colsum_rows if c is not None else 0,
                                                M=it.A.shape[0] if it.M is None else it.M))
        items = flat
    # the items of ONE launch are summed into their outputs concurrently (a block that is left with one workgroup adds its
    # result into C / colsum with a plain read-modify-write): two items with the same output must not share a launch
    # (include/dhaug.h, dhaug_gemm_tn_group_bf16).  A later contribution to an output waits for a launch of its own.
    seen, first, later = set(), [], []
    for it in items:
        keys = {("C", _p(it.out))} | ({("s", _p(it.colsum))} if it.colsum is not None else set())
        if keys & seen:
            later.append(it)
        else:
            seen |= keys
            first.append(it)
    if later:
        gemm_tn_group(first, max_workgroups)
        gemm_tn_group(later, max_workgroups)
        return
    for i0 in range(0, len(items), _lib.TN_GROUP_MAX):
        chunk = items[i0:i0 + _lib.TN_GROUP_MAX]
        arr = (_lib.TnLayer * len(chunk))()
        for d, it in zip(arr, chunk):
            A, B, out = it.A, it.B, it.out
            assert A.dtype == BF16 and B.dtype == BF16 and out.dtype == torch.float32
            d.planes_a, d.planes_b = int(it.planes_a), int(it.planes_b)
            d.A, d.lda, d.B, d.ldb = _p(A), A.stride(0) if it.lda is None else it.lda, _p(B), B.stride(0) if it.ldb is None else it.ldb
            d.C, d.ldc, d.colsum_a, d.colsum_rows = _p(out), out.stride(0), _p(it.colsum), it.colsum_rows
            d.M, d.N1, d.N2, d.accumulate = A.shape[0] if it.M is None else it.M, it.N1, it.N2, int(bool(it.accumulate))
            d.max_workgroups = int(max_workgroups)
        _lib.call("dhaug_gemm_tn_group_bf16", arr, len(chunk), _p(_tn_group_workspace(chunk[0].A.device)), _stream())


# Set while the posenet step is captured (function_aug.model_pos_train.StepRunner): gemm_tn and colsum then zero a fresh output with a
# fill KERNEL and call the library in its accumulating form, instead of letting it issue hipMemset2DAsync / hipMemsetAsync.  Measured
# on an MI355X: the memset nodes of the most recently captured step stopped zeroing once the allocator had released cached memory
# (torch.cuda.empty_cache, which every later capture calls) -- the replayed weight gradient then came out as 1e23 .. 1e30, while the
# same step with kernel nodes only replays the eager path's bits.  The sums are the same either way (zero, then atomic adds).
ZERO_BY_KERNEL = False


def gemm_tn(A, B, N1, N2, out=None, accumulate=False, M=None, lda=None, ldb=None, colsum=None, colsum_rows=None):
    """C[N1,N2] (+)= A[M,N1]^T B[M,N2], bf16 operands, fp32 result; colsum (fp32 [N1], optional) (+)= column sums of A
    (over rows [0, colsum_rows) only when given: a multiple of 128)."""
    assert A.dtype == BF16 and B.dtype == BF16
    M = A.shape[0] if M is None else M
    if out is None:
        out = torch.empty((N1, N2), dtype=torch.float32, device=A.device)
        accumulate = False
    la, lb = A.stride(0) if lda is None else lda, B.stride(0) if ldb is None else ldb
    cr = M if colsum_rows is None else colsum_rows
    if TN256 and N1 == 256 and N2 == 256 and tn_group_ok(M, N1, N2, cr):
        # a long 256 x 256 contraction alone: a group of one (whole-output tiles, dhaug_tn256.hip)
        gemm_tn_group([TnItem(A=A, B=B, N1=N1, N2=N2, out=out, colsum=colsum, colsum_rows=cr, accumulate=accumulate, M=M, lda=la, ldb=lb)])
        return out
    if ZERO_BY_KERNEL and not accumulate:
        out.zero_()
        if colsum is not None:
            colsum.zero_()
        accumulate = True
    _lib.call("dhaug_gemm_tn_bf16_rows", _p(A), la, _p(B), lb, _p(out), out.stride(0), _p(colsum), cr, M, N1, N2, int(accumulate), _stream())
    return out


def colsum(src, N=None, out=None, accumulate=False):
    N = src.shape[1] if N is None else N
    if out is None:
        out = torch.empty((N,), dtype=torch.float32, device=src.device)
        accumulate = False
    name = "dhaug_colsum_bf16" if src.dtype == BF16 else "dhaug_colsum_f32"
    if ZERO_BY_KERNEL and not accumulate:
        out.zero_()
        accumulate = True
    _lib.call(name, _p(src), src.stride(0), _p(out), src.shape[0], N, int(accumulate), _stream())
    return out


def act_backward(g, y, act, slope=0.0, out=None):
    """g * act'(y), same dtype/shape as g (bf16: widths multiple of 8, row-strided views allowed; fp32: contiguous).
    out: write there (may be g itself)."""
    assert g.dtype == y.dtype and g.shape == y.shape
    if out is None:
        out = torch.empty_like(g) if g.is_contiguous() else torch.empty(g.shape, dtype=g.dtype, device=g.device)
    if g.dtype == BF16:
        _lib.call("dhaug_act_backward_bf16", _p(g), g.stride(0), _p(y), y.stride(0), _p(out), out.stride(0), g.shape[0],
                  g.shape[1], act, float(slope), _stream())
    else:
        assert g.is_contiguous() and y.is_contiguous() and out.is_contiguous()
        _lib.call("dhaug_act_backward_f32", _p(g), _p(y), _p(out), g.numel(), act, float(slope), _stream())
    return out


def adam_step(param, grad, exp_avg, exp_avg_sq, step, lr=1e-4, betas=(0.5, 0.9), eps=1e-8, grad_scale=1.0):
    n = param.numel()
    assert param.is_contiguous() and grad.is_contiguous() and grad.numel() == n
    _lib.call("dhaug_adam_step", _p(param), _p(grad), _p(exp_avg), _p(exp_avg_sq), n, lr, betas[0], betas[1], eps,
              int(step), float(grad_scale), _stream())


def adam_step_dev(param, grad, exp_avg, exp_avg_sq, step_dev, lr=1e-4, betas=(0.5, 0.9), eps=1e-8, grad_scale=1.0):
    """Adam step whose count lives on the device (int32 tensor, advanced here): replayable inside a captured graph"""
    n = param.numel()
    assert param.is_contiguous() and grad.is_contiguous() and grad.numel() == n and step_dev.dtype == torch.int32
    _lib.call("dhaug_counter_add", _p(step_dev), 1, _stream())
    _lib.call("dhaug_adam_step_dev", _p(param), _p(grad), _p(exp_avg), _p(exp_avg_sq), n, lr, betas[0], betas[1], eps,
              _p(step_dev), float(grad_scale), _stream())


# --------------------------------------------------------------------------------------- WGAN-GP arithmetic
def gp_assemble(real, fake, alpha, out=None, bf16_rows=False):
    """(3B, W) fp32 = [real; fake; alpha * real + (1 - alpha) * fake].  bf16_rows (W a multiple of 16): the real / fake rows also as
    bf16 (2B, W), attached as out._dhaug_bf16_rows -- what cast_pad_bf16(out[:2B], W) would make, from the same launch"""
    r = _dev(real, torch.float32, "gp_assemble")
    r = r.reshape(r.shape[0], -1)
    f = _dev(fake, torch.float32, "gp_assemble").reshape(r.shape)
    a = _dev(alpha, torch.float32, "gp_assemble").reshape(-1)
    B, W = r.shape
    assert a.shape[0] == B
    if out is None:
        out = torch.empty((3 * B, W), dtype=torch.float32, device=r.device)
    if bf16_rows and W % 16 == 0:
        xb = torch.empty((2 * B, W), dtype=BF16, device=r.device)
        _lib.call("dhaug_gp_assemble_bf16", _p(r), _p(f), _p(a), _p(out), _p(xb), W, B, W, _stream())
        out._dhaug_bf16_rows = xb
        return out
    _lib.call("dhaug_gp_assemble", _p(r), _p(f), _p(a), _p(out), B, W, _stream())
    return out


def gp_penalty(grad, coef, bf16=False):
    """per-row (||g|| - 1)^2 and the penalty's cotangent coef * (n - 1) / n * g.  bf16 (W a multiple of 16): v also as bf16,
    attached as v._dhaug_bf16 (= cast_pad_bf16(v, W), from the same launch)"""
    g = _dev(grad, torch.float32, "gp_penalty")
    B, W = g.shape
    v = torch.empty_like(g)
    pen = torch.empty((B,), dtype=torch.float32, device=g.device)
    if bf16 and W % 16 == 0:
        vb = torch.empty((B, W), dtype=BF16, device=g.device)
        _lib.call("dhaug_gp_penalty_bf16", _p(g), _p(v), _p(vb), W, _p(pen), B, W, float(coef), _stream())
        v._dhaug_bf16 = vb
        return v, pen
    _lib.call("dhaug_gp_penalty", _p(g), _p(v), _p(pen), B, W, float(coef), _stream())
    return v, pen


def d3_penalty(pose16, grad_kcs, grad_pose, coef):
    """The 3D critic's penalty step in one launch (dhaug_d3_penalty): from the x_hat poses (N, 48) fp32 and the two branches' input
    cotangents (N, 30) / (N, 48) fp32 -> (tangent input of the KCS branch (N, 32) bf16, of the pose branch (N, 48) bf16, pen (N) fp32)
    = kcs_backward + add_f32 + gp_penalty + kcs_jvp + the two bf16 casts (same operations, same order)."""
    x = _dev(pose16, torch.float32, "d3_penalty").reshape(-1, 48)
    N = x.shape[0]
    gk = _dev(grad_kcs, torch.float32, "d3_penalty").reshape(N, 30)
    gp = _dev(grad_pose, torch.float32, "d3_penalty").reshape(N, 48)
    tk = torch.empty((N, 32), dtype=BF16, device=x.device)
    tv = torch.empty((N, 48), dtype=BF16, device=x.device)
    pen = torch.empty((N,), dtype=torch.float32, device=x.device)
    _lib.call("dhaug_d3_penalty", _p(x), _p(gk), _p(gp), float(coef), _p(tk), _p(tv), _p(pen), N, _stream())
    return tk, tv, pen


CRITIC_SCALARS_SCRATCH = 192      # floats: DHAUG_CRITIC_SCALARS_SCRATCH of include/dhaug.h (tests/test_cpu_boundary.py compares)


def critic_scalars(logits, pen, B, lam):
    """(5,) fp32: D_real, D_fake, GP, Wasserstein_D, D_cost (logit means over B rows per half, penalty mean over len(pen))"""
    # result (5 floats, padded to 8 so that the scratch stays 32-byte aligned) + the partial sums of stage 1
    buf = torch.empty((8 + CRITIC_SCALARS_SCRATCH,), dtype=torch.float32, device=logits.device)
    scratch = buf[8:]
    assert scratch.numel() >= CRITIC_SCALARS_SCRATCH
    _lib.call("dhaug_critic_scalars", _p(logits), logits.stride(0), _p(pen), B, pen.numel(), float(lam), _p(buf), _p(scratch), _stream())
    return buf[:5]


def rank1_mask(seed, w_col, mask, n, act, slope=0.0, out=None):
    """bf16 (M, pad): bf16(seed[r] * w[c]) * act'(mask[r][c]) -- the first backward step through a 1-wide logit layer.
    seed (M, >=1) bf16 (column 0), w_col: bf16 view with the layer's n weights along dim 0 (any stride); mask (M, >= ceil16 n):
    the kernel writes as many columns as it reads mask columns, and every one of the result's ceil16 n columns is an operand
    column of the K-padded GEMM behind it"""
    assert seed.dtype == BF16 and w_col.dtype == BF16 and mask.dtype == BF16
    M, pad = mask.shape[0], ceil_to(n, 16)
    assert mask.shape[1] >= pad, "rank1_mask: the mask has %d columns, the result %d" % (mask.shape[1], pad)
    if out is None:
        out = torch.empty((M, pad), dtype=BF16, device=mask.device)
    bits = getattr(mask, "_dhaug_bits", None)
    if bits is not None and n == 256 and act != 0 and out.stride(0) % 8 == 0 and out.shape[1] >= 256:
        assert bits.device == out.device, "sign bits must live on the operands' device"
        _lib.call("dhaug_rank1_bits_bf16", _p(seed), seed.stride(0), _p(w_col), w_col.stride(0), _p(bits), _p(out), out.stride(0), M,
                  act, float(slope), _stream())
        return out
    _lib.call("dhaug_rank1_mask_bf16", _p(seed), seed.stride(0), _p(w_col), w_col.stride(0), _p(mask), mask.stride(0), _p(out),
              out.stride(0), M, n, pad, act, float(slope), _stream())
    return out


def top_backward_ok(M, n0, nc, masks, bits_cols):
    """dhaug_critic_top_backward_bf16 covers: whole 64-row tiles, a merge block of at most 112 features behind a concatenation of two
    256-wide branches whose masks are sign-bit arrays, bf16 activations with 16-byte aligned rows"""
    return (TOP_FUSED and M >= 64 and M % 64 == 0 and 1 <= n0 <= 112 and nc == 512 and bits_cols is not None and len(bits_cols) == 2
            and all(b is not None for b in bits_cols)
            and all(t.dtype == BF16 and t.dim() == 2 and t.stride(1) == 1 and t.stride(0) % 8 == 0 and t.shape[1] >= 112
                    and t.data_ptr() % 16 == 0 for t in masks))


def critic_top_backward(seed, w_out_col, m1, mh, m0, W2nn, W1nn, Wmnn, bits_cols, n0, act, slope=0.0, gcat=None):
    """sweep 2 through the top of a branch critic in ONE launch (dhaug_critic_top_backward_bf16): returns (gz_m2, gz_m1, gz_m0, gcat) --
    bf16 (M, 112) cotangents at the logit layer's input / the merge block's fc1 pre-activation / the merge layer's pre-activation, and
    (M, 512) at the branches' outputs.  seed (M, >= 1) bf16; w_out_col: the logit layer's weights along dim 0; m1, mh, m0: saved
    activations; W2nn, W1nn (n0, >= 112), Wmnn (512, >= 112): operand copies whose rows are the products' outputs."""
    M = m1.shape[0]
    dev = m1.device
    g2, g1, g0 = (torch.empty((M, 112), dtype=BF16, device=dev) for _ in range(3))
    if gcat is None:
        gcat = torch.empty((M, 512), dtype=BF16, device=dev)
    assert gcat.dtype == BF16 and gcat.stride(1) == 1 and gcat.shape[0] == M and gcat.shape[1] >= 512
    assert all(b.device == dev for b in bits_cols), "sign bits must live on the operands' device"
    d = _lib.TopDesc()
    d.seed, d.ld_seed, d.wout, d.ld_wout = _p(seed), seed.stride(0), _p(w_out_col), w_out_col.stride(0)
    d.x, d.ldx = None, 0
    d.m1, d.mh, d.m0, d.ld_m = _p(m1), _p(mh), _p(m0), m1.stride(0)
    assert mh.stride(0) == m1.stride(0) and m0.stride(0) == m1.stride(0)
    d.w2, d.ldw2, d.w1, d.ldw1, d.wm, d.ldwm = _p(W2nn), W2nn.stride(0), _p(W1nn), W1nn.stride(0), _p(Wmnn), Wmnn.stride(0)
    d.bits0, d.bits1 = _p(bits_cols[0]), _p(bits_cols[1])
    d.g2, d.g1, d.g0, d.ld_g, d.gcat, d.ld_gcat = _p(g2), _p(g1), _p(g0), 112, _p(gcat), gcat.stride(0)
    d.M, d.n0, d.nc, d.mask_act, d.mask_slope = M, n0, 512, act, float(slope)
    _lib.call("dhaug_critic_top_backward_bf16", ctypes.byref(d), _stream())
    return g2, g1, g0, gcat


def critic_top_tangent(ucat, m0, mh, m1, Wm_nt, W1_nt, W2_nt, n0, act, slope=0.0):
    """sweep 3 through the top of a branch critic in ONE launch (dhaug_critic_top_tangent_bf16), IN PLACE: the rows of the saved
    activations m0, mh, m1 (the interpolated rows' views) are overwritten with the tangents um0, umh, um1, which are returned.
    ucat (M, 512) bf16; Wm_nt (n0, >= 512), W1_nt / W2_nt (n0, >= 112): the layers' "nt" operand copies."""
    M = ucat.shape[0]
    assert ucat.dtype == BF16 and ucat.stride(1) == 1 and ucat.shape[1] >= 512
    assert mh.stride(0) == m0.stride(0) and m1.stride(0) == m0.stride(0)
    d = _lib.TopDesc()
    d.seed, d.ld_seed, d.wout, d.ld_wout = None, 0, None, 0
    d.x, d.ldx = _p(ucat), ucat.stride(0)
    d.m1, d.mh, d.m0, d.ld_m = _p(m1), _p(mh), _p(m0), m0.stride(0)
    d.w2, d.ldw2, d.w1, d.ldw1, d.wm, d.ldwm = _p(W2_nt), W2_nt.stride(0), _p(W1_nt), W1_nt.stride(0), _p(Wm_nt), Wm_nt.stride(0)
    d.bits0, d.bits1, d.g2, d.g1, d.g0, d.ld_g, d.gcat, d.ld_gcat = None, None, None, None, None, 0, None, 0
    d.M, d.n0, d.nc, d.mask_act, d.mask_slope = M, n0, 512, act, float(slope)
    _lib.call("dhaug_critic_top_tangent_bf16", ctypes.byref(d), _stream())
    return m0, mh, m1


def top_tangent_ok(M, n0, nc, ucat, masks):
    return (TOP_FUSED and M >= 64 and M % 64 == 0 and 1 <= n0 <= 112 and nc == 512 and ucat.dtype == BF16 and ucat.dim() == 2
            and ucat.stride(1) == 1 and ucat.stride(0) % 8 == 0 and ucat.shape[1] >= 512 and ucat.data_ptr() % 16 == 0
            and all(t.dtype == BF16 and t.dim() == 2 and t.stride(1) == 1 and t.stride(0) % 8 == 0 and t.shape[1] >= 112
                    and t.data_ptr() % 16 == 0 and t.stride(0) == masks[0].stride(0) for t in masks))


def add_f32(a, b):
    """a + b (fp32, same shape)"""
    a, b = _dev(a, torch.float32, "add_f32"), _dev(b, torch.float32, "add_f32")
    assert a.shape == b.shape
    out = torch.empty_like(a)
    _lib.call("dhaug_add_f32", _p(a), _p(b), _p(out), a.numel(), _stream())
    return out


def frame_diff(x, R, in_w, w=None, adjoint=False):
    """clips (rows, R*in_w) -> adjacent-frame differences (rows, (R-1)*w) over the first w columns of every frame; adjoint:
    (rows, (R-1)*w) -> (rows, R*in_w), the transposed map"""
    w = in_w if w is None else w
    v = _dev(x, torch.float32, "frame_diff")
    rows = v.shape[0]
    out = torch.empty((rows, R * in_w if adjoint else (R - 1) * w), dtype=torch.float32, device=v.device)
    _lib.call("dhaug_frame_diff", _p(v), _p(out), rows, R, in_w, w, int(bool(adjoint)), _stream())
    return out


def frame_reverse(x, R, w):
    """clips (rows, R*w) -> the frames of every clip in reverse order (its own transpose: also the backward map)"""
    v = _dev(x, torch.float32, "frame_reverse")
    rows = v.shape[0]
    assert v.shape[1] == R * w
    out = torch.empty_like(v)
    _lib.call("dhaug_frame_reverse", _p(v), _p(out), rows, R, w, _stream())
    return out


def weighted_means(arrays, weights):
    """0-dim fp32 tensor sum_i weights[i] * mean(arrays[i]) (fp32 device tensors, contiguous), one launch"""
    n = len(arrays)
    assert 1 <= n <= 16 and len(weights) == n
    arrs = [_dev(a, torch.float32, "weighted_means").reshape(-1) for a in arrays]
    out = torch.empty((1,), dtype=torch.float32, device=arrs[0].device)
    P = (_vp * n)(*[a.data_ptr() for a in arrs])
    C = (ctypes.c_int64 * n)(*[a.numel() for a in arrs])
    W = (ctypes.c_float * n)(*[float(w) for w in weights])
    _lib.call("dhaug_weighted_means", P, C, W, n, _p(out), _stream())
    return out.reshape(())


# ---------------------------------------------------------------------------------------------- posenet: BatchNorm + ReLU + dropout
def bn_workspace(C, device=None):
    """the chunk partials between the two launches of a BatchNorm pass (DHAUG_BN_MAX_CHUNKS x 2 x C fp64; one pass at a time)"""
    return torch.empty(_lib.BN_MAX_CHUNKS * 2 * C, dtype=torch.float64, device=device if device is not None else "cuda")


def _bn_rows(t, C, name, what, like=None):
    """a (M, >= C) fp32 / bf16 matrix the BatchNorm kernels read where it lies: (tensor, row pitch)"""
    if not t.is_cuda:
        raise RuntimeError("dhaug op `%s` needs a GPU tensor (no CPU fallback exists)" % name)
    if t.dim() != 2 or t.shape[1] < C or t.dtype not in (torch.float32, BF16):
        raise ValueError("%s: %s must be a fp32 or bf16 (M, >= %d) matrix, got %s %s" % (name, what, C, t.dtype, tuple(t.shape)))
    if like is not None and (t.dtype != like.dtype or t.shape[0] != like.shape[0]):
        raise ValueError("%s: %s must have z's dtype and rows, got %s %s" % (name, what, t.dtype, tuple(t.shape)))
    if t.stride(1) != 1 or (t.stride(0) * t.element_size()) % 16 or t.data_ptr() % 16 or t.stride(0) < C:
        t = t.contiguous()
        if t.data_ptr() % 16 or (t.stride(0) * t.element_size()) % 16:
            raise ValueError("%s: the rows of %s do not start 16-byte aligned" % (name, what))
    return t, t.stride(0)


def _bn_vec(t, C, name, what):
    if not (t.is_cuda and t.dtype == torch.float32 and t.numel() == C and t.is_contiguous()):
        raise ValueError("%s: %s must be a contiguous fp32 device vector of %d elements" % (name, what, C))
    return t


def _bn_outputs(M, C, dev, out_bf16, out_f32):
    yb = torch.empty((M, ceil_to(C, 16)), dtype=BF16, device=dev) if out_bf16 else None
    yf = torch.empty((M, C), dtype=torch.float32, device=dev) if out_f32 else None
    return yb, yf


def _bn_rng(rng, name):
    """(entry suffix, the two rng arguments): rng = (seed, offset) as numbers, or (cell, delta) with cell a 2-element int64 device
    tensor {seed, base} that the launch reads when it runs (the _dr entries)"""
    if torch.is_tensor(rng[0]):
        cell = rng[0]
        if not (cell.is_cuda and cell.dtype == torch.int64 and cell.numel() == 2 and cell.is_contiguous()):
            raise ValueError("%s: an rng cell must be a contiguous int64 device tensor of 2 elements {seed, base}" % name)
        return "_dr", (_p(cell), int(rng[1]) & 0xFFFFFFFFFFFFFFFF)
    return "", (int(rng[0]), int(rng[1]))


def bn_act_forward(z, C, gamma, beta, residual=None, stats=None, buffers=None, momentum=0.1, eps=1e-5, p=0.0, rng=(0, 0),
                   workspace=None, out_bf16=None, out_f32=None):
    """y = dropout_p(relu(batchnorm(z))) (+ residual) over the first C columns of z (M, >= C; fp32 or bf16; residual of the same type),
    dhaug_bn_partials + dhaug_bn_act_forward.  stats = (mean, rstd): the given-statistics mode (one launch, nothing updated);
    otherwise batch statistics, and buffers = (running_mean, running_var, num_batches_tracked) are updated as nn.BatchNorm1d does.
    rng = (seed, offset) of the dropout's Philox stream, or (cell, delta): seed = cell[0], offset = cell[1] + delta, read on the
    device (dhaug_bn_act_forward_dr).  Returns (y_bf16 (M, ceil16 C) | None, y_f32 (M, C) | None, mean, rstd);
    by default the output has z's type."""
    z, ld_z = _bn_rows(z, C, "bn_act_forward", "z")
    M, dev, zb = z.shape[0], z.device, z.dtype == BF16
    res, ld_res = (None, 0) if residual is None else _bn_rows(residual, C, "bn_act_forward", "residual", z)
    g, b = _bn_vec(gamma, C, "bn_act_forward", "gamma"), _bn_vec(beta, C, "bn_act_forward", "beta")
    out_bf16 = zb if out_bf16 is None else out_bf16
    out_f32 = (not zb) if out_f32 is None else out_f32
    yb, yf = _bn_outputs(M, C, dev, out_bf16, out_f32)
    rm = rv = nbt = ws = None
    if stats is not None:
        mean, rstd = _bn_vec(stats[0], C, "bn_act_forward", "mean"), _bn_vec(stats[1], C, "bn_act_forward", "rstd")
    else:
        if M == 1:
            raise ValueError("Expected more than 1 value per channel when training, got input size %s" % (tuple(z.shape),))
        mean, rstd = torch.empty(C, dtype=torch.float32, device=dev), torch.empty(C, dtype=torch.float32, device=dev)
        ws = workspace if workspace is not None else bn_workspace(C, dev)
        assert ws.is_cuda and ws.dtype == torch.float64 and ws.numel() >= _lib.BN_MAX_CHUNKS * 2 * C
        if buffers is not None:
            rm, rv, nbt = buffers
            _bn_vec(rm, C, "bn_act_forward", "running_mean"), _bn_vec(rv, C, "bn_act_forward", "running_var")
            assert nbt is None or (nbt.is_cuda and nbt.dtype == torch.int64 and nbt.numel() == 1)
        _lib.call("dhaug_bn_partials", _p(z), int(zb), ld_z, M, C, _p(ws), _stream())
    dr, rng_args = _bn_rng(rng, "bn_act_forward")
    _lib.call("dhaug_bn_act_forward" + dr, _p(z), int(zb), ld_z, _p(res), ld_res, _p(g), _p(b), _p(mean), _p(rstd), _p(ws), _p(rm), _p(rv),
              _p(nbt), float(momentum), float(eps), float(p), rng_args[0], rng_args[1], _p(yb), 0 if yb is None else yb.stride(0),
              _p(yf), 0 if yf is None else yf.stride(0), M, C, _stream())
    return yb, yf, mean, rstd


def bn_act_backward(z, C, g, gamma, beta, mean, rstd, p=0.0, rng=(0, 0), workspace=None, out_bf16=None, out_f32=None):
    """backward of bn_act_forward's branch for the cotangent g (z's type and rows): (dz_bf16 | None, dz_f32 | None, dgamma, dbeta);
    dhaug_bn_act_backward_partials + dhaug_bn_act_backward (their _dr forms for rng = (cell, delta)) with the forward call's (p, rng)."""
    z, ld_z = _bn_rows(z, C, "bn_act_backward", "z")
    g, ld_g = _bn_rows(g, C, "bn_act_backward", "g", z)
    M, dev, zb = z.shape[0], z.device, z.dtype == BF16
    vec = [_bn_vec(t, C, "bn_act_backward", n) for t, n in ((gamma, "gamma"), (beta, "beta"), (mean, "mean"), (rstd, "rstd"))]
    out_bf16 = zb if out_bf16 is None else out_bf16
    out_f32 = (not zb) if out_f32 is None else out_f32
    dzb, dzf = _bn_outputs(M, C, dev, out_bf16, out_f32)
    dgamma, dbeta = torch.empty(C, dtype=torch.float32, device=dev), torch.empty(C, dtype=torch.float32, device=dev)
    ws = workspace if workspace is not None else bn_workspace(C, dev)
    assert ws.is_cuda and ws.dtype == torch.float64 and ws.numel() >= _lib.BN_MAX_CHUNKS * 2 * C
    dr, rng_args = _bn_rng(rng, "bn_act_backward")
    head = (_p(z), int(zb), ld_z, _p(g), ld_g, _p(vec[0]), _p(vec[1]), _p(vec[2]), _p(vec[3]), float(p)) + rng_args
    _lib.call("dhaug_bn_act_backward_partials" + dr, *head, M, C, _p(ws), _stream())
    _lib.call("dhaug_bn_act_backward" + dr, *head, _p(ws), _p(dzb), 0 if dzb is None else dzb.stride(0), _p(dzf),
              0 if dzf is None else dzf.stride(0), _p(dgamma), _p(dbeta), M, C, _stream())
    return dzb, dzf, dgamma, dbeta


def bn_fold(W, gamma, beta, running_mean, running_var, eps=1e-5, want_weight=True, layer_bias=None):
    """evaluation-mode BatchNorm folded into the (N, K) layer in front of it (dhaug_bn_fold): returns (W' | None, b', rstd_run).
    layer_bias: the layer's own bias (N fp32), which b' then carries through the BatchNorm (dhaug_bn_fold_bias)"""
    N = gamma.numel()
    v = [_bn_vec(t, N, "bn_fold", n) for t, n in ((gamma, "gamma"), (beta, "beta"), (running_mean, "running_mean"),
                                                  (running_var, "running_var"))]
    dev = gamma.device
    Wd = Wo = None
    K = 0
    if want_weight:
        Wd = _dev(W.detach().reshape(N, -1), torch.float32, "bn_fold")
        K = Wd.shape[1]
        Wo = torch.empty_like(Wd)
    bias, rstd = torch.empty(N, dtype=torch.float32, device=dev), torch.empty(N, dtype=torch.float32, device=dev)
    if layer_bias is None:
        _lib.call("dhaug_bn_fold", _p(Wd), K, _p(v[0]), _p(v[1]), _p(v[2]), _p(v[3]), float(eps), _p(Wo), K, _p(bias), _p(rstd), N, K,
                  _stream())
    else:
        lb = _bn_vec(layer_bias.detach(), N, "bn_fold", "layer_bias")
        _lib.call("dhaug_bn_fold_bias", _p(Wd), K, _p(lb), _p(v[0]), _p(v[1]), _p(v[2]), _p(v[3]), float(eps), _p(Wo), K, _p(bias),
                  _p(rstd), N, K, _stream())
    return Wo, bias, rstd


# ---------------------------------------------------------------------------------------------- multi-frame posenets: tap layout
def conv_taps_pack_bf16(W, want_nn=True, nt=None, nn=None):
    """fp32 Conv1d weight (N, Cin, k) -> (nt bf16 (N, k Cin), nn bf16 (k Cin, ceil16 N) | None): dhaug_conv_taps_pack_bf16.
    nt / nn: write into these (row-strided views allowed) instead of allocating."""
    w = _dev(W, torch.float32, "conv_taps_pack_bf16")
    if w.dim() != 3:
        raise ValueError("conv_taps_pack_bf16: a Conv1d weight (N, Cin, k) is expected, got %s" % (tuple(w.shape),))
    N, Cin, k = w.shape
    if nt is None:
        nt = torch.empty((N, k * Cin), dtype=BF16, device=w.device)
    if nn is None and want_nn:
        nn = torch.empty((k * Cin, ceil_to(N, 16)), dtype=BF16, device=w.device)
    for t, rows in ((nt, N), (nn, k * Cin)):
        assert t is None or (t.dtype == BF16 and t.is_cuda and t.dim() == 2 and t.stride(1) == 1 and t.shape[0] == rows)
    _lib.call("dhaug_conv_taps_pack_bf16", _p(w), N, Cin, k, _p(nt), nt.stride(0), _p(nn), 0 if nn is None else nn.stride(0), _stream())
    return nt, nn


def conv_taps_permute_f32(src, N, Cin, k, to_taps, out=None, accumulate=False):
    """to_taps: fp32 (N, Cin, k) -> (N, k Cin) with out[n, j Cin + c] = src[n, c, j]; otherwise (N, k Cin) -> (N, Cin, k), added
    into `out` when accumulate is set (dhaug_conv_taps_permute_f32)"""
    s = _dev(src, torch.float32, "conv_taps_permute_f32")
    if s.numel() != N * Cin * k:
        raise ValueError("conv_taps_permute_f32: %d elements given for N, Cin, k = %d, %d, %d" % (s.numel(), N, Cin, k))
    shape = (N, k * Cin) if to_taps else (N, Cin, k)
    if out is None:
        if accumulate:
            raise ValueError("conv_taps_permute_f32: accumulate needs a destination")
        out = torch.empty(shape, dtype=torch.float32, device=s.device)
    assert out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and out.numel() == s.numel()
    _lib.call("dhaug_conv_taps_permute_f32", _p(s), _p(out), N, Cin, k, int(bool(to_taps)), int(bool(accumulate)), _stream())
    return out


def tap_gather(x, nseq, t_in, C, k, dilation=1, stride=1, out_bf16=None, out_f32=None, want_bf16=None, want_f32=None):
    """the A operand of a k-tap layer: x (nseq * t_in, >= C) fp32 / bf16 rows -> (out_bf16 | None, out_f32 | None), each
    (nseq * t_out, k C) with out[s t_out + t, j C + c] = x[s t_in + t stride + j dilation, c] (dhaug_tap_gather).  By default the
    output has x's type; out_bf16 / out_f32: write into these (row-strided views allowed)."""
    if not x.is_cuda:
        raise RuntimeError("dhaug op `tap_gather` needs a GPU tensor (no CPU fallback exists)")
    if x.dim() != 2 or x.dtype not in (torch.float32, BF16) or x.shape[0] != nseq * t_in or x.shape[1] < C:
        raise ValueError("tap_gather: x must be a fp32 or bf16 (%d, >= %d) matrix, got %s %s" % (nseq * t_in, C, x.dtype, tuple(x.shape)))
    xb = x.dtype == BF16
    if x.stride(1) != 1 or (x.stride(0) * x.element_size()) % 16 or x.data_ptr() % 16 or x.stride(0) < C:
        x = x.contiguous()
    want_bf16 = (xb or out_bf16 is not None) if want_bf16 is None else want_bf16
    want_f32 = ((not xb and out_bf16 is None) or out_f32 is not None) if want_f32 is None else want_f32
    t_out = (t_in - (k - 1) * dilation - 1) // stride + 1
    rows = nseq * max(t_out, 0)
    if want_bf16 and out_bf16 is None:
        out_bf16 = torch.empty((rows, k * C), dtype=BF16, device=x.device)
    if want_f32 and out_f32 is None:
        out_f32 = torch.empty((rows, k * C), dtype=torch.float32, device=x.device)
    for t, dt in ((out_bf16, BF16), (out_f32, torch.float32)):
        assert t is None or (t.dtype == dt and t.is_cuda and t.dim() == 2 and t.stride(1) == 1 and t.shape[0] == rows)
    _lib.call("dhaug_tap_gather", _p(x), int(xb), x.stride(0), nseq, t_in, C, k, dilation, stride, _p(out_bf16),
              0 if out_bf16 is None else out_bf16.stride(0), _p(out_f32), 0 if out_f32 is None else out_f32.stride(0), _stream())
    return out_bf16, out_f32


# ---------------------------------------------------------------------------------------------- SemGCN posenet: the joint mix
def graph_adj_workspace(device=None):
    """the per-workgroup partials of one adjacency gradient (DHAUG_GRAPH_ADJ_WORKSPACE_DOUBLES fp64; one call at a time)"""
    return torch.empty(_lib.GRAPH_ADJ_WORKSPACE_DOUBLES, dtype=torch.float64, device=device if device is not None else "cuda")


def _graph_rows(t, width, name, what):
    """a (16 x poses, >= width) fp32 / bf16 matrix the graph kernels read where it lies, at any pitch and address (they take 16-byte
    accesses only where both allow it): (tensor, row pitch)"""
    if not t.is_cuda:
        raise RuntimeError("dhaug op `%s` needs a GPU tensor (no CPU fallback exists)" % name)
    if t.dim() != 2 or t.shape[1] < width or t.dtype not in (torch.float32, BF16):
        raise ValueError("%s: %s must be a fp32 or bf16 (M, >= %d) matrix, got %s %s" % (name, what, width, t.dtype, tuple(t.shape)))
    if t.shape[0] % 16:
        raise ValueError("%s: %s must hold 16 rows per pose, got %d rows" % (name, what, t.shape[0]))
    if t.stride(1) != 1 or t.stride(0) < width:
        t = t.contiguous()
    return t, t.stride(0)


def _graph_vec(t, n, name, what, dtype=torch.float32):
    if not (t.is_cuda and t.dtype == dtype and t.numel() == n and t.is_contiguous()):
        raise ValueError("%s: %s must be a contiguous %s device tensor of %d elements" % (name, what, dtype, n))
    return t


def graph_mix(H, A, bias, C, transpose=False, out_bf16=None, out=None):
    """dhaug_graph_mix.  Forward: H = [h0 | h1] (M, >= 2C), fp32 or bf16, a row-strided view allowed; A 16 x 16 fp32; bias (C,) fp32 or
    None -> z[b,i] = A[i,i] h0[b,i] + sum_{j != i} A[i,j] h1[b,j] + bias, fp32 (M, C) or bf16 (M, ceil16 C) with a zero pad.
    transpose: H is the cotangent g (M, >= C) -> dH (M, 2C) (bf16: ceil16(2C) columns), dh0[b,i] = A[i,i] g[b,i], dh1[b,j] =
    sum_{i != j} A[i,j] g[b,i].  By default the output has the input's type; out: write into this matrix (a column block of a wider
    buffer allowed; no column beyond its own is touched) instead of allocating."""
    name = "graph_mix"
    src, ld = _graph_rows(H, C if transpose else 2 * C, name, "g" if transpose else "H")
    A = _graph_vec(A, 256, name, "A")
    if bias is not None:
        if transpose:
            raise ValueError("graph_mix: the adjoint takes no bias")
        bias = _graph_vec(bias, C, name, "bias")
    width = 2 * C if transpose else C
    M = src.shape[0]
    if out is not None:
        out_bf16 = out.dtype == BF16
        need = ceil_to(width, 16) if out_bf16 else width
        if not (out.is_cuda and out.dim() == 2 and out.dtype in (torch.float32, BF16) and out.shape == (M, need) and out.stride(1) == 1
                and out.stride(0) >= need):
            raise ValueError("graph_mix: out must be a fp32 or bf16 (%d, %d) matrix with contiguous rows, got %s %s"
                             % (M, need, out.dtype, tuple(out.shape)))
    else:
        out_bf16 = (src.dtype == BF16) if out_bf16 is None else bool(out_bf16)
        out = torch.empty((M, ceil_to(width, 16) if out_bf16 else width), dtype=BF16 if out_bf16 else torch.float32, device=src.device)
    _lib.call("dhaug_graph_mix", _p(src), int(src.dtype == BF16), ld, _p(A), _p(bias), _p(out), int(out_bf16), out.stride(0), M, C,
              int(bool(transpose)), _stream())
    return out


def graph_adj_grad(G, H, pairs, C, workspace=None, out=None):
    """dhaug_graph_adj_grad: dA (16, 16) fp32 with dA[i,j] = sum_{b,c} G[b,i,c] (i == j ? h0 : h1)[b,j,c] at the pairs (i, j) listed in
    `pairs` (int32 (nnz, 2) on the device, nnz <= 256) and exactly 0 elsewhere; fp64 sums in a fixed order"""
    name = "graph_adj_grad"
    g, ld_g = _graph_rows(G, C, name, "G")
    h, ld_h = _graph_rows(H, 2 * C, name, "H")
    if g.shape[0] != h.shape[0]:
        raise ValueError("graph_adj_grad: G and H differ in rows, %d and %d" % (g.shape[0], h.shape[0]))
    if pairs.dim() != 2 or pairs.shape[1] != 2 or pairs.shape[0] > _lib.GRAPH_MAX_PAIRS:
        raise ValueError("graph_adj_grad: pairs must be (nnz <= %d, 2), got %s" % (_lib.GRAPH_MAX_PAIRS, tuple(pairs.shape)))
    pairs = _graph_vec(pairs, pairs.numel(), name, "pairs", torch.int32)
    ws = workspace if workspace is not None else graph_adj_workspace(g.device)
    assert ws.is_cuda and ws.dtype == torch.float64 and ws.numel() >= _lib.GRAPH_ADJ_WORKSPACE_DOUBLES
    dA = torch.empty((16, 16), dtype=torch.float32, device=g.device) if out is None else _graph_vec(out, 256, name, "out")
    _lib.call("dhaug_graph_adj_grad", _p(g), int(g.dtype == BF16), ld_g, _p(h), int(h.dtype == BF16), ld_h, _p(pairs), pairs.shape[0],
              _p(dA), _p(ws), g.shape[0], C, _stream())
    return dA


def graph_wcat(src, to_cat=True):
    """dhaug_graph_wcat: W (2, in, out) -> Wcat (2 out, in) = [W[0]^T ; W[1]^T]; to_cat False: the adjoint, (2 out, in) -> (2, in, out)"""
    s = _graph_vec(src.detach(), src.numel(), "graph_wcat", "src")
    if to_cat:
        if s.dim() != 3 or s.shape[0] != 2:
            raise ValueError("graph_wcat: W must be (2, in, out), got %s" % (tuple(s.shape),))
        n_in, n_out = s.shape[1], s.shape[2]
        dst = torch.empty((2 * n_out, n_in), dtype=torch.float32, device=s.device)
    else:
        if s.dim() != 2 or s.shape[0] % 2:
            raise ValueError("graph_wcat: Wcat must be (2 out, in), got %s" % (tuple(s.shape),))
        n_out, n_in = s.shape[0] // 2, s.shape[1]
        dst = torch.empty((2, n_in, n_out), dtype=torch.float32, device=s.device)
    _lib.call("dhaug_graph_wcat", _p(s), _p(dst), n_in, n_out, int(bool(to_cat)), _stream())
    return dst


# ---------------------------------------------------------------------------------------------- PoseFormer posenet: LayerNorm, attention, GELU
def _vec_rows(t, width, name, what, dtypes=(torch.float32, BF16)):
    """a (M, >= width) matrix the vector kernels read where it lies: contiguous rows, base and pitch on the 4-element grid (a view
    that is not is copied): (tensor, row pitch)"""
    if not t.is_cuda:
        raise RuntimeError("dhaug op `%s` needs a GPU tensor (no CPU fallback exists)" % name)
    if t.dim() != 2 or t.shape[1] < width or t.dtype not in dtypes:
        raise ValueError("%s: %s must be a %s (M, >= %d) matrix, got %s %s"
                         % (name, what, " or ".join(str(d) for d in dtypes), width, t.dtype, tuple(t.shape)))
    if t.stride(1) != 1 or t.stride(0) < width or t.stride(0) % 4 or t.data_ptr() % (8 if t.dtype == BF16 else 16):
        if t.shape[1] % 4:
            raise ValueError("%s: %s has rows off the 4-element grid (pitch %d)" % (name, what, t.shape[1]))
        t = t.contiguous()
        if t.data_ptr() % 16:
            t = t.clone()
    return t, t.stride(0)


def _vec_param(t, n, name, what):
    if not (t.is_cuda and t.dtype == torch.float32 and t.numel() == n and t.is_contiguous()):
        raise ValueError("%s: %s must be a contiguous fp32 device tensor of %d elements" % (name, what, n))
    return t


def _check_layernorm_cols(C, name):
    if C < 16 or C % 16 or C > _lib.LAYERNORM_MAX_COLS:
        raise ValueError("%s: C must be a multiple of 16 up to %d (DHAUG_LAYERNORM_MAX_COLS), got %d" % (name, _lib.LAYERNORM_MAX_COLS, C))


def layernorm_forward(x, gamma, beta, eps=1e-5, out_bf16=False, want_stats=True, out=None):
    """dhaug_layernorm_forward: x fp32 or bf16 (M, >= C), C = gamma.numel() -> (y fp32 or bf16 (M, C), mean, rstd) (the statistics fp32
    (M,), None without want_stats).  out: write y into this matrix (any pitch >= C; no column beyond C is touched)."""
    name = "layernorm_forward"
    C = gamma.numel()
    _check_layernorm_cols(C, name)
    x, ld_x = _vec_rows(x, C, name, "x")
    gamma, beta = _vec_param(gamma, C, name, "gamma"), _vec_param(beta, C, name, "beta")
    M = x.shape[0]
    if out is None:
        out = torch.empty((M, C), dtype=BF16 if out_bf16 else torch.float32, device=x.device)
    y, ld_y = _vec_rows(out, C, name, "out")
    if y is not out or y.shape[0] != M:
        raise ValueError("layernorm_forward: out must be a (%d, >= %d) matrix with rows on the 4-element grid" % (M, C))
    mean = torch.empty((M,), dtype=torch.float32, device=x.device) if want_stats else None
    rstd = torch.empty((M,), dtype=torch.float32, device=x.device) if want_stats else None
    _lib.call("dhaug_layernorm_forward", _p(x), int(x.dtype == BF16), ld_x, _p(gamma), _p(beta), float(eps), _p(y), int(y.dtype == BF16),
              ld_y, _p(mean), _p(rstd), M, C, _stream())
    return out, mean, rstd


def layernorm_backward(x, g, gamma, mean, rstd, want_dx=True, want_params=True, dx_bf16=False, workspace=None):
    """dhaug_layernorm_backward: (dx fp32 or bf16 (M, C) or None, dgamma, dbeta fp32 (C,) or None); the parameter gradients are fp64
    column sums in a fixed order through a workspace of _lib.layernorm_workspace_doubles(C) doubles"""
    name = "layernorm_backward"
    C = gamma.numel()
    _check_layernorm_cols(C, name)
    x, ld_x = _vec_rows(x, C, name, "x")
    g, ld_g = _vec_rows(g, C, name, "g")
    M = x.shape[0]
    if g.shape[0] != M or mean.numel() != M or rstd.numel() != M:
        raise ValueError("layernorm_backward: x, g, mean and rstd differ in rows")
    gamma, mean, rstd = _vec_param(gamma, C, name, "gamma"), _vec_param(mean, M, name, "mean"), _vec_param(rstd, M, name, "rstd")
    dx = torch.empty((M, C), dtype=BF16 if dx_bf16 else torch.float32, device=x.device) if want_dx else None
    dgamma = dbeta = ws = None
    if want_params:
        dgamma = torch.empty((C,), dtype=torch.float32, device=x.device)
        dbeta = torch.empty((C,), dtype=torch.float32, device=x.device)
        ws = workspace if workspace is not None else torch.empty(_lib.layernorm_workspace_doubles(C), dtype=torch.float64, device=x.device)
        assert ws.is_cuda and ws.dtype == torch.float64 and ws.numel() >= _lib.layernorm_workspace_doubles(C)
    _lib.call("dhaug_layernorm_backward", _p(x), int(x.dtype == BF16), ld_x, _p(g), int(g.dtype == BF16), ld_g, _p(gamma), _p(mean),
              _p(rstd), _p(dx), int(dx_bf16), C, _p(dgamma), _p(dbeta), _p(ws), M, C, _stream())
    return dx, dgamma, dbeta


def _check_attn(S, N, H, hd, name):
    if not 1 <= N <= _lib.ATTN_MAX_TOKENS:
        raise ValueError("%s: sequences of 1 to %d tokens (DHAUG_ATTN_MAX_TOKENS), got %d" % (name, _lib.ATTN_MAX_TOKENS, N))
    if hd % 4 or not 4 <= hd <= _lib.ATTN_MAX_HEAD_DIM:
        raise ValueError("%s: the head width must be a multiple of 4 from 4 to %d (DHAUG_ATTN_MAX_HEAD_DIM), got %d"
                         % (name, _lib.ATTN_MAX_HEAD_DIM, hd))
    if S < 0 or H < 1:
        raise ValueError("%s: S >= 0 sequences and H >= 1 heads, got %d and %d" % (name, S, H))


def attn_forward(qkv, S, N, H, hd, scale, out_bf16=None, want_lse=True, out=None):
    """dhaug_attn_forward: qkv fp32 or bf16 (S N, >= 3 H hd) = [q | k | v], head h in columns [h hd, (h + 1) hd) of each third ->
    (out (S N, H hd) = softmax(scale q k^T) v per sequence and head, lse fp32 (S, H, N) or None).  By default out has qkv's type."""
    name = "attn_forward"
    _check_attn(S, N, H, hd, name)
    C = H * hd
    qkv, ld = _vec_rows(qkv, 3 * C, name, "qkv")
    if qkv.shape[0] != S * N:
        raise ValueError("attn_forward: qkv must hold S N = %d rows, got %d" % (S * N, qkv.shape[0]))
    if out is None:
        out_bf16 = (qkv.dtype == BF16) if out_bf16 is None else bool(out_bf16)
        out = torch.empty((S * N, C), dtype=BF16 if out_bf16 else torch.float32, device=qkv.device)
    o, ld_o = _vec_rows(out, C, name, "out")
    if o is not out or o.shape[0] != S * N:
        raise ValueError("attn_forward: out must be a (%d, >= %d) matrix with rows on the 4-element grid" % (S * N, C))
    lse = torch.empty((S, H, N), dtype=torch.float32, device=qkv.device) if want_lse else None
    _lib.call("dhaug_attn_forward", _p(qkv), int(qkv.dtype == BF16), ld, _p(o), int(o.dtype == BF16), ld_o, _p(lse), S, N, H, hd,
              float(scale), _stream())
    return out, lse


def attn_backward(qkv, out, lse, dout, S, N, H, hd, scale, dqkv_bf16=None, dqkv=None):
    """dhaug_attn_backward: the whole (S N, 3 H hd) cotangent of qkv = [dq | dk | dv] (by default of qkv's type) from qkv and the
    cotangent dout of out; the forward's out and lse are part of the entry's signature and checked, the kernel forms P again
    from qkv and reads neither (include/dhaug.h)"""
    name = "attn_backward"
    _check_attn(S, N, H, hd, name)
    C = H * hd
    qkv, ld = _vec_rows(qkv, 3 * C, name, "qkv")
    out, ld_o = _vec_rows(out, C, name, "out")
    dout, ld_d = _vec_rows(dout, C, name, "dout")
    if not (qkv.shape[0] == out.shape[0] == dout.shape[0] == S * N):
        raise ValueError("attn_backward: qkv, out and dout must hold S N = %d rows" % (S * N))
    lse = _vec_param(lse, S * H * N, name, "lse")
    if dqkv is None:
        dqkv_bf16 = (qkv.dtype == BF16) if dqkv_bf16 is None else bool(dqkv_bf16)
        dqkv = torch.empty((S * N, 3 * C), dtype=BF16 if dqkv_bf16 else torch.float32, device=qkv.device)
    d, ld_q = _vec_rows(dqkv, 3 * C, name, "dqkv")
    if d is not dqkv or d.shape[0] != S * N:
        raise ValueError("attn_backward: dqkv must be a (%d, >= %d) matrix with rows on the 4-element grid" % (S * N, 3 * C))
    _lib.call("dhaug_attn_backward", _p(qkv), int(qkv.dtype == BF16), ld, _p(out), int(out.dtype == BF16), ld_o, _p(lse), _p(dout),
              int(dout.dtype == BF16), ld_d, _p(d), int(d.dtype == BF16), ld_q, S, N, H, hd, float(scale), _stream())
    return dqkv


def _gelu_rows(t, name, what, dtypes):
    """(tensor, M, C, pitch) of a vector or matrix for the GELU kernels: contiguous data is one row (no rule on its length)"""
    if not t.is_cuda:
        raise RuntimeError("dhaug op `%s` needs a GPU tensor (no CPU fallback exists)" % name)
    if t.dtype not in dtypes or t.dim() not in (1, 2):
        raise ValueError("%s: %s must be a %s vector or matrix, got %s %s" % (name, what, " or ".join(str(d) for d in dtypes), t.dtype, tuple(t.shape)))
    if t.dim() == 2 and t.stride(1) == 1 and t.stride(0) % 4 == 0 and t.stride(0) >= t.shape[1] and t.shape[1] % 4 == 0 \
            and 0 < t.shape[1] < (1 << 28) \
            and t.data_ptr() % (8 if t.dtype == BF16 else 16) == 0:
        return t, t.shape[0], t.shape[1], t.stride(0)
    if not t.is_contiguous():
        t = t.contiguous()
    if t.data_ptr() % 16:
        t = t.clone()
    if t.numel() >= (1 << 28):
        raise ValueError("%s: %s: %d contiguous elements whose rows are off the 4-element grid" % (name, what, t.numel()))
    return t, 1, t.numel(), t.numel()


def gelu_forward(z, out_bf16=False):
    """dhaug_gelu_forward: y = z Phi(z) (the exact GELU) of a fp32 vector or matrix, fp32 or bf16, in z's shape"""
    zz, M, C, ld = _gelu_rows(z, "gelu_forward", "z", (torch.float32,))
    y = torch.empty(z.shape, dtype=BF16 if out_bf16 else torch.float32, device=z.device)
    _lib.call("dhaug_gelu_forward", _p(zz), ld, _p(y), int(out_bf16), C if M > 1 else y.numel(), M, C, _stream())
    return y


def gelu_backward(z, g, out_bf16=False):
    """dhaug_gelu_backward: dz = g (Phi(z) + z phi(z)), g fp32 or bf16 in z's shape, dz fp32 or bf16"""
    name = "gelu_backward"
    if tuple(g.shape) != tuple(z.shape):
        raise ValueError("gelu_backward: z and g differ in shape, %s and %s" % (tuple(z.shape), tuple(g.shape)))
    zz, M, C, ld = _gelu_rows(z, name, "z", (torch.float32,))
    gg, Mg, Cg, ld_g = _gelu_rows(g, name, "g", (torch.float32, BF16))
    if (Mg, Cg) != (M, C):                       # (one of the two is a strided view, the other one row: both as one row)
        zz, M, C, ld = _gelu_rows(z.contiguous().view(-1), name, "z", (torch.float32,))
        gg, Mg, Cg, ld_g = _gelu_rows(g.contiguous().view(-1), name, "g", (torch.float32, BF16))
    dz = torch.empty(z.shape, dtype=BF16 if out_bf16 else torch.float32, device=z.device)
    _lib.call("dhaug_gelu_backward", _p(zz), ld, _p(gg), int(gg.dtype == BF16), ld_g, _p(dz), int(out_bf16),
              C if M > 1 else dz.numel(), M, C, _stream())
    return dz
