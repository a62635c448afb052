"""The streaming kernels of csrc/dhaug_pose.hip and the WGAN-GP / video helpers of csrc/dhaug_elem.hip, kernel by kernel, against fp64
restatements (oracle/dhaug_oracle.py, autograd / forward-mode AD on it, plain fp64 torch where the oracle has no function) at ragged
sizes (1, 63, 64, 65, 1000) and at one size per kernel family that makes the capped grid-stride loop run more than once with a
ragged tail (tests/pose_elem_util.py derives those from the launch constants of the sources).

A  size sweeps.  Tolerance, one rule: max|gpu - ref64| <= max(T_project, 4 max|ref32 - ref64|) with T_project the bound the older
   test of that entry point uses and ref32 the same restatement run in fp32 (pose_elem_util.rule prints the figures); pure data
   movement is compared bit for bit; the two reductions against a bound counted from the kernel's summation shape.
B  the clamp of the projection kernels (a fifth of the ratios beyond +-1), forward and backward, and the rule at exactly +-1.
C  linear-map properties on integer-valued inputs, where fp32 arithmetic is exact: <A x, g> == <x, A^T g>, involutions.
D  bounds (outputs with NaN-payload guards on both sides, inputs untouched) and row isolation of the 64-pose tile kernels.
   (Argument errors need no device: tests/test_cpu_boundary.py::test_pose_and_elem_argument_errors.)

entry point                               tests
dhaug_bone_length                         test_bone_kernels_sizes, test_outputs_stay_in_bounds
dhaug_kcs_forward (f32, bf16)             test_bone_kernels_sizes, test_outputs_stay_in_bounds, test_tile_kernels_isolate_rows
dhaug_center_kcs_forward                  test_bone_kernels_sizes, test_outputs_stay_in_bounds, test_tile_kernels_isolate_rows
dhaug_kcs_backward, dhaug_kcs_jvp         test_bone_kernels_sizes, test_outputs_stay_in_bounds, test_tile_kernels_isolate_rows
dhaug_bone_length_swap                    test_bone_kernels_sizes, test_outputs_stay_in_bounds, test_tile_kernels_isolate_rows
dhaug_d3_penalty                          test_bone_kernels_sizes, test_outputs_stay_in_bounds, test_tile_kernels_isolate_rows
dhaug_world_to_camera_project             test_camera_kernels_sizes, test_projection_clamp, test_outputs_stay_in_bounds
dhaug_world_to_camera_project_backward    test_camera_kernels_sizes, test_projection_clamp, test_clamp_boundary_passes_the_gradient,
                                          test_outputs_stay_in_bounds
dhaug_camera_to_world                     test_camera_kernels_sizes, test_outputs_stay_in_bounds
dhaug_project_to_2d                       test_camera_kernels_sizes, test_projection_clamp, test_outputs_stay_in_bounds
dhaug_center_flip, _backward (C = 2, 3)   test_center_flip_sizes, test_center_flip_pairing, test_outputs_stay_in_bounds
dhaug_gp_assemble, _bf16                  test_gp_assemble_sizes, test_outputs_stay_in_bounds
dhaug_gp_penalty, _bf16                   test_gp_penalty_sizes, test_outputs_stay_in_bounds
dhaug_frame_diff (forward, adjoint)       test_frame_kernels_sizes, test_frame_diff_pairing, test_outputs_stay_in_bounds
dhaug_frame_reverse                       test_frame_kernels_sizes, test_frame_reverse_is_an_involution, test_outputs_stay_in_bounds
dhaug_weighted_means                      test_weighted_means_one_array, test_weighted_means_many_arrays
dhaug_critic_scalars                      test_critic_scalars
"""
import argparse
import ctypes
import os
import sys

import pytest
import torch

import pose_elem_util as U
from oracle import dhaug_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
F64, F32, BF16 = torch.float64, torch.float32, torch.bfloat16


@pytest.fixture(scope="module")
def M():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    sys.path.insert(0, ROOT)
    import dhaug_amd
    L = dhaug_amd._lib.lib()
    from dhaug_amd import ops
    return argparse.Namespace(L=L, ops=ops, lib=dhaug_amd._lib)


def dev(t):
    return t.contiguous().cuda()


def ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def bf16_half_ulp(ref64):
    """what rounding an fp32 value near ref to bf16 (8 significant bits) may add: 2^-8 |ref| (+ a hair for |value| vs |ref|)"""
    return ref64.detach().double().abs() * (2.0 ** -8 * 1.001)


# =================================================================================================== A. size sweeps: camera
# T_project: 2e-6 (camera space and projection: test_camera_golden_and_backward, test_random_bl_aug_golden), 1e-4 of the
# gradient's largest element (the same test's backward)
@pytest.mark.parametrize("N", U.N_JOINT)
def test_camera_kernels_sizes(M, N):
    ops, c = M.ops, U.camera_case(N, seed=1)
    r64, r32 = U.w2c_project_ref(c, F64, c["g3"], c["g2"]), U.w2c_project_ref(c, F32, c["g3"], c["g2"])
    X = dev(c["X"])
    c3, p2 = ops.world_to_camera_project(X, c["q"], c["t"], c["cam"])
    U.rule("world_to_camera_project cam3d N=%d" % N, c3, r64[0], r32[0], 2e-6)
    U.rule("world_to_camera_project proj2d N=%d" % N, p2, r64[1], r32[1], 2e-6)
    only3, none2 = ops.world_to_camera_project(X, c["q"], c["t"], None, want2d=False)
    none3, only2 = ops.world_to_camera_project(X, c["q"], c["t"], c["cam"], want3d=False)
    assert none2 is None and none3 is None and same_bits(only3, c3) and same_bits(only2, p2)

    _, _, near = U.clamp_stats(r64[0])
    gx = ops.world_to_camera_project_backward(X, c["q"], c["t"], c["cam"], dev(c["g3"]), dev(c["g2"]))
    U.rule("world_to_camera_project_backward N=%d" % N, gx, r64[2], r32[2], 1e-4 * r64[2].abs().max().item(), keep=~near)

    w = ops.camera_to_world(dev(c["xc"]), dev(c["qn"]), dev(c["tn"]))
    ref = [O.camera_to_world(c["xc"].to(d), c["qn"].to(d), c["tn"].to(d)) for d in (F64, F32)]
    U.rule("camera_to_world N=%d" % N, w, ref[0], ref[1], 2e-6)

    p = ops.project_to_2d(dev(c["xc"]), dev(c["camn"]))
    ref = [O.project_to_2d(c["xc"].to(d), c["camn"].to(d)) for d in (F64, F32)]
    U.rule("project_to_2d N=%d" % N, p, ref[0], ref[1], 2e-6)


# ========================================================================================================== B. the clamp
@pytest.mark.parametrize("with3,with2", [(True, False), (False, True), (True, True)])
def test_projection_clamp(M, with3, with2):
    """x, y ~ N(0, 2), z ~ U(0.5, 6): both sides of the clamp, in w2c_project, project_batch and the backward's zeroed gradient"""
    ops, N = M.ops, U.POSES_PER_PASS_JOINT + 17
    c = U.camera_case(N, seed=1)
    g3, g2 = (c["g3"] if with3 else None), (c["g2"] if with2 else None)
    r64, r32 = U.w2c_project_ref(c, F64, g3, g2), U.w2c_project_ref(c, F32, g3, g2)
    _, clamped, near = U.clamp_stats(r64[0])
    frac, fnear = clamped.double().mean().item(), near.double().mean().item()
    print("clamped ratios %.2f %%, joints within 1e-4 of the boundary %.4f %%" % (100 * frac, 100 * fnear))
    assert 0.10 <= frac <= 0.90 and fnear <= 1e-3
    X = dev(c["X"])
    gx = ops.world_to_camera_project_backward(X, c["q"], c["t"], c["cam"], None if g3 is None else dev(g3),
                                              None if g2 is None else dev(g2))
    U.rule("backward grad3d=%d grad2d=%d" % (with3, with2), gx, r64[2], r32[2], 1e-4 * r64[2].abs().max().item(), keep=~near)
    if with3 and not with2:
        return
    _, p2 = ops.world_to_camera_project(X, c["q"], c["t"], c["cam"], want3d=False)
    U.rule("world_to_camera_project proj2d (clamp)", p2, r64[1], r32[1], 2e-6)
    # at the clamp the output does not depend on the ratio: exactly the value of u = +-1
    _, cl_xc, _ = U.clamp_stats(c["xc"].double())
    frac = cl_xc.double().mean().item()
    assert 0.10 <= frac <= 0.90
    p = ops.project_to_2d(dev(c["xc"]), dev(c["camn"]))
    ref = [O.project_to_2d(c["xc"].to(d), c["camn"].to(d)) for d in (F64, F32)]
    U.rule("project_to_2d (clamp, %.1f %% of the ratios)" % (100 * frac), p, ref[0], ref[1], 2e-6)


def test_clamp_boundary_passes_the_gradient(M):
    """x / z == +-1.0 exactly passes the gradient, as torch.clamp's backward does; one ulp outside does not.  Identity rotation, zero
    translation and x = z make the kernel's ratio exact."""
    up = lambda v: torch.nextafter(torch.tensor(v, dtype=F32), torch.tensor(float("inf") if v > 0 else float("-inf"), dtype=F32)).item()
    X = torch.zeros(2, 16, 3)
    X[..., 2] = 4.0
    X[0, 0] = torch.tensor([2.0, 0.5, 2.0]);     X[0, 1] = torch.tensor([up(2.0), 0.5, 2.0])         # u = 1, 1 + ulp
    X[0, 2] = torch.tensor([-2.0, 0.5, 2.0]);    X[0, 3] = torch.tensor([up(-2.0), 0.5, 2.0])        # u = -1, -(1 + ulp)
    X[0, 4] = torch.tensor([0.5, 3.0, 3.0]);     X[0, 5] = torch.tensor([0.5, up(3.0), 3.0])         # v = 1, 1 + ulp
    X[1, 7] = torch.tensor([0.25, -3.0, 3.0]);   X[1, 8] = torch.tensor([0.25, up(-3.0), 3.0])       # v = -1, -(1 + ulp)
    X[1, 9] = torch.tensor([1.5, -1.5, 1.5])                                                        # both on the boundary
    c = dict(X=X, q=torch.tensor([[1.0, 0.0, 0.0, 0.0]]), t=torch.zeros(1, 3),
             cam=torch.tensor([[1.5, 2.5, 0.1, -0.2, 0.2, 0.05, 0.01, 0.01, -0.02]]))
    g2 = torch.randn(2, 16, 2, generator=U.gen(3)) + 3.0                                            # (no zero cotangent)
    r64 = U.w2c_project_ref(c, F64, None, g2)
    got = M.ops.world_to_camera_project_backward(dev(X), c["q"], c["t"], c["cam"], None, dev(g2)).cpu()
    err, scale = U.maxabs(got, r64[2]), r64[2].abs().max().item()
    print("boundary case: err %.3e, bound %.3e" % (err, 1e-4 * scale))
    assert err <= 1e-4 * scale
    for (n, j, k) in ((0, 0, 0), (0, 2, 0), (0, 4, 1), (1, 7, 1), (1, 9, 0), (1, 9, 1)):             # on the boundary: passes
        assert got[n, j, k].item() != 0.0 and r64[2][n, j, k].item() != 0.0, (n, j, k)
    for (n, j, k) in ((0, 1, 0), (0, 3, 0), (0, 5, 1), (1, 8, 1)):                                   # one ulp outside: exactly 0
        assert got[n, j, k].item() == 0.0 and r64[2][n, j, k].item() == 0.0, (n, j, k)


# ============================================================================================= A. size sweeps: bone kernels
# T_project: 1e-6 bone length and 5e-6 KCS features (test_kcs_golden), 1e-4 of the largest element for VJP / JVP
# (test_kcs_vjp_jvp), 1e-5 bone-length swap (test_random_bl_aug_golden); the penalty of d3_penalty: 1e-5 (1 + pen), the bound of
# test_gradient_penalty_dead_rows for the same quantity; its bf16 tangents: the derivative bound + half a bf16 ulp of the value
@pytest.mark.parametrize("N", U.N_TILE)
def test_bone_kernels_sizes(M, N):
    ops = M.ops
    x = U.fk_poses(N, seed=N)
    X = dev(x)
    g = U.gen(7 * N + 1)
    U.rule("bone_length N=%d" % N, ops.bone_length(X), O.bone_lengths(x.double()), O.bone_lengths(x), 1e-6)
    xc = X - X[:, :1]
    for wl, W, lds in ((True, 30, (32, 40)), (False, 15, (16,))):
        gf, tan = torch.randn(N, W, generator=g), torch.randn(N, 16, 3, generator=g)
        (f64, v64), (f32, v32) = U.kcs_vjp_ref(x, gf, wl, F64), U.kcs_vjp_ref(x, gf, wl, F32)
        f, _ = ops.kcs_forward(X, with_lengths=wl)
        U.rule("kcs_forward W=%d N=%d" % (W, N), f, f64, f32, 5e-6)
        for ld in lds:
            f2, b = ops.kcs_forward(X, with_lengths=wl, f32=(ld == lds[0]), bf16_ld=ld)
            assert f2 is None or same_bits(f2, f)
            assert same_bits(b[:, :W], f.to(BF16)) and not bits(b[:, W:]).any()
            cen, kb = ops.center_kcs_forward(X, ld, wl)
            assert same_bits(cen, xc.reshape(N, 48)) and same_bits(kb, b)
        got = ops.kcs_backward(X, dev(gf), with_lengths=wl)
        U.rule("kcs_backward W=%d N=%d" % (W, N), got.reshape(N, 16, 3), v64, v32, 1e-4 * v64.abs().max().item())
        j64, j32 = U.kcs_jvp_ref(x, tan, wl, F64), U.kcs_jvp_ref(x, tan, wl, F32)
        U.rule("kcs_jvp W=%d N=%d" % (W, N), ops.kcs_jvp(X, dev(tan), with_lengths=wl), j64, j32, 1e-4 * j64.abs().max().item())

    nl = torch.rand(N, 15, generator=g) * 0.4 + 0.1
    sw = ops.bone_length_swap(X, dev(nl))
    U.rule("bone_length_swap N=%d" % N, sw, O.random_bl_aug(x.double(), nl.double()), O.random_bl_aug(x, nl), 1e-5)

    gk, gp = torch.randn(N, 30, generator=g) * 0.01, torch.randn(N, 48, generator=g) * 0.01
    dead = N - 1
    gk[dead] = 0.0; gp[dead] = 0.0                                # every unit of the critic dead on this row: norm 0
    coef = 2.0 * 10.0 / max(N, 64)
    (tk64, v64, pen64), (tk32, v32, pen32) = U.d3_penalty_ref(x, gk, gp, coef, F64), U.d3_penalty_ref(x, gk, gp, coef, F32)
    tk, tv, pen = ops.d3_penalty(X, dev(gk), dev(gp), coef)
    U.rule("d3_penalty pen N=%d" % N, pen, pen64, pen32, 1e-5 * (1.0 + pen64.abs().max().item()))
    U.rule("d3_penalty v (bf16) N=%d" % N, tv.float(), v64, v32, 1e-4 * v64.abs().max().item(), slack=bf16_half_ulp(v64))
    U.rule("d3_penalty tk (bf16) N=%d" % N, tk.float()[:, :30], tk64, tk32, 1e-4 * tk64.abs().max().item(), slack=bf16_half_ulp(tk64))
    assert not bits(tk[:, 30:]).any()
    assert pen[dead].item() == 1.0 and tv[dead].float().abs().max().item() == 0.0 and tk[dead].float().abs().max().item() == 0.0


# ============================================================================================ A. size sweeps: centre / flip
# T_project: 1e-7 forward with centring, 1e-5 adjoint (test_camera_golden_and_backward); without centring the map moves and negates
# values: bit for bit.  References: fp64 / fp32 torch on the device (the oracle's flip_lr on x - x[:, :1], autograd for the adjoint).
@pytest.mark.parametrize("C", [2, 3])
@pytest.mark.parametrize("N", U.N_FLIP)
def test_center_flip_sizes(M, N, C):
    x = dev(torch.randn(N, 16, C, generator=U.gen(N + C)) + torch.randn(N, 1, C, generator=U.gen(N + C + 1)) * 3.0)
    n5 = min(N, 5)
    assert torch.equal(U.center_flip_fwd(x[:n5].cpu(), True, True), O.flip_lr(x[:n5].cpu() - x[:n5, :1].cpu()))
    for center in (False, True):
        for flip in (False, True):
            for adj in (False, True):
                got = M.ops.center_flip(x, center, flip, adjoint=adj)
                ref = U.center_flip_adj if adj else U.center_flip_fwd
                name = "center_flip%s C=%d center=%d flip=%d N=%d" % ("_backward" if adj else "", C, center, flip, N)
                if not center:
                    assert same_bits(got, ref(x, center, flip)), name
                else:
                    U.rule(name, got, ref(x.double(), center, flip), ref(x, center, flip), 1e-5 if adj else 1e-7)


# =============================================================================================== A. size sweeps: WGAN-GP rows
# one lane per element, 4 096 x 256 elements per pass: B = 65 553 rows are 3 passes at W = 48, 2 at W = 30, 18 at W = 288
@pytest.mark.parametrize("W", [30, 48, 32 * 9, 1])
@pytest.mark.parametrize("B", U.N_JOINT)
def test_gp_assemble_sizes(M, B, W):
    g = U.gen(B * 1000 + W)
    r, f, a = dev(torch.randn(B, W, generator=g) * 2.0), dev(torch.randn(B, W, generator=g) - 1.0), dev(torch.rand(B, generator=g))
    out = M.ops.gp_assemble(r, f, a)
    assert out.shape == (3 * B, W) and same_bits(out[:B], r) and same_bits(out[B:2 * B], f)
    ref = [a.to(d)[:, None] * r.to(d) + (1.0 - a.to(d)[:, None]) * f.to(d) for d in (F64, F32)]
    # no older bound: four roundings (1 - alpha, two products, one sum) of values up to max(|r|, |f|)
    floor = 4 * U.U32 * max(r.abs().max().item(), f.abs().max().item())
    U.rule("gp_assemble interpolates B=%d W=%d" % (B, W), out[2 * B:], ref[0], ref[1], floor)
    if W % 16 == 0:
        ob = M.ops.gp_assemble(r, f, a, bf16_rows=True)
        assert same_bits(ob, out) and same_bits(ob._dhaug_bf16_rows, torch.cat([r, f]).to(BF16))


# T_project: 1e-5 on v, 1e-5 (1 + pen) on the penalty (test_gradient_penalty_dead_rows)
@pytest.mark.parametrize("W", [30, 48, 32 * 9, 1])
@pytest.mark.parametrize("B", U.B_GP)
def test_gp_penalty_sizes(M, B, W):
    g = dev(torch.randn(B, W, generator=U.gen(B * 1000 + W)))
    dead = sorted({B // 2, B - 1})
    g[dead] = 0.0
    v, pen = M.ops.gp_penalty(g, 0.25)
    (v64, p64), (v32, p32) = U.gp_penalty_ref(g, 0.25, F64), U.gp_penalty_ref(g, 0.25, F32)
    U.rule("gp_penalty v B=%d W=%d" % (B, W), v, v64, v32, 1e-5)
    U.rule("gp_penalty pen B=%d W=%d" % (B, W), pen, p64, p32, 1e-5 * (1.0 + p64.max().item()))
    assert torch.isfinite(v).all() and v[dead].abs().max().item() == 0.0 and (pen[dead] == 1.0).all()
    if W % 16 == 0:
        vb, pb = M.ops.gp_penalty(g, 0.25, bf16=True)
        assert same_bits(vb, v) and same_bits(pb, pen) and same_bits(vb._dhaug_bf16, v.to(BF16))


# ================================================================================================ A. size sweeps: frame kernels
FRAME_SHAPES = [(2, 48, 48), (9, 48, 48), (9, 48, 30), (27, 32, 32), (3, 5, 1)]


def _frame_rows(R, in_w, w):
    """the ragged sizes and the first row count whose FORWARD launch (rows (R - 1) w elements, the smaller of the two directions)
    needs a second pass of its 4 096 x 256 lanes"""
    return U.RAGGED + [U.ELEMS_PER_PASS // ((R - 1) * w) + 3]


@pytest.mark.parametrize("R,in_w,w", FRAME_SHAPES)
def test_frame_kernels_sizes(M, R, in_w, w):
    for rows in _frame_rows(R, in_w, w):
        g = U.gen(rows + R)
        x, gr = dev(torch.randn(rows, R * in_w, generator=g) * 3.0), dev(torch.randn(rows, (R - 1) * w, generator=g))
        # one subtraction per element: no older bound, the floor is one rounding of the largest value
        y = M.ops.frame_diff(x, R, in_w, w)
        r64 = U.frame_diff_ref(x.double(), R, in_w, w)
        U.rule("frame_diff R=%d in_w=%d w=%d rows=%d" % (R, in_w, w, rows), y, r64, U.frame_diff_ref(x, R, in_w, w),
               U.U32 * r64.abs().max().item())
        a = M.ops.frame_diff(gr, R, in_w, w, adjoint=True)
        a64 = U.frame_diff_adj_ref(gr.double(), R, in_w, w)
        U.rule("frame_diff adjoint R=%d in_w=%d w=%d rows=%d" % (R, in_w, w, rows), a, a64, U.frame_diff_adj_ref(gr, R, in_w, w),
               U.U32 * a64.abs().max().item())
        assert a.shape == (rows, R * in_w) and not bits(a.reshape(rows, R, in_w)[:, :, w:]).any()
        rev = M.ops.frame_reverse(x, R, in_w)
        assert same_bits(rev, x.reshape(rows, R, in_w).flip(1).reshape(rows, R * in_w))


# =================================================================================================== A. the two reductions
def _logits(n, seed, shift=0.3):
    return torch.randn(n, generator=U.gen(seed)) + shift


WM_COUNTS = [1, 2, 63, 1023, 1024, 1025, 3072, 3073, 4096, 4097, 8193, U.N_REDUCE]


@pytest.mark.parametrize("n", WM_COUNTS)
def test_weighted_means_one_array(M, n):
    """|got - mean64| <= gamma_k mean|x|, k = pose_elem_util.wm_depth(n) fp32 operations on the longest path (a dropped wave is off
    by a sixteenth of the mean, a dropped accumulator by a quarter)"""
    x = dev(_logits(n, n))
    got = M.ops.weighted_means([x], [1.0]).item()
    ref, scale = x.double().mean().item(), x.double().abs().mean().item()
    k = U.wm_depth(n)
    print("weighted_means n=%d: err %.3e, bound %.3e (k = %d, mean|x| = %.3f)" % (n, abs(got - ref), U.gamma(k) * scale, k, scale))
    assert abs(got - ref) <= U.gamma(k) * scale


@pytest.mark.parametrize("counts", [[1, 4097, 1023], [4096, 1, U.N_REDUCE],
                                    [1, 1023, 1024, 4096, 4097, U.N_REDUCE, 63, 64, 65, 1000, 3073, 8192, 8193, 2, 5000, 12289]])
def test_weighted_means_many_arrays(M, counts):
    """sum_i w_i mean_i: every mean to its own bound, + the product and the i-th addition of the running total (1 + n operations)"""
    n = len(counts)
    xs = [dev(_logits(c, 31 * i + c, shift=0.3 * (-1) ** i)) for i, c in enumerate(counts)]
    ws = [(-1.0) ** i * (0.5 + 0.25 * i) for i in range(n)]
    got = M.ops.weighted_means(xs, ws).item()
    ref = sum(w * x.double().mean().item() for w, x in zip(ws, xs))
    bound = sum(abs(w) * U.gamma(U.wm_depth(c) + 1 + n) * x.double().abs().mean().item() for w, x, c in zip(ws, xs, counts))
    print("weighted_means %d arrays: err %.3e, bound %.3e" % (n, abs(got - ref), bound))
    assert abs(got - ref) <= bound
    # the arrays in another order: the same means, so the same sum to the same bound (a mean that leaked into the next array would not be)
    got2 = M.ops.weighted_means(xs[::-1], ws[::-1]).item()
    assert abs(got2 - ref) <= bound


@pytest.mark.parametrize("ld", [1, 2, 3])
@pytest.mark.parametrize("B", U.RAGGED + [192, 193, U.N_REDUCE])
def test_critic_scalars(M, B, ld):
    """every mean to gamma_k mean|x| (pose_elem_util.cs_depth), the two derived scalars exactly; the unused columns of a strided
    logit array hold NaN"""
    lam = 10.0
    for P in (B, 3 * B):
        g = U.gen(B + ld + P)
        lg = torch.full((2 * B, ld), float("nan"))
        lg[:B, 0] = torch.randn(B, generator=g) + 0.5
        lg[B:, 0] = torch.randn(B, generator=g) - 0.3
        pen = torch.rand(P, generator=g) * 2.0
        out = M.ops.critic_scalars(dev(lg), dev(pen), B, lam).cpu()
        real, fake, p = lg[:B, 0].double(), lg[B:, 0].double(), pen.double()
        want = (real.mean().item(), fake.mean().item(), lam * p.mean().item())
        bound = (U.gamma(U.cs_depth(B)) * real.abs().mean().item(), U.gamma(U.cs_depth(B)) * fake.abs().mean().item(),
                 lam * U.gamma(U.cs_depth(P, scaled=True)) * p.abs().mean().item())
        err = [abs(out[i].item() - want[i]) for i in range(3)]
        print("critic_scalars B=%d P=%d ld=%d: err %.3e %.3e %.3e, bound %.3e %.3e %.3e" % ((B, P, ld) + tuple(err) + bound))
        assert all(e <= b for e, b in zip(err, bound))
        assert out[3].item() == (out[0] - out[1]).item() and out[4].item() == ((out[1] - out[0]) + out[2]).item()


# ================================================================================================ C. linear-map properties
def _ints(shape, seed):
    return dev(torch.randint(-8, 9, shape, generator=U.gen(seed)).float())


def _dot(a, b):
    return (a.double() * b.double()).sum().item()


@pytest.mark.parametrize("R,in_w,w", FRAME_SHAPES)
def test_frame_diff_pairing(M, R, in_w, w):
    """<frame_diff(x), g> == <x, frame_diff^T(g)> on integers in [-8, 8] (differences, products and their fp64 sums are exact)"""
    for rows in (1, 7, 512, U.ELEMS_PER_PASS // (R * in_w) + 3):
        x, g = _ints((rows, R * in_w), rows + R), _ints((rows, (R - 1) * w), rows + R + 1)
        y, a = M.ops.frame_diff(x, R, in_w, w), M.ops.frame_diff(g, R, in_w, w, adjoint=True)
        assert _dot(y, g) == _dot(x, a), (rows, R, in_w, w)
        assert not bits(a.reshape(rows, R, in_w)[:, :, w:]).any()


@pytest.mark.parametrize("C", [2, 3])
def test_center_flip_pairing(M, C):
    for N in (1, 7, 512, U.POSES_PER_PASS_FLIP + 3):
        x, g = _ints((N, 16, C), N + C), _ints((N, 16, C), N + C + 1)
        for center in (False, True):
            for flip in (False, True):
                y, a = M.ops.center_flip(x, center, flip), M.ops.center_flip(g, center, flip, adjoint=True)
                assert _dot(y, g) == _dot(x, a), (N, C, center, flip)
                assert same_bits(y + 0.0, U.center_flip_fwd(x, center, flip) + 0.0)      # (integers: exact; + 0.0 folds -0)


@pytest.mark.parametrize("R,w", [(1, 48), (2, 48), (9, 32), (27, 5), (3, 1)])
def test_frame_reverse_is_an_involution(M, R, w):
    for rows in (1, 7, 512, U.ELEMS_PER_PASS // (R * w) + 3):
        x = dev(torch.randn(rows, R * w, generator=U.gen(rows + R)))
        x[0, 0] = float("nan")
        x.view(torch.int32)[-1, -1] = 0x7fc0beef                                          # payloads travel too
        y = M.ops.frame_reverse(x, R, w)
        assert same_bits(M.ops.frame_reverse(y, R, w), x)
        assert same_bits(y, x) if R == 1 else same_bits(y.reshape(rows, R, w)[:, 0], x.reshape(rows, R, w)[:, R - 1])


# ==================================================================================================== D. bounds, isolation
PAYLOAD32, PAYLOAD16 = 0x7fc0dead, 0x7fc1


class Guarded:
    """an output of `numel` elements with 64 floats of NaN payload behind it and a guard in front (one float for fp32 outputs, which
    have no alignment contract: the output then starts 4 bytes past a 16-byte boundary; 16 bytes for bf16 ones, which have one)"""

    def __init__(self, numel, dtype):
        self.n, self.lead = numel, (1 if dtype == F32 else 8)
        tail = 64 if dtype == F32 else 128
        self.raw = torch.full((self.lead + numel + tail,), PAYLOAD32 if dtype == F32 else PAYLOAD16,
                              dtype=torch.int32 if dtype == F32 else torch.int16, device="cuda")
        self.out = self.raw[self.lead:self.lead + numel].view(dtype)
        self.payload = self.raw[0].item()

    def check(self, name, written=True):
        assert (self.raw[:self.lead] == self.payload).all() and (self.raw[self.lead + self.n:] == self.payload).all(), name
        if written:                                                        # every element of the output proper was stored
            assert (self.raw[self.lead:self.lead + self.n] != self.payload).all(), name


def _bounds_cases(M, N):
    """(name, inputs, outputs {name: (numel, dtype)}, call(i, o) -> rc): every entry point of the table at N poses / rows"""
    L, s = M.L, stream
    g = U.gen(N)
    x = dev(U.fk_poses(N, seed=N + 2))
    rn = lambda *shape: dev(torch.randn(*shape, generator=g))
    c = U.camera_case(N, seed=2)
    q, t, cam = M.ops._host3(c["q"], 4), M.ops._host3(c["t"], 3), M.ops._host3(c["cam"], 9)      # host float arrays
    X, xc, qn, tn, camn = dev(c["X"]), dev(c["xc"]), dev(c["qn"]), dev(c["tn"]), dev(c["camn"])
    cases = [
        ("bone_length", dict(x=x), dict(o=(N * 15, F32)), lambda i, o: L.dhaug_bone_length(i["x"], o["o"], N, s())),
        ("kcs_backward", dict(x=x, g=rn(N, 30)), dict(o=(N * 48, F32)), lambda i, o: L.dhaug_kcs_backward(i["x"], i["g"], o["o"], N, 1, s())),
        ("kcs_backward15", dict(x=x, g=rn(N, 15)), dict(o=(N * 48, F32)), lambda i, o: L.dhaug_kcs_backward(i["x"], i["g"], o["o"], N, 0, s())),
        ("kcs_jvp", dict(x=x, g=rn(N, 48)), dict(o=(N * 30, F32)), lambda i, o: L.dhaug_kcs_jvp(i["x"], i["g"], o["o"], N, 1, s())),
        ("kcs_jvp15", dict(x=x, g=rn(N, 48)), dict(o=(N * 15, F32)), lambda i, o: L.dhaug_kcs_jvp(i["x"], i["g"], o["o"], N, 0, s())),
        ("bone_length_swap", dict(x=x, l=dev(torch.rand(N, 15, generator=g) + 0.1)), dict(o=(N * 48, F32)),
         lambda i, o: L.dhaug_bone_length_swap(i["x"], i["l"], o["o"], N, s())),
        ("d3_penalty", dict(x=x, gk=rn(N, 30), gp=rn(N, 48)), dict(tk=(N * 32, BF16), tv=(N * 48, BF16), pen=(N, F32)),
         lambda i, o: L.dhaug_d3_penalty(i["x"], i["gk"], i["gp"], 0.5, o["tk"], o["tv"], o["pen"], N, s())),
        ("world_to_camera_project", dict(x=X), dict(c3=(N * 48, F32), p2=(N * 32, F32)),
         lambda i, o: L.dhaug_world_to_camera_project(i["x"], q, t, cam, o["c3"], o["p2"], N, s())),
        ("world_to_camera_project_backward", dict(x=X, g3=rn(N, 48), g2=rn(N, 32)), dict(o=(N * 48, F32)),
         lambda i, o: L.dhaug_world_to_camera_project_backward(i["x"], q, t, cam, i["g3"], i["g2"], o["o"], N, s())),
        ("camera_to_world", dict(x=xc, q=qn, t=tn), dict(o=(N * 48, F32)),
         lambda i, o: L.dhaug_camera_to_world(i["x"], i["q"], i["t"], o["o"], N, s())),
        ("project_to_2d", dict(x=xc, c=camn), dict(o=(N * 32, F32)), lambda i, o: L.dhaug_project_to_2d(i["x"], i["c"], o["o"], N, s())),
        ("frame_reverse", dict(x=rn(N, 9 * 5)), dict(o=(N * 45, F32)), lambda i, o: L.dhaug_frame_reverse(i["x"], o["o"], N, 9, 5, s())),
        ("frame_diff", dict(x=rn(N, 9 * 48)), dict(o=(N * 8 * 30, F32)), lambda i, o: L.dhaug_frame_diff(i["x"], o["o"], N, 9, 48, 30, 0, s())),
        ("frame_diff adjoint", dict(x=rn(N, 8 * 30)), dict(o=(N * 9 * 48, F32)),
         lambda i, o: L.dhaug_frame_diff(i["x"], o["o"], N, 9, 48, 30, 1, s())),
        ("gp_assemble", dict(r=rn(N, 30), f=rn(N, 30), a=rn(N)), dict(o=(3 * N * 30, F32)),
         lambda i, o: L.dhaug_gp_assemble(i["r"], i["f"], i["a"], o["o"], N, 30, s())),
        ("gp_penalty", dict(g=rn(N, 30)), dict(v=(N * 30, F32), pen=(N, F32)),
         lambda i, o: L.dhaug_gp_penalty(i["g"], o["v"], o["pen"], N, 30, 0.25, s())),
        ("gp_penalty W=1", dict(g=rn(N, 1)), dict(v=(N, F32), pen=(N, F32)),
         lambda i, o: L.dhaug_gp_penalty(i["g"], o["v"], o["pen"], N, 1, 0.25, s())),
    ]
    for wl, W in ((1, 30), (0, 15)):
        cases.append(("kcs_forward f32 W=%d" % W, dict(x=x), dict(o=(N * W, F32)),
                      lambda i, o, wl=wl: L.dhaug_kcs_forward(i["x"], o["o"], None, 0, N, wl, s())))
        for ld in (32, 40):
            cases.append(("kcs_forward bf16 W=%d ld=%d" % (W, ld), dict(x=x), dict(o=(N * W, F32), b=(N * ld, BF16)),
                          lambda i, o, wl=wl, ld=ld: L.dhaug_kcs_forward(i["x"], o["o"], o["b"], ld, N, wl, s())))
            cases.append(("center_kcs_forward W=%d ld=%d" % (W, ld), dict(x=x), dict(c=(N * 48, F32), b=(N * ld, BF16)),
                          lambda i, o, wl=wl, ld=ld: L.dhaug_center_kcs_forward(i["x"], o["c"], o["b"], ld, N, wl, s())))
    for C in (2, 3):
        for center in (0, 1):
            for flip in (0, 1):
                for fn in ("dhaug_center_flip", "dhaug_center_flip_backward"):
                    cases.append(("%s C=%d center=%d flip=%d" % (fn, C, center, flip), dict(x=rn(N, 16 * C)), dict(o=(N * 16 * C, F32)),
                                  lambda i, o, C=C, center=center, flip=flip, fn=fn: getattr(L, fn)(i["x"], o["o"], N, C, center, flip, s())))
    return cases


@pytest.mark.parametrize("N", [1, 63, 65])
def test_outputs_stay_in_bounds(M, N):
    for name, ins, outs, call in _bounds_cases(M, N):
        keep = {k: v.clone() for k, v in ins.items()}
        bufs = {k: Guarded(n, dt) for k, (n, dt) in outs.items()}
        rc = call({k: ptr(v) for k, v in ins.items()}, {k: ptr(b.out) for k, b in bufs.items()})
        torch.cuda.synchronize()
        assert rc == 0, name
        for k, b in bufs.items():
            b.check((name, k, N))
        assert all(same_bits(ins[k], keep[k]) for k in ins), name
    # the bf16 copies with a leading dimension beyond W: the columns [W, ld) belong to the caller
    g = U.gen(N + 5)
    r, f, gr = (dev(torch.randn(N, 30, generator=g)) for _ in range(3))
    a = dev(torch.rand(N, generator=g))
    o, b = Guarded(3 * N * 30, F32), Guarded(2 * N * 32, BF16)
    assert M.L.dhaug_gp_assemble_bf16(ptr(r), ptr(f), ptr(a), ptr(o.out), ptr(b.out), 32, N, 30, stream()) == 0
    o.check("gp_assemble_bf16 out"); b.check("gp_assemble_bf16 rows", written=False)
    rows = b.out.view(2 * N, 32)
    assert same_bits(rows[:, :30], torch.cat([r, f]).to(BF16)) and (bits(rows[:, 30:]) == PAYLOAD16).all()
    v, vb, pen = Guarded(N * 30, F32), Guarded(N * 32, BF16), Guarded(N, F32)
    assert M.L.dhaug_gp_penalty_bf16(ptr(gr), ptr(v.out), ptr(vb.out), 32, ptr(pen.out), N, 30, 0.25, stream()) == 0
    v.check("gp_penalty_bf16 v"); pen.check("gp_penalty_bf16 pen"); vb.check("gp_penalty_bf16 rows", written=False)
    rows = vb.out.view(N, 32)
    assert same_bits(rows[:, :30], v.out.view(N, 30).to(BF16)) and (bits(rows[:, 30:]) == PAYLOAD16).all()


def _tile_outputs(M, x, aux):
    """every output of the 64-pose tile kernels for the poses x (N,48), flattened to per-pose rows"""
    ops, N = M.ops, x.shape[0]
    out = {}
    for wl in (True, False):
        f, b32 = ops.kcs_forward(x, with_lengths=wl, bf16_ld=32)
        _, b40 = ops.kcs_forward(x, with_lengths=wl, f32=False, bf16_ld=40)
        cen, cb = ops.center_kcs_forward(x, 32, wl)
        out.update({"kcs f32 %d" % wl: f, "kcs bf16 ld=32 %d" % wl: b32, "kcs bf16 ld=40 %d" % wl: b40, "center_kcs centred %d" % wl: cen,
                    "center_kcs bf16 %d" % wl: cb, "kcs_backward %d" % wl: ops.kcs_backward(x, aux["gf"][:, :30 if wl else 15].contiguous(), wl),
                    "kcs_jvp %d" % wl: ops.kcs_jvp(x, aux["tan"], wl)})
    out["bone_length"] = ops.bone_length(x)
    out["bone_length_swap"] = ops.bone_length_swap(x, aux["nl"]).reshape(N, 48)
    tk, tv, pen = ops.d3_penalty(x, aux["gk"], aux["gp"], 0.1)
    out.update({"d3_penalty tk": tk, "d3_penalty v": tv, "d3_penalty pen": pen.reshape(N, 1)})
    return out


@pytest.mark.parametrize("poison", ["nan", "zero_bone"])
@pytest.mark.parametrize("row", [0, 70, 199])
def test_tile_kernels_isolate_rows(M, poison, row):
    """64 poses share a workgroup's LDS tile: a NaN pose, or one with a zero-length bone (0 / 0 in its cosines), changes its own
    output rows and no bit of any other row (N = 200: three full tiles and a ragged one; rows in the first, second and last)"""
    N = 200
    g = U.gen(11)
    x = dev(U.fk_poses(N, seed=9)).reshape(N, 48)
    aux = dict(gf=dev(torch.randn(N, 30, generator=g)), tan=dev(torch.randn(N, 48, generator=g)),
               nl=dev(torch.rand(N, 15, generator=g) * 0.4 + 0.1), gk=dev(torch.randn(N, 30, generator=g) * 0.01),
               gp=dev(torch.randn(N, 48, generator=g) * 0.01))
    clean = _tile_outputs(M, x, aux)
    bad = x.clone()
    if poison == "nan":
        bad[row] = float("nan")
    else:
        bad[row, 3 * 8:3 * 8 + 3] = bad[row, 3 * 7:3 * 7 + 3]                 # joint 8 on joint 7: bone (7, 8) of both bone tables
    dirty = _tile_outputs(M, bad, aux)
    others = torch.arange(N, device="cuda") != row
    for k in clean:
        assert same_bits(clean[k][others], dirty[k][others]), k
        assert not same_bits(clean[k][row], dirty[k][row]), k                  # (the poison did arrive)
        if poison == "nan" and "bf16" not in k and k != "d3_penalty tk" and k != "d3_penalty v":
            assert torch.isnan(dirty[k][row].float()).all(), k


def test_empty_batches_through_the_wrappers(M):
    """(the C-ABI's N = 0 and argument-error returns need no device: tests/test_cpu_boundary.py)"""
    assert M.ops.frame_diff(torch.empty(0, 9 * 48, device="cuda"), 9, 48, 30).shape == (0, 8 * 30)
    assert M.ops.frame_diff(torch.empty(0, 8 * 30, device="cuda"), 9, 48, 30, adjoint=True).shape == (0, 9 * 48)
    assert M.ops.frame_reverse(torch.empty(0, 9 * 48, device="cuda"), 9, 48).shape == (0, 9 * 48)
    assert M.ops.center_flip(torch.empty(0, 16, 3, device="cuda"), True, True).shape == (0, 16, 3)
    assert M.ops.gp_penalty(torch.empty(0, 48, device="cuda"), 0.25)[1].shape == (0,)
