"""GPU tests of dhaug_mlp_forward_x3 unit by unit (csrc/dhaug_mlp_x3.hip, the parity kernel): small programs built from
_lib.MlpUnit and dhaug_pack_wfrag_f16x2[_t16], no module involved, against the fp64 reference of tests/mlp_x3_unit_util.py.

Tier 1 -- exact programs, torch.equal, in both fragment layouts (gemm_layer on v_mfma_f32_32x32x16_f16, gemm_layer16 on
v_mfma_f32_16x16x32_f16) and two data families: integers (every lo piece zero) and two-piece data (inputs a + b 2^-12, weights
c + d 2^-11: the lo planes and both cross terms hold exactly known non-zero content).  For every GEMM unit, row and feature
sum|terms| < 2^22 q over the three kept product terms, the bias and the residual, every stored value equals its hi + lo and every
piece is a normal fp16 number (asserted for every program by tests/test_mlp_x3_units_cpu.py, none excluded): fp32 accumulation is
then exact in any order, and a stale or swapped lo plane, a dropped cross term, a residual taken as hi alone or a bias seeded
into the wrong register quad changes bits.  Outputs wider than 64 columns are read out of the image by OUT_F32 units whose
weights select 64 columns each (weight 1: hi + lo, exact), one launch of the whole program per group.  Every output lies in a
NaN-filled tensor longer and wider than what the program writes; the rest must stay NaN.  Every program runs at M = 1, 127, 128,
129, 300; one per family at M = 643 on two workgroups (three tiles each, the ragged one last: the prefetch of the next tile's
first layer).

Tier 2 -- realistic values (normal weights / sqrt(K), normal inputs, slope 0.01, fp32 biases like 0.1 + 2^-13 that are no fp16
values), one unit per (layout, chunks, map) at M = 129, against fp64 on the fp32 operands.  It catches what exact data cannot: a
bias rounded to fp16, an accumulator that is not fp32.  The bound, derived as in tests/test_gpu_graph_mix.py, per output element
with S = sum|w||x| + |bias|:
  * an operand v is carried as hi + lo with hi = fp16(v), lo = fp16(v - hi): |v - hi| <= 2^-11 |v| and the rounding of lo is
    2^-11 of that, so |dv| <= 2^-22 |v| -- or 2^-25 absolute where the piece is subnormal (spacing 2^-24); a product then errs by
    |w| dx + |x| dw + dw dx <= 2 * 2^-22 |w||x| (1 + 2^-22) + 2^-25 (|w| + |x|);
  * the dropped Wlo Xlo: |lo| <= 2^-11 (1 + 2^-11) of the value, 2^-22 (1 + 2^-10) |w||x|;
    together 3.01 * 2^-22 sum|w||x| + 1.001 * 2^-25 sum(|w| + |x|) over the K products;
  * the three products per k are exact in fp32 (11 x 11 bits); 3 K + 2 fp32 additions, each rounding by at most 2^-24 of a running
    sum below S (1 + 2^-21): 1.001 (3 K + 2) 2^-24 S;
  * the activation does not enlarge a difference (slopes <= 1); the slope's product rounds by 2^-24 of the value;
  * a result read out of the image was split once more: 2^-22 |y| + 2^-25.
The measured error is printed beside the bound (FIGURE ...).  A bound that needs widening to pass is a finding about the kernel."""
import argparse
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

import mlp_x3_unit_util as X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dhaug():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    sys.path.insert(0, ROOT)
    import dhaug_amd
    from dhaug_amd import _lib, ops  # noqa: F401
    return dhaug_amd


@pytest.fixture(scope="module")
def ws(dhaug):
    """the 64 MB workspace of the parked sums: one per module"""
    return torch.empty(X.WORKSPACE_BYTES, dtype=torch.uint8, device="cuda")


@pytest.mark.parametrize("name", [n for f in X.TIER1 for n in X.names(f)])
def test_exact_program(dhaug, ws, name):
    p = X.get(name)
    dev = X.Device(p, dhaug, ws)
    for M in X.MS:
        X.compare(p, dev.run(M), M)


@pytest.mark.parametrize("name", X.names("cap"))
def test_exact_program_three_tiles_per_workgroup(dhaug, ws, name):
    """M = 128 * 5 + 3 under workgroup_cap(2): each persistent workgroup walks three tiles and takes the ragged one last"""
    p = X.get(name)
    assert p.cap == 2 and p.mmax == X.M_CAP
    X.compare(p, X.Device(p, dhaug, ws).run(p.mmax), p.mmax)


@pytest.mark.parametrize("name", X.names("kcs") + ["kcs_cap_int_t32", "kcs_cap_int_t16"])
def test_load_kcs_equals_the_standalone_features(dhaug, ws, name):
    """a program fed poses (LOAD_KCS) and the same program fed ops.kcs_forward(..., f32=True) features through LOAD_F32: bit
    for bit, and both equal to the fp64 reference on those features"""
    p = X.get(name)
    dev = X.Device(p, dhaug, ws)
    feat, _ = dhaug.ops.kcs_forward(dev.inputs["pose"][:, :48].contiguous(), True, f32=True)
    assert torch.equal(feat.cpu().double(), torch.from_numpy(X.kcs_features(p.tensors["pose"]["data"])))
    for M in ((p.mmax,) if p.cap else X.MS):
        a, b = dev.run(M), dev.run(M, features=feat)
        assert torch.equal(a["y"][:M, :p.obs], b["y"][:M, :p.obs])
        X.compare(p, a, M)
        X.compare(p, b, M)


@pytest.mark.parametrize("name", X.names("real"))
def test_realistic_unit_within_derived_bound(dhaug, ws, name):
    p = X.get(name)
    X.compare(p, X.Device(p, dhaug, ws).run(p.mmax), p.mmax, report=lambda s: print("FIGURE", s))


def _module(dhaug, kind, D):
    from dhaug_amd.models_Fk_GAN import Fk_discriminator, Fk_generator, forward_kinematics_DH_model
    args = argparse.Namespace(batch_size=64, random_seed=0, GAN_OUTPUT_DIM=35, GAN_LAMBDA=10, GAN_whether_use_preAngle=True,
                              Gen_DenseDim=D, Dis_DenseDim_3D=D, Dis_DenseDim_2D=D, video_Dis_DenseDim_3D=32,
                              video_Dis_DenseDim_2D=32, GAN_3d_loss_weight=1.0, GAN_2d_loss_weight=0.2, bone_len_scaler="different",
                              whether_use_RT=True, flip_GAN_model_input=True, single_or_multi_train_mode="single",
                              architecture="3,3,3", motion_Dis_whether_use_3dPos_branch=True,
                              motion_Dis_whether_use_3dDiff_branch=True)
    if kind == "gen":
        fk = forward_kinematics_DH_model.Forward_Kinematics_DH_Model(args, ["S1"], None)
        return Fk_generator.Fk_Generator(fk, args, "cuda").cuda()
    if kind == "d3":
        return Fk_discriminator.Fk_3D_Discriminator("cuda", args).cuda()
    return Fk_discriminator.Fk_2D_Discriminator(args, 16).cuda()


@pytest.mark.parametrize("name", X.names("ship"))
def test_shipped_builders_exact(dhaug, ws, name):
    """fused.generator_head / critic2d / critic3d with mode="f16x3" on modules that hold exact parameters, against the same
    programs written out unit by unit in mlp_x3_unit_util (and run that way too): bit for bit at every width the builders accept"""
    from dhaug_amd import fused
    p = X.get(name)
    kind, D = name.split("_")[1], int(name.split("_")[2][1:])
    mod = _module(dhaug, kind, D)
    params = dict(mod.named_parameters())
    with torch.no_grad():
        for k, v in p.sd.items():
            assert params[k].shape == v.shape, k
            params[k].copy_(torch.from_numpy(v).float())
    if kind == "d2":
        mod.slope = 0.25                                                      # a power of two: the slope multiplies exactly
    dev = {n: torch.from_numpy(T["data"]).float().cuda() for n, T in p.tensors.items() if T["data"] is not None}
    ref = torch.from_numpy(p.ref()["out"]["y"]).float()
    unit_by_unit = X.Device(p, dhaug, ws)
    for M in X.MS:
        with torch.no_grad():
            if kind == "gen":
                got = fused.generator_head(mod, dev["z"][:M], mode="f16x3")
            elif kind == "d2":
                got = fused.critic2d(mod, dev["x"][:M], mode="f16x3")
            else:
                got = fused.critic3d(mod, dev["x"][:M], kcs=dev["kcs"][:M], mode="f16x3")
        own = unit_by_unit.run(M)["y"][:M]
        assert got.shape == ref[:M].shape and torch.equal(got.cpu(), ref[:M]), (name, M)
        assert torch.equal(own.cpu(), got.cpu()), (name, M)


@pytest.mark.parametrize("t16", [False, True])
def test_device_packers_match_the_header_formula(dhaug, t16):
    """dhaug_pack_wfrag_f16x2[_t16] against the numpy form of the header's formula: bit for bit, hi and lo blocks both, the
    sentinel words behind the blob untouched; weights with non-zero lo pieces, one on an fp16 rounding tie, a negative zero"""
    lib, ops = dhaug._lib, dhaug.ops
    vp = ctypes.c_void_p
    rng = np.random.default_rng(11)
    for N, K, k0, ldw in ((1, 2, 0, 2), (33, 72, 0, 72), (100, 100, 28, 128), (256, 256, 0, 256), (129, 40, 128, 168), (225, 200, 3, 210)):
        W = rng.standard_normal((N, ldw)).astype(np.float32)
        W[0, k0] = np.float32(1.0 + 2.0 ** -11)                               # a tie: hi = 1 (even), lo = 2^-11
        W[N - 1, k0 + K - 1] = np.float32(-0.0)
        Wd = torch.from_numpy(W).cuda()
        ksteps = 4 * ((K + 63) // 64)
        blob = torch.full((2 * 8 * ksteps * 512 + 16,), 0x7E01, dtype=torch.int16, device="cuda")
        lib.call("dhaug_pack_wfrag_f16x2_t16" if t16 else "dhaug_pack_wfrag_f16x2", vp(Wd.data_ptr()), ldw, vp(blob.data_ptr()), N, K, k0,
                 ops._stream())
        got = blob.cpu().numpy().view(np.uint16)
        want = X.pack_f16x2(W.astype(np.float64), K, k0, t16)
        assert np.array_equal(got[:-16], want), (N, K, k0, int((got[:-16] != want).sum()))
        assert (got[-16:] == 0x7E01).all()
        assert 0x8000 in want and np.count_nonzero(want.reshape(-1, 2, 512)[:, 1]) > 0       # the negative zero; lo blocks hold content
