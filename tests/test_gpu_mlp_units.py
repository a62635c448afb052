"""GPU tests of dhaug_mlp_forward unit by unit (csrc/dhaug_mlp.hip): small programs built from _lib.MlpUnit and the pack entry
points, no module involved, against the fp64 reference of tests/mlp_unit_util.py.

Tier 1 -- exact programs, torch.equal.  The data (small integers, a few weights per row from {+-1/2, +-1}, integer biases, slope
2^-2) make fp32 arithmetic exact in any order of summation: for every GEMM unit, row and feature sum|terms| < 2^22 q, q the
largest power of two dividing every term (asserted for every program by tests/test_mlp_units_cpu.py, none excluded).  The result
then does not depend on tiling, wave ownership, k-chunk order, accumulator seeding or epilogue order, and the comparison has no
tolerance: one wrong column, a residual from the wrong buffer, a dropped or swapped k-chunk changes bits.  Every output lies in a
NaN-filled tensor that is wider and longer than what the program writes; the rest must stay NaN.  Families: single
layer-at-a-time units (shapes 17, 34, 68; all K x N of the issue, three activations, three residual forms, all three buffers, both
LOADs with and without padding columns), two-source units (33, 66, 132), narrow pairs with and without DHAUG_MLP_NOPAIR, DOT_OUT
in and outside a pair, stacks (lead K 32 / 48 / 128 / none, runs of 2, 3, 6, 7, residuals on odd / even / no positions, N = 232 and
225 inside a run, fp32 and bf16 tails, DHAUG_MLP_NOTAIL2 / DHAUG_MLP_NOSTACK), parking through STORE_BF16 / LOAD_BF16, stale
columns.  Every program runs at M = 1, 127, 128, 129, 300; one per family at M = 643 on two workgroups (three tiles each, the
ragged one last).

Tier 2 -- realistic values (normal weights / sqrt(K), normal inputs, slope 0.01, fp32 biases like 0.1 + 2^-13 that are no bf16
values), one unit per shape class at M = 129, against fp64 on the bf16 values the kernel consumed.  It catches what exact data
cannot: a bias rounded to bf16, a slope applied in the wrong precision, an accumulator that is not fp32.  Bounds, derived as in
tests/test_gpu_graph_mix.py:
  * fp32 output: the result is a sum of K products (exact in fp32: bf16 x bf16), the bias and the residual, K + 2 terms, each
    addition rounding by at most 2^-24 of a running sum that never exceeds S = sum|w||x| + |bias| + |res|: (K + 2) 2^-24 S.  The
    activation does not enlarge a difference (slopes <= 1; the slope's own rounding is 2^-24 of the value, inside the same sum);
  * bf16 output: one more rounding, half a unit in the last of 8 significant bits: at most 2^-8 of the value, 2^-8 |ref|;
  * DOT_OUT: the activations enter the dot product rounded to bf16, in the reference as in the kernel; the kernel's pre-activation
    lies within the fp32 bound e of the reference's, so its rounded activation lies between bf16(act(pre - e)) and
    bf16(act(pre + e)) (both monotone) and the dot product differs by at most sum |w2| (hi - lo); plus the fmaf roundings of the dot
    itself, 130 2^-24 (sum|a||w2| + |bias2|) for at most 128 products, the bias and the final additions.
A chain of several realistic bf16 layers has no clean bound (a flipped tie), so the stack, pair and pair-DOT_OUT classes run an
exact first layer and a realistic last one."""
import argparse
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

import mlp_unit_util as U

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


@pytest.mark.parametrize("name", [n for f in U.TIER1 for n in U.names(f)])
def test_exact_program(dhaug, name):
    p = U.get(name)
    dev = U.Device(p, dhaug)
    for M in U.MS:
        U.compare(p, dev.run(M), M)


@pytest.mark.parametrize("name", U.names("cap"))
def test_exact_program_three_tiles_per_workgroup(dhaug, name):
    """M = 128 * 5 + 3 under workgroup_cap(2): each persistent workgroup walks three tiles and takes the ragged one last"""
    p = U.get(name)
    assert p.cap == 2 and p.mmax == U.M_CAP
    U.compare(p, U.Device(p, dhaug).run(p.mmax), p.mmax)


@pytest.mark.parametrize("name", U.names("real"))
def test_realistic_unit_within_derived_bound(dhaug, name):
    p = U.get(name)
    U.compare(p, U.Device(p, dhaug).run(p.mmax), p.mmax, report=print)


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


@pytest.mark.parametrize("D", [64, 128, 256])
@pytest.mark.parametrize("kind", ["gen", "d2", "d3"])
def test_shipped_builders_exact(dhaug, kind, D):
    """fused.generator_head / critic2d (with its composed layer) / critic3d in "bf16" mode on modules that hold exact parameters,
    against the same programs written out unit by unit in mlp_unit_util: bit for bit at every width the builders accept"""
    from dhaug_amd import fused
    p = U.get("ship_%s_D%d" % (kind, D))
    mod = _module(dhaug, kind, D)
    params = dict(mod.named_parameters())
    with torch.no_grad():
        for k, v in p.sd.items():
            assert params[k].shape == v.shape, k
            params[k].copy_(torch.from_numpy(v).float())
    if kind == "d2":
        mod.slope = 0.25                                                      # a power of two: the slope multiplies exactly
    dev = {n: torch.from_numpy(T["data"]).float().cuda().to(torch.bfloat16 if T["dtype"] == "bf16" else torch.float32)
           for n, T in p.tensors.items() if T["data"] is not None}
    ref = torch.from_numpy(p.ref()["out"]["y"]).float()
    for M in U.MS:
        with torch.no_grad():
            if kind == "gen":
                got = fused.generator_head(mod, dev["z"][:M])
            elif kind == "d2":
                got = fused.critic2d(mod, dev["x"][:M])
            else:
                got = fused.critic3d(mod, dev["x"][:M], kcs=dev["kcs"][:M])
        assert got.shape == ref[:M].shape and torch.equal(got.cpu(), ref[:M]), (kind, D, M)


def test_device_packers_match_the_header_formula(dhaug):
    """dhaug_pack_wfrag against the numpy form of the header's formula, bit for bit, and dhaug_pack_wfrag_composed against its
    documented rule (fp64 sums, then fp32, then one rounding to bf16) -- on random factors to a neighbouring bf16 value where the
    fp64 sum sits on a tie (the exact factors of test_shipped_builders_exact leave no tie: there it is bit for bit)"""
    lib, ops = dhaug._lib, dhaug.ops
    vp = ctypes.c_void_p
    rng = np.random.default_rng(11)
    for N, K, k0, ldw in ((1, 8, 0, 8), (33, 72, 0, 72), (100, 100, 28, 128), (256, 256, 0, 256), (129, 40, 128, 168), (225, 200, 3, 210)):
        W = rng.standard_normal((N, ldw)).astype(np.float32)
        Wd = torch.from_numpy(W).cuda()
        ksteps = 4 * ((K + 63) // 64)
        blob = torch.full((8 * ksteps * 512 + 16,), 0x7FC0, dtype=torch.int16, device="cuda")
        lib.call("dhaug_pack_wfrag", vp(Wd.data_ptr()), ldw, vp(blob.data_ptr()), N, K, k0, ops._stream())
        got = blob.cpu().numpy().view(np.uint16)
        assert np.array_equal(got[:-16], U.pack_wfrag(W.astype(np.float64), K, k0)), (N, K, k0)
        assert (got[-16:] == 0x7FC0).all()
    for N, Ki, K, k0 in ((100, 256, 256, 0), (37, 100, 72, 8)):
        Wa, Wb = rng.standard_normal((N, Ki)).astype(np.float32), rng.standard_normal((Ki, k0 + K)).astype(np.float32)
        ba, bb = rng.standard_normal(N).astype(np.float32), rng.standard_normal(Ki).astype(np.float32)
        d = [torch.from_numpy(a).cuda() for a in (Wa, ba, Wb, bb)]
        ksteps = 4 * ((K + 63) // 64)
        blob = torch.full((8 * ksteps * 512,), 0x7FC0, dtype=torch.int16, device="cuda")
        bias = torch.full((256,), float("nan"), device="cuda")
        lib.call("dhaug_pack_wfrag_composed", vp(d[0].data_ptr()), Ki, vp(d[1].data_ptr()), vp(d[2].data_ptr()), k0 + K, vp(d[3].data_ptr()),
                 vp(blob.data_ptr()), vp(bias.data_ptr()), N, Ki, K, k0, ops._stream())
        W, b = U.composed_weights(Wa.astype(np.float64), ba.astype(np.float64), Wb.astype(np.float64)[:, k0:], bb.astype(np.float64))
        # the device sums in the order m = 0 .. Ki-1 in fp64; numpy's order differs by far less than the fp32 rounding that
        # follows, but a sum within that of an fp32 tie may round the other way: compare through the weights' bf16 neighbours
        got = (blob.cpu().numpy().view(np.uint16).astype(np.uint32) << 16).view(np.float32).astype(np.float64)
        want = (U.pack_wfrag(W, K, 0).astype(np.uint32) << 16).view(np.float32).astype(np.float64)
        assert np.mean(got == want) > 0.9999 and np.all(np.abs(got - want) <= 2.0 ** -7 * np.abs(want))
        bg = bias.cpu().numpy().astype(np.float64)
        assert np.all(bg[N:] == 0) and np.all(np.abs(bg[:N] - b) <= 2.0 ** -23 * np.abs(b))
