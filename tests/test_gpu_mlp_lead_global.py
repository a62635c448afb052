"""GPU tests of the route "stack with its lead operand from global memory" of dhaug_mlp_forward (csrc/dhaug_mlp.hip, PLAN_LEADG):
a bf16 LOAD of 32 / 48 columns and the stack whose lead layer it feeds run as one unit, and every lane reads its MFMA B fragments
(16 aligned bytes of one row) from the tensor itself through a buffer resource over the tile's rows.

Tier-1 exact programs of tests/mlp_lead_util.py against the fp64 reference of tests/mlp_unit_util.py, torch.equal (the exactness
condition is asserted by tests/test_mlp_plan_cpu.py, which also proves through dhaug_mlp_plan that the programs called "fused"
here take the new route and the "refused" ones do not: an in-place residual from the LOAD's buffer, a program that parks rows, a
second consumer of the image, a first run layer that reads the LOAD's buffer as its source).  Sizes: M = 1, 31, 33, 127, 128, 129, 300 and one program at M = 643 on
two workgroups (three tiles each, the ragged one last).  Every program runs with ld == cols and with ld = cols + 8, with the route
on and with DHAUG_MLP_NOLEADG set: both results equal the reference and each other bit for bit.

What an over-read would show: every input of a launch over M rows lies in a NaN-filled allocation that holds exactly its M rows,
with 16 NaN elements in front, behind each row's columns (ld > cols) and behind row M - 1 -- a fragment load that reaches past
a row, past the tile or past row M - 1 multiplies a NaN into a result (0 * NaN is NaN on the matrix unit).  Every output lies in
a NaN-filled tensor that is longer and wider than what the program writes; the rest must stay NaN."""
import argparse
import os
import sys

import pytest
import torch

import mlp_lead_util as LG
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


class GuardedDevice(U.Device):
    """U.Device whose inputs, per launch, are the first M rows alone inside NaN"""

    def run(self, M):
        torch_ = self.torch
        whole = self.inputs
        self.inputs = {}
        try:
            for name, buf in whole.items():
                T = self.p.tensors[name]
                ld, w = T["ld"], T["width"]
                flat = torch_.full((LG.GUARD + M * ld + LG.GUARD,), float("nan"), dtype=buf.dtype, device="cuda")
                rows = torch_.as_strided(flat, (M, ld), (ld, 1), LG.GUARD)
                rows[:, :w] = buf[:M, :w]
                assert rows.data_ptr() % 16 == 0 and rows.stride(0) == ld
                self.inputs[name] = rows
            return super().run(M)
        finally:
            self.inputs = whole


def _bits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _on_off(p, dev, M):
    with LG.route(True):
        on = dev.run(M)
    with LG.route(False):
        off = dev.run(M)
    U.compare(p, on, M)
    U.compare(p, off, M)
    assert on.keys() == off.keys()
    for name in on:                                                           # NaN filling included
        assert torch.equal(_bits(on[name]), _bits(off[name])), (p.name, M, name)


CASES = [(n, LG.FUSED[n][0]) for n in sorted(LG.FUSED)] + [("refused_" + n, LG.REFUSED[n]) for n in sorted(LG.REFUSED)]


@pytest.mark.parametrize("lde", [0, 8])
@pytest.mark.parametrize("name,build", CASES, ids=[c[0] for c in CASES])
def test_exact_program_route_on_and_off(dhaug, name, build, lde):
    p = LG.get(build, lde)
    dev = GuardedDevice(p, dhaug)
    for M in LG.MS:
        _on_off(p, dev, M)


@pytest.mark.parametrize("lde", [0, 8])
def test_three_tiles_per_workgroup(dhaug, lde):
    """M = 128 * 5 + 3 under workgroup_cap(2): the resource of every tile starts at that tile's rows, the last one is ragged"""
    p = LG.get(LG.d3_cap, lde)
    assert p.cap == 2 and p.mmax == U.M_CAP
    _on_off(p, GuardedDevice(p, dhaug), p.mmax)


def test_empty_batch_is_a_no_op(dhaug):
    """an empty tensor's pointer is null: dhaug_mlp_forward looks at no unit when M = 0"""
    from dhaug_amd import fused
    D3m, D2m = _module("d3", 256), _module("d2", 256)
    e = lambda w: torch.empty((0, w), dtype=torch.bfloat16, device="cuda")
    with torch.no_grad():
        o3, o2 = fused.critics(D3m, D2m, e(48), e(32), e(32))
    assert o3.shape == (0, 1) and o2.shape == (0, 1)


def _module(kind, D):
    from dhaug_amd.models_Fk_GAN import Fk_discriminator
    args = argparse.Namespace(batch_size=64, random_seed=0, GAN_OUTPUT_DIM=35, GAN_LAMBDA=10, GAN_whether_use_preAngle=True,
                              Gen_DenseDim=D, Dis_DenseDim_3D=D, Dis_DenseDim_2D=D, video_Dis_DenseDim_3D=32,
                              video_Dis_DenseDim_2D=32, GAN_3d_loss_weight=1.0, GAN_2d_loss_weight=0.2, bone_len_scaler="different",
                              whether_use_RT=True, flip_GAN_model_input=True, single_or_multi_train_mode="single",
                              architecture="3,3,3", motion_Dis_whether_use_3dPos_branch=True,
                              motion_Dis_whether_use_3dDiff_branch=True)
    if kind == "d3":
        return Fk_discriminator.Fk_3D_Discriminator("cuda", args).cuda()
    return Fk_discriminator.Fk_2D_Discriminator(args, 16).cuda()


def test_module_critics_route_on_equals_off(dhaug):
    """fused.critics on the modules' own programs, bf16 inputs as Fk_Generator.sample_for_critics hands them over: the planner
    takes the route at all three places (asked for the very units of the launch), and the logits do not change by a bit"""
    import ctypes
    from dhaug_amd import fused, _lib
    torch.manual_seed(3)
    D3m, D2m = _module("d3", 256), _module("d2", 256)
    for M in (300, 129):
        x3 = (0.3 * torch.randn(M, 48, device="cuda")).to(torch.bfloat16)
        kcs = torch.randn(M, 32, device="cuda").to(torch.bfloat16)
        x2 = (0.3 * torch.randn(M, 32, device="cuda")).to(torch.bfloat16)
        with torch.no_grad():
            u3, _ = fused.D3["program"](D3m, fused._net(D3m, fused.D3, "bf16")._fresh(), dict(x=x3, kcs=kcs), M)
            u2, _ = fused.D2["program"](D2m, fused._net(D2m, fused.D2, "bf16")._fresh(), dict(x=x2), M)
            units = u3 + u2
            arr = (_lib.MlpUnit * len(units))(*units)
            out = (ctypes.c_int32 * len(units))()
            got = {}
            for on in (True, False):
                with LG.route(on):
                    assert _lib.lib().dhaug_mlp_plan(arr, len(units), M, out) == 0
                    places = [i for i, w in enumerate(out) if units[i].kind == fused.LOAD_BF16 and (w & LG.PLAN_LEADG)]
                    assert places == ([0, 9, len(u3)] if on else [])
                    got[on] = fused.critics(D3m, D2m, x3, kcs, x2)
            torch.cuda.synchronize()
        for a, b in zip(got[True], got[False]):
            assert a.shape == (M, 1) and torch.isfinite(a).all() and torch.equal(a, b)
            assert a.float().std() > 0
