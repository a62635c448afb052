"""GPU tests of the inverse-kinematics public surface: ops.fk_jacobian / ik_fit / ik_track, Forward_Kinematics_DH_Model.fit_pose /
fit_sequences and unpack_angles.  The kernels themselves are tested through the C-ABI in tests/test_gpu_ik_kernels.py; here it is
shapes, types, the limit tables, numpy inputs, the round trip through the reference's own keyword interface and the refusals."""
import argparse

import numpy as np
import pytest
import torch

import ik_util as K

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def M():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import dhaug_amd
    dhaug_amd._lib.lib()
    from dhaug_amd import ops
    from dhaug_amd.models_Fk_GAN import forward_kinematics_DH_model as fkm
    args = argparse.Namespace(batch_size=3, random_seed=0, single_or_multi_train_mode="single", architecture="3,3,3")
    return argparse.Namespace(ops=ops, fkm=fkm, fk=fkm.Forward_Kinematics_DH_Model(args, ["S1"], None), lib=dhaug_amd._lib)


@pytest.fixture(scope="module")
def batch():
    return K.trial_fit_inputs(96)


def test_fit_pose_round_trip(M, batch):
    """fit_pose returns the named tuple of device tensors, and change_3d_joint_angle(**unpack_angles(...)) -- the reference's
    keyword interface -- rebuilds every converged pose within 1e-4 m"""
    pose, init = batch["pose"].cuda(), batch["init"].cuda()
    fit = M.fk.fit_pose(pose, init=init, iters=12)
    assert type(fit).__name__ == "IkFit" and fit._fields == ("angles37", "bone_len", "root", "residual")
    assert [tuple(t.shape) for t in fit] == [(96, 37), (96, 15), (96, 3), (96,)]
    assert all(t.is_cuda and t.dtype == torch.float32 for t in fit)
    ok = fit.residual <= K.CONVERGED_M
    assert int((~ok).sum()) <= 0.005 * 96                                   # the kernel tests' cap
    out32 = M.fk.change_3d_joint_angle(**M.fkm.unpack_angles(fit.angles37), **M.fkm.bone_len_kwargs(fit.bone_len),
                                       root_3d_pos=fit.root)
    back = out32[:, M.fkm.H36M_32_To_16_Table]
    assert (back - pose).norm(dim=2).max(dim=1).values[ok].max().item() <= 1e-4
    # any leading shape that views as (..., 16, 3); default start = T-pose, default 20 steps
    cold = M.fk.fit_pose(pose.reshape(4, 24, 16, 3))
    assert tuple(cold.angles37.shape) == (96, 37) and bool(torch.isfinite(cold.residual).all())
    print("FIGURE cold start from the T-pose, 20 steps, 96 poses: %d not converged (not gated)" % int((cold.residual > K.CONVERGED_M).sum()))


def test_fit_pose_limits_normal_and_pair(M, batch):
    pose, truth = batch["pose"].cuda(), batch["truth"]
    lo, hi = M.fk.ik_limits("normal")
    assert len(lo) == 37 and len(hi) == 37 and all(a <= b for a, b in zip(lo, hi))
    assert (lo[34], hi[34], lo[36], hi[36]) == (-20.0, 20.0, -180.0, 180.0) and (lo[23], hi[23], lo[33], hi[33]) == (0, 0, 0, 0)
    assert lo[:3] == [-90.0, -90.0, -45.0] and hi[:3] == [45.0, 45.0, 120.0]
    fit = M.fk.fit_pose(pose, iters=6, limits="normal")
    lo_t, hi_t = torch.tensor(lo).cuda(), torch.tensor(hi).cuda()
    assert bool((fit.angles37 >= lo_t).all() and (fit.angles37 <= hi_t).all()) and bool(torch.isfinite(fit.residual).all())
    # a (lo, hi) pair: the generator's own tables give the bits of the default
    a = M.fk.fit_pose(pose, init=batch["init"].cuda(), iters=3, limits=(M.ops.IK_GENERATOR_LO, M.ops.IK_GENERATOR_HI))
    b = M.fk.fit_pose(pose, init=batch["init"].cuda(), iters=3)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    with pytest.raises(ValueError):
        M.fk.fit_pose(pose, limits="tight")


def test_numpy_inputs_and_sequences(M):
    d = K.trial_track_inputs(5, [6, 1, 4, 3, 2])
    off, pose = d["offsets"], d["pose"]
    seqs = [pose[off[s]:off[s + 1]].numpy() for s in range(5)]
    got = M.fk.fit_sequences(seqs, init=d["init"].numpy(), iters=8)
    assert [tuple(t.shape) for t in got] == [(16, 37), (16, 15), (16, 3), (16,)] and all(t.is_cuda for t in got)
    assert int((got.residual > K.CONVERGED_M).sum()) == 0
    # one concatenated device tensor with lengths, and a list of device tensors: the same bits
    for other in (M.fk.fit_sequences(pose.cuda(), [6, 1, 4, 3, 2], init=d["init"].cuda(), iters=8),
                  M.fk.fit_sequences([torch.from_numpy(q).cuda() for q in seqs], init=d["init"].cuda(), iters=8)):
        assert all(torch.equal(x, y) for x, y in zip(got, other))
    one = M.fk.fit_pose(seqs[0], init=d["init"][:1].numpy().repeat(6, 0), iters=8)         # numpy poses and start
    assert torch.equal(one.angles37[0], got.angles37[0])
    J = M.ops.fk_jacobian(got.angles37, got.bone_len)
    assert tuple(J.shape) == (16, 48, 37) and bool((J[:, :, K.DEAD] == 0).all())


def test_refusals_raise_before_any_launch(M, batch):
    pose, init = batch["pose"][:8].cuda(), batch["init"][:8].cuda()
    calls = M.lib.CALLS[0]
    lo, hi = list(M.ops.IK_GENERATOR_LO), list(M.ops.IK_GENERATOR_HI)
    bad_lo = list(lo)
    bad_lo[2] = hi[2] + 1.0
    outside = init.clone()
    outside[3, 0] = hi[0] + 1.0
    for fn in (lambda: M.ops.ik_fit(pose.reshape(8, 48)), lambda: M.ops.ik_fit(pose[:, :15]),
               lambda: M.ops.ik_fit(pose, lo=bad_lo, hi=hi), lambda: M.ops.ik_fit(pose, lo=lo), lambda: M.ops.ik_fit(pose, iters=0),
               lambda: M.ops.ik_fit(pose, init=outside), lambda: M.ops.ik_fit(pose, init=init[:7]),
               lambda: M.ops.ik_track(pose, [0, 4, 4, 8]), lambda: M.ops.ik_track(pose, [0, 5, 3, 8]),
               lambda: M.ops.ik_track(pose, [0, 4, 9]), lambda: M.ops.ik_track(pose, [1, 8]),
               lambda: M.ops.ik_track(pose, [0, 8], iters=0), lambda: M.ops.ik_track(pose, [0, 4, 8], init=outside[:2] + 500.0),
               lambda: M.fk.fit_sequences(pose, None), lambda: M.fk.fit_sequences(pose, [8, 0])):
        with pytest.raises(ValueError):
            fn()
    assert M.lib.CALLS[0] == calls, "a refused call reached the library"
    for fn in (lambda: M.ops.ik_fit(pose.cpu()), lambda: M.ops.ik_track(pose.cpu(), [0, 8]),
               lambda: M.ops.fk_jacobian(init.cpu(), torch.zeros(8, 15))):
        with pytest.raises(RuntimeError):
            fn()
    assert M.lib.CALLS[0] == calls
    # clamp_init=True takes the start that was refused
    fit = M.ops.ik_fit(pose, init=outside, iters=2, clamp_init=True)
    assert bool((fit.angles37[:, 0] <= hi[0]).all())


def test_golden_poses_do_not_get_worse(M, golden):
    """tests/golden/fk_N8.npz: poses of the full +-180 degree model (slots 23 and 28 among them, which no fit can use), fitted from
    their own recorded angles clamped to the generator's limits: accept / reject never lets the cost rise"""
    g = golden("fk_N8")
    pose = g["out32"][:, M.fkm.H36M_32_To_16_Table].contiguous()
    start = torch.minimum(torch.maximum(g["angles"].double(), K.LO), K.HI)
    start[:, K.DEAD] = 0.0
    fit = M.fk.fit_pose(pose.cuda(), init=g["angles"].cuda(), iters=20, clamp_init=True)
    c0 = K.cost64(start, fit.bone_len.cpu(), fit.root.cpu(), pose)
    c1 = K.cost64(fit.angles37.cpu(), fit.bone_len.cpu(), fit.root.cpu(), pose)
    print("FIGURE golden fk_N8: cost %s -> %s" % (np.round(c0.numpy(), 4), np.round(c1.numpy(), 4)))
    assert bool((c1 <= c0 + 2 * c0.sqrt() * (45 ** 0.5) * 1e-5 + 1e-10).all())         # (fp32 FK error on both costs, as in the kernel tests)
    with pytest.raises(ValueError):
        M.fk.fit_pose(pose.cuda(), init=g["angles"].cuda())                           # not clamped: refused
