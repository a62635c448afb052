"""Inverse kinematics without a GPU: the packing helpers, the refusals that need no device, the fp64 restatement of the solver
(tests/ik_util.py) on the trial's inputs, and the per-pose arithmetic of csrc/dhaug_ik_math.h compiled for the host as a stand-alone
program under AddressSanitizer + UBSan (tests/ikcheck)."""
import argparse
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import ik_util as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def pkg():
    import dhaug_amd
    from dhaug_amd import ops
    from dhaug_amd.models_Fk_GAN import forward_kinematics_DH_model as fkm
    return argparse.Namespace(ops=ops, fkm=fkm, lib=dhaug_amd._lib)


def test_unpack_angles_inverts_pack_angles(pkg):
    g = torch.Generator().manual_seed(1)
    parts = [torch.randn(7, n, generator=g) for n in (5, 5, 13, 5, 5, 3)]
    a = pkg.fkm.pack_angles(*parts)
    kw = pkg.fkm.unpack_angles(a)
    assert list(kw) == ["right_leg_joints_angle", "left_leg_joints_angle", "body_joints_angle", "right_hand_joints_angle",
                        "left_hand_joints_angle", "generator_global_rot_3d_pos_angle"]
    assert all(torch.equal(x, y) for x, y in zip(kw.values(), parts))
    again = pkg.fkm.pack_angles(kw["right_leg_joints_angle"], kw["left_leg_joints_angle"], kw["body_joints_angle"],
                                kw["right_hand_joints_angle"], kw["left_hand_joints_angle"], kw["generator_global_rot_3d_pos_angle"])
    assert torch.equal(again, a)
    b = torch.rand(7, 15, generator=g)
    assert list(pkg.fkm.bone_len_kwargs(b)) == pkg.fkm._BONE_KW and torch.equal(pkg.fkm.bone_len_kwargs(b)["neck_len"], b[:, 14])


def test_tables_agree(pkg):
    """the binding's copy of the generator's limits = the oracle's; the header's grid caps = the binding's mirror; the kernel's eps
    and lambda constants = the restatement's"""
    from oracle import dhaug_oracle as O
    assert pkg.ops.IK_GENERATOR_LO == O.ANGLE_LO and pkg.ops.IK_GENERATOR_HI == O.ANGLE_HI
    assert tuple(pkg.ops.IK_DEAD_SLOTS) == tuple(O.ZERO_SLOTS)
    hdr = open(os.path.join(ROOT, "include", "dhaug.h")).read()
    define = lambda n: int(re.search(r"#define\s+%s\s+(\d+)" % n, hdr).group(1))
    assert define("DHAUG_IK_MAX_BLOCKS") == pkg.lib.IK_MAX_BLOCKS and define("DHAUG_FK_JACOBIAN_MAX_BLOCKS") == pkg.lib.FK_JACOBIAN_MAX_BLOCKS
    src = open(os.path.join(os.path.dirname(pkg.lib.__file__), "csrc", "dhaug_ik_math.h")).read()
    assert "kEpsDiag = 1e-8f" in src and K.EPS_DIAG == 1e-8
    assert "kLamMin = 1e-9f, kLamMax = 1e6f, kLamDown = 0.3f, kLamUp = 5.0f" in src
    assert (K.LAM_MIN, K.LAM_MAX, K.LAM_DOWN, K.LAM_UP) == (1e-9, 1e6, 0.3, 5.0)


def test_refusals_without_a_device(pkg):
    pose = torch.zeros(4, 16, 3)
    lo, hi = list(pkg.ops.IK_GENERATOR_LO), list(pkg.ops.IK_GENERATOR_HI)
    bad = list(lo)
    bad[36] = 181.0
    for fn in (lambda: pkg.ops.ik_fit(torch.zeros(4, 48)), lambda: pkg.ops.ik_fit(torch.zeros(4, 17, 3)),
               lambda: pkg.ops.ik_fit(pose, iters=0), lambda: pkg.ops.ik_fit(pose, lo=bad, hi=hi), lambda: pkg.ops.ik_fit(pose, hi=hi),
               lambda: pkg.ops.ik_fit(pose, lo=lo[:36], hi=hi), lambda: pkg.ops.ik_fit(pose, lambda0=0.0),
               lambda: pkg.ops.ik_track(pose, [0, 2, 2, 4]), lambda: pkg.ops.ik_track(pose, [0, 3, 2, 4]),
               lambda: pkg.ops.ik_track(pose, [0, 5]), lambda: pkg.ops.ik_track(pose, [0, 4], iters=-1),
               lambda: pkg.ops.ik_track(torch.zeros(4, 16, 2), [0, 4])):
        with pytest.raises(ValueError):
            fn()
    # what passes the host checks then asks for a GPU tensor, as every op does
    for fn in (lambda: pkg.ops.ik_fit(pose), lambda: pkg.ops.ik_track(pose, [0, 1, 4]),
               lambda: pkg.ops.fk_jacobian(torch.zeros(4, 37), torch.zeros(4, 15))):
        with pytest.raises(RuntimeError, match="needs a GPU tensor"):
            fn()
    fk = pkg.fkm.Forward_Kinematics_DH_Model(argparse.Namespace(batch_size=2, random_seed=0), ["S1"], None)
    lo_n, hi_n = fk.ik_limits("normal")
    assert len(lo_n) == 37 and all(a <= b for a, b in zip(lo_n, hi_n)) and (lo_n[35], hi_n[35]) == (-20.0, 20.0)
    assert all(lo_n[s] == 0 and hi_n[s] == 0 for s in K.DEAD)
    with pytest.raises(ValueError):
        fk.ik_limits("none")
    with pytest.raises(ValueError):
        fk.fit_sequences(pose, None)


def test_restatement_meets_both_caps():
    """the caps the GPU tests hold the kernels to, met by the fp64 restatement on the trial's inputs: warm start, 512 poses, 12 steps,
    at most 0.5 % not converged; tracking, 128 sequences of 24 frames, 8 steps per frame, at most 1 % of the frames"""
    d = K.trial_fit_inputs(512)
    ang, bl, root, res = K.lm_fit(d["pose"], d["init"], iters=12)
    err = K.joint_error(ang, bl, root, d["pose"])
    print("FIGURE restatement, warm start: %d of 512 not converged, error median %.3g max %.3g m" % (K.not_converged(err), err.median(), err.max()))
    assert K.not_converged(err) <= 0.005 * 512
    assert (res - err).abs().max().item() <= 1e-12
    assert bool((ang >= K.LO).all() and (ang <= K.HI).all() and (ang[:, K.DEAD] == 0).all())
    t = K.trial_track_inputs(128)
    ang, bl, root, res = K.lm_track(t["pose"], t["offsets"], t["init"], iters=8)
    err = K.joint_error(ang, bl, root, t["pose"])
    print("FIGURE restatement, tracking: %d of %d frames not converged, error median %.3g max %.3g m"
          % (K.not_converged(err), len(err), err.median(), err.max()))
    assert len(err) == 3072 and K.not_converged(err) <= 0.01 * 3072


def test_jacobian_by_autograd_is_a_derivative():
    """ik_util.jacobian64 against a central difference of the oracle's FK (the reference of the GPU tests is itself checked once)"""
    g = torch.Generator().manual_seed(3)
    a, bl = K.trial_angles(3, g), K.trial_lengths(3, g)
    J = K.jacobian64(a, bl)
    h = 1e-4
    for s in (0, 12, 23, 26, 27, 36):
        e = torch.zeros(37, dtype=K.F64)
        e[s] = h
        z = torch.zeros(3, 3)
        fd = (K.fk64(a.double() + e, bl, z) - K.fk64(a.double() - e, bl, z)).reshape(3, 48) / (2 * h)
        assert (fd - J[:, :, s]).abs().max().item() <= 1e-9
    assert bool((J[:, :, K.STILL + [4, 9, 22, 33]] == 0).all())


def test_host_program_under_sanitizers(tmp_path):
    """tests/ikcheck: dhaug_ik_math.h compiled for the host with -fsanitize=address,undefined as a program of its own; it fits 64
    warm-started poses, every one converges by its own residual and by the fp64 FK of what it returns, and it exits clean"""
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    exe = ge.build_ikcheck_sanitized(verbose=False)
    out = str(tmp_path / "ikcheck_out.bin")
    r = subprocess.run([exe, "64", out], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
    assert r.returncode == 0, r.stderr[-3000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
    res = [float(m) for m in re.findall(r"^pose \d+ residual (\S+)$", r.stdout, flags=re.M)]
    assert len(res) == 64 and max(res) <= K.CONVERGED_M, max(res)
    N = 64
    raw = np.fromfile(out, dtype=np.float32)
    parts, at = [], 0
    for w in (37, 15, 48, 37, 37, 15, 3, 1, 48 * 37):
        parts.append(torch.from_numpy(raw[at:at + N * w].reshape(N, w).copy()))
        at += N * w
    assert at == raw.size
    truth, length, pose, init, ang, bl, root, residual, J = parts
    err = K.joint_error(ang, bl, root, pose)
    assert K.not_converged(err) == 0 and (residual.reshape(-1).double() - err).abs().max().item() <= 1e-5
    assert bool((ang[:, K.DEAD] == 0).all()) and torch.equal(root, pose[:, :3])
    ref = K.jacobian64(truth, length)
    J = J.reshape(N, 48, 37).double()
    assert (J[:, :, K.LIVE] - ref[:, :, K.LIVE]).abs().max().item() <= K.JAC_TOL and bool((J[:, :, K.DEAD + K.STILL] == 0).all())
