"""The staged, joint-weighted inverse-kinematics fit without a GPU: the refusals that need no device, the recorded fp64 restatement
(tests/ik_staged_util.py, tests/golden/ik_staged.npz) and the per-pose arithmetic of csrc/dhaug_ik_math.h compiled for the host as a
second stand-alone program under AddressSanitizer + UBSan (tests/ikcheck/ikcheck_staged_main.hip)."""
import argparse
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import ik_util as K
import ik_staged_util as KS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def pkg():
    import dhaug_amd
    from dhaug_amd import ops
    from dhaug_amd.models_Fk_GAN import forward_kinematics_DH_model as fkm
    fk = fkm.Forward_Kinematics_DH_Model(argparse.Namespace(batch_size=2, random_seed=0), ["S1"], None)
    return argparse.Namespace(ops=ops, fkm=fkm, fk=fk, lib=dhaug_amd._lib)


def test_schedule_tables_agree(pkg):
    """ops.IK_COARSE_TO_FINE = the restatement's schedule = the recorded one; the binding knows the entry; the stage cap is the header's"""
    sched = pkg.ops.IK_COARSE_TO_FINE
    assert [(list(w), n) for w, n in sched] == KS.COARSE_TO_FINE
    assert sum(n for _, n in sched) == 40 and [int(sum(w)) for w, _ in sched] == [3, 6, 11, 16]
    g = KS.load_golden()
    assert np.array_equal(g["schedule_w"], np.array([w for w, _ in sched])) and list(g["schedule_iters"]) == [n for _, n in sched]
    assert len(pkg.lib.SIGNATURES["dhaug_ik_fit_staged"]) == 15
    src = open(os.path.join(os.path.dirname(pkg.lib.__file__), "csrc", "dhaug_ik_math.h")).read()
    assert "MAX_STAGES = %d;" % pkg.ops.IK_MAX_STAGES in src
    hdr = open(os.path.join(ROOT, "include", "dhaug.h")).read()
    assert "int dhaug_ik_fit_staged(" in hdr


def test_staged_refusals_without_a_device(pkg):
    """every case the entry refuses is a ValueError on the host, before a device is asked for"""
    pose = torch.zeros(4, 16, 3)
    ones, zeros = [1.0] * 16, [0.0] * 16
    root_only = [1.0] + [0.0] * 15
    nan = ones[:5] + [float("nan")] + ones[6:]
    staged = pkg.ops.ik_fit_staged
    for what, fn in (
            ("no stage", lambda: staged(pose, [], [])),
            ("nine stages", lambda: staged(pose, [ones] * 9, [1] * 9)),
            ("a step count of 0", lambda: staged(pose, [ones, ones], [4, 0])),
            ("a negative step count", lambda: staged(pose, [ones], [-1])),
            ("a negative weight", lambda: staged(pose, [ones[:3] + [-0.5] + ones[4:]], [4])),
            ("a NaN weight", lambda: staged(pose, [nan], [4])),
            ("an infinite weight", lambda: staged(pose, [ones[:15] + [float("inf")]], [4])),
            ("a weight whose square overflows fp32", lambda: staged(pose, [ones[:15] + [1e30]], [4])),
            ("a last stage of zeros", lambda: staged(pose, [ones, zeros], [4, 4])),
            ("a last stage with the root's weight only", lambda: staged(pose, [ones, root_only], [4, 4])),
            ("15 weights", lambda: staged(pose, [ones[:15]], [4])),
            ("more step counts than stages", lambda: staged(pose, [ones], [4, 4])),
            ("lambda0 = 0", lambda: staged(pose, [ones], [4], lambda0=0.0)),
            ("only lo", lambda: staged(pose, [ones], [4], lo=list(pkg.ops.IK_GENERATOR_LO))),
            ("a bad shape", lambda: staged(torch.zeros(4, 48), [ones], [4])),
            ("an unknown schedule", lambda: pkg.fk.fit_pose(pose, schedule="fine_to_coarse")),
            ("a schedule of bare rows", lambda: pkg.fk.fit_pose(pose, schedule=[ones, ones])),
            ("a schedule and weights", lambda: pkg.fk.fit_pose(pose, schedule="coarse_to_fine", joint_weights=ones)),
            ("bone_len without weights", lambda: pkg.fk.fit_pose(pose, bone_len=torch.ones(4, 15))),
            ("zero weights alone", lambda: pkg.fk.fit_pose(pose, joint_weights=zeros)),
            ("weights with iters = 0", lambda: pkg.fk.fit_pose(pose, joint_weights=ones, iters=0))):
        with pytest.raises(ValueError):
            fn()
            pytest.fail("not refused: " + what)
    # what passes the host checks then asks for a GPU tensor, as every op does
    for fn in (lambda: staged(pose, [ones], [4]), lambda: staged(pose, *zip(*pkg.ops.IK_COARSE_TO_FINE)),
               lambda: staged(pose, torch.ones(2, 16), torch.tensor([3, 5])),
               lambda: pkg.fk.fit_pose(pose, schedule="coarse_to_fine"), lambda: pkg.fk.fit_pose(pose, joint_weights=ones),
               lambda: pkg.fk.fit_sequences(pose, [1, 3], cold_start=True)):
        with pytest.raises(RuntimeError, match="needs a GPU tensor"):
            fn()


def test_fit_pose_without_new_arguments_calls_the_old_op(pkg, monkeypatch):
    """fit_pose / fit_sequences with none of the new arguments make exactly the call they made before; the new ones select the staged op"""
    seen = []
    monkeypatch.setattr(pkg.ops, "ik_fit", lambda *a, **k: seen.append(("ik_fit", a, k)) or "fit")
    monkeypatch.setattr(pkg.ops, "ik_track", lambda *a, **k: seen.append(("ik_track", a, k)) or "track")
    monkeypatch.setattr(pkg.ops, "ik_fit_staged", lambda *a, **k: seen.append(("ik_fit_staged", a, k)) or "staged")
    pose, init = torch.zeros(4, 16, 3), torch.zeros(4, 37)
    lo, hi = pkg.fk.ik_limits("generator")
    assert pkg.fk.fit_pose(pose, init=init, iters=7, clamp_init=True) == "fit"
    name, a, k = seen.pop()
    assert name == "ik_fit" and a[0] is pose and a[1] is init and list(a[2:]) == [lo, hi] and k == {"iters": 7, "clamp_init": True} and not seen
    assert pkg.fk.fit_sequences(pose, [1, 3], init=init[:2]) == "track"
    name, a, k = seen.pop()
    assert name == "ik_track" and a[0] is pose and a[1] == [0, 1, 4] and torch.equal(a[2], init[:2]) and list(a[3:]) == [lo, hi]
    assert k == {"iters": 8, "clamp_init": False} and not seen
    assert pkg.fk.fit_sequences(pose, [1, 3], init=init[:2], cold_start=True) == "track" and seen.pop()[0] == "ik_track" and not seen
    assert pkg.fk.fit_pose(pose, schedule="coarse_to_fine") == "staged"
    name, a, k = seen.pop()
    assert name == "ik_fit_staged" and [list(w) for w in a[1]] == [w for w, _ in KS.COARSE_TO_FINE] and list(a[2]) == [8, 8, 8, 16]
    w = [0.5] * 16
    assert pkg.fk.fit_pose(pose, joint_weights=w, iters=9) == "staged"
    name, a, k = seen.pop()
    assert name == "ik_fit_staged" and a[1] == [w] and a[2] == [9]
    assert pkg.fk.fit_pose(pose, schedule=[(w, 2), ([1.0] * 16, 3)]) == "staged"
    name, a, k = seen.pop()
    assert a[1] == [w, [1.0] * 16] and a[2] == [2, 3]


def test_restatement_equals_its_recording():
    """tests/golden/ik_staged.npz was made by tests/golden/make_ik_staged.py from this restatement: the first 32 poses recomputed.  fp64
    throughout, so the two differ by rounding in another order of summation at the most: 1e-9 m is a thousand times what 40 steps
    of 1e-16 relative error reach and ten thousand times below CONVERGED_M"""
    g = KS.load_golden()
    assert g["err"].shape == (KS.GOLDEN_POSES,) and int(g["not_converged"]) == int((g["err"] > K.CONVERGED_M).sum())
    err = KS.cold_errors(32).numpy()
    print("FIGURE restatement, cold, staged: recorded R = %d of %d (single stage of 40 steps: %d); first 32 recomputed: largest "
          "difference %.3g m" % (int(g["not_converged"]), KS.GOLDEN_POSES, int((g["single_err"] > K.CONVERGED_M).sum()),
                                 np.abs(err - g["err"][:32]).max()))
    assert np.abs(err - g["err"][:32]).max() <= 1e-9
    assert np.array_equal(err > K.CONVERGED_M, g["err"][:32] > K.CONVERGED_M)
    # the recording itself says what the schedule is for: it leaves less than a tenth of what one stage of 40 steps leaves
    assert 10 * int(g["not_converged"]) <= int((g["single_err"] > K.CONVERGED_M).sum())


def test_weighted_restatement_with_ones_is_the_plain_one():
    """one stage of weights 1: ik_util.lm_fit to the last bit of what both return (the same operations on the same numbers)"""
    d = K.trial_fit_inputs(16)
    a = K.lm_fit(d["pose"], d["init"], iters=6)
    b = KS.lm_fit_staged(d["pose"], [([1.0] * 16, 6)], init=d["init"])
    assert all(torch.equal(x, y) for x, y in zip(a, b))


def test_staged_host_program_under_sanitizers(tmp_path):
    """tests/ikcheck/ikcheck_staged_main.hip: dhaug_ik_math.h compiled for the host with -fsanitize=address,undefined as a program of
    its own; it fits 64 poses cold by the coarse-to-fine schedule and exits clean.  Its cost decisions are the
    restatement's: in every stage, from the program's own angles at that stage's start, the weighted fp64 cost where the program
    stops is no higher than where the restatement stops, nor than the start's, within the allowance 2 sqrt(cost) sqrt(45) 1e-5 of the
    fp32 FK's error on both costs (cost = the stage start's, as in tests/test_gpu_ik_kernels.py::exact_properties)."""
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    exe = ge.build_ikcheck_staged_sanitized(verbose=False)
    out = str(tmp_path / "ikcheck_staged_out.bin")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, "64", out], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
    printed = [float(m) for m in re.findall(r"^pose \d+ residual (\S+)$", r.stdout, flags=re.M)]
    N, S = 64, 4
    raw = np.fromfile(out, dtype=np.float32)
    parts, at = [], 0
    for n, w in ((N, 37), (N, 15), (N, 48), (S, 16), (N, S * 37), (N, 37), (N, 15), (N, 3), (N, 1)):
        parts.append(torch.from_numpy(raw[at:at + n * w].reshape(n, w).copy()))
        at += n * w
    assert at == raw.size
    truth, length, pose, weights, stage_ang, ang, bl, root, residual = parts
    stage_ang = stage_ang.reshape(N, S, 37)
    assert weights.tolist() == [w for w, _ in KS.COARSE_TO_FINE]
    assert torch.equal(stage_ang[:, S - 1], ang), "fit_pose_staged is not its stages run one after the other"
    assert len(printed) == N and np.allclose(printed, residual.reshape(-1).numpy(), rtol=1e-7, atol=0)
    err = K.joint_error(ang, bl, root, pose)
    assert (residual.reshape(-1).double() - err).abs().max().item() <= 1e-5
    assert bool((ang[:, K.DEAD] == 0).all()) and torch.equal(root, pose[:, :3])
    assert bool((ang.double() >= K.LO).all() and (ang.double() <= K.HI).all())
    restated = K.joint_error(*KS.lm_fit_staged(pose, KS.COARSE_TO_FINE)[:3], pose)
    print("FIGURE host program, cold, staged: %d of 64 not converged (restatement on the same poses: %d), worst %.3g m"
          % (K.not_converged(err), K.not_converged(restated), err.max().item()))
    start = torch.zeros(N, 37)
    p64 = pose.double().reshape(N, 16, 3)
    for s, (w, iters) in enumerate(KS.COARSE_TO_FINE):
        c0 = KS.weighted_cost64(start, bl, root, pose, w)
        c1 = KS.weighted_cost64(stage_ang[:, s], bl, root, pose, w)
        ref = KS.lm_stage(p64, start.double(), bl.double(), root.double(), w, iters, K.LO, K.HI, K.LAMBDA0)
        cr = KS.weighted_cost64(ref, bl, root, pose, w)
        allow = KS.cost_allowance(c0)
        print("FIGURE host program, stage %d: cost medians %.3g -> %.3g (restatement %.3g); largest excess over the restatement %.3g "
              "against an allowance of %.3g" % (s, c0.median(), c1.median(), cr.median(), (c1 - cr).max(), allow[(c1 - cr).argmax()]))
        assert bool((c1 <= c0 + allow).all()), "stage %d let the cost rise" % s
        assert bool((c1 <= cr + allow).all()), "stage %d stops above the restatement" % s
        start = stage_ang[:, s]
