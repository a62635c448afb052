"""GPU tests of the inverse-kinematics kernels (csrc/dhaug_ik.hip) through the C-ABI, with buffers of their own: every output has
3 extra rows of poison behind it that must be found untouched.

    dhaug_fk_jacobian   test_jacobian_matches_autograd, test_jacobian_second_trip, test_jacobian_transposed_is_fk_backward,
                        test_jacobian_single_slot
    dhaug_ik_fit        test_warm_start_fit, test_fit_exact_properties, test_fit_second_trip, test_fit_limits
    dhaug_ik_track      test_tracking

References (tests/ik_util.py): the oracle's FK in fp64, its autograd Jacobian, and an fp64 restatement of the solver.  A solution
is judged by the pose it reproduces -- converged = every joint of the fp64 FK of the returned fp32 angles, lengths and root within
1e-4 m of the target -- never by its angles.

The Jacobian is the one with respect to the generator's 31 live slots.  Columns 4, 9, 22, 23, 28, 33 must be exact zeros; of these
the oracle's FK reads slots 23 and 28 (the first joint of each arm, which the generator pins to 0), so autograd has a nonzero
column there: the element-wise comparison runs over the 31 live columns, and so does J^T g against dhaug_fk_backward, whose own
dead set is the columns that cannot move a joint (4, 9, 22, 27, 32, 33).

Bound of the Jacobian: 1e-5 m x pi/180 per degree = 1.745e-7, the FK's own tolerance carried through the derivative's scale."""
import os
import sys

import pytest
import torch

import ik_util as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
POISON = 7.5e37
EXTRA = 3
ITERS, TRACK_ITERS = 12, 8
FIT_NS = (1, 63, 64, 65, 512)
PERIOD = 251                                   # rows of the multi-trip batches repeat with a period that no tile size divides


@pytest.fixture(scope="module")
def L():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    sys.path.insert(0, ROOT)
    import dhaug_amd
    dhaug_amd._lib.lib()
    return dhaug_amd._lib


def stream():
    return torch.cuda.current_stream().cuda_stream or None


class Out:
    """an (N, W) fp32 output with EXTRA poisoned rows behind it"""

    def __init__(self, N, W):
        self.N = N
        self.full = torch.full((N + EXTRA, W), POISON, dtype=torch.float32, device="cuda")

    @property
    def ptr(self):
        return self.full.data_ptr()

    def rows(self):
        assert bool((self.full[self.N:] == POISON).all()), "rows behind the output were written"
        return self.full[:self.N]


def ptr(t):
    return None if t is None else t.data_ptr()


def same_bits(a, b):
    return a.shape == b.shape and bool(torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)))


def dev(t):
    return t.contiguous().cuda()


def jacobian(L, a, bl, N):
    J = Out(N, 48 * 37)
    L.call("dhaug_fk_jacobian", ptr(a), ptr(bl), J.ptr, N, stream())
    return J.rows().reshape(N, 48, 37)


def ik_fit(L, pose, init, N, iters=ITERS, lo=None, hi=None, lambda0=K.LAMBDA0):
    o = [Out(N, 37), Out(N, 15), Out(N, 3), Out(N, 1)]
    L.call("dhaug_ik_fit", ptr(pose), ptr(init), ptr(lo), ptr(hi), o[0].ptr, o[1].ptr, o[2].ptr, o[3].ptr, N, iters, lambda0, stream())
    return [x.rows() for x in o[:3]] + [o[3].rows().reshape(N)]


def ik_track(L, pose, offsets, init, iters=TRACK_ITERS, lambda0=K.LAMBDA0):
    T, S = offsets[-1], len(offsets) - 1
    off = torch.tensor(offsets, dtype=torch.int64, device="cuda")
    o = [Out(T, 37), Out(T, 15), Out(T, 3), Out(T, 1)]
    L.call("dhaug_ik_track", ptr(pose), ptr(off), ptr(init), None, None, o[0].ptr, o[1].ptr, o[2].ptr, o[3].ptr, S, iters, lambda0,
           stream())
    return [x.rows() for x in o[:3]] + [o[3].rows().reshape(T)]


def measured(got, pose):
    """fp64 joint error of a returned solution (angles, bone_len, root, residual) against the target"""
    return K.joint_error(got[0].cpu(), got[1].cpu(), got[2].cpu(), pose.cpu())


# ---- shared inputs and references, computed once ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def jac_batch():
    g = torch.Generator().manual_seed(11)
    a, bl = K.trial_angles(PERIOD, g, spread=1.0), K.trial_lengths(PERIOD, g)     # the whole generator range
    return {"a": a, "bl": bl, "ref": K.jacobian64(a, bl)}


@pytest.fixture(scope="module")
def fit_batch():
    d = K.trial_fit_inputs(max(FIT_NS))
    d["restated"] = K.joint_error(*K.lm_fit(d["pose"], d["init"], iters=ITERS)[:3], d["pose"])
    return d


@pytest.fixture(scope="module")
def track_batch():
    d = K.trial_track_inputs(65, K.ragged_lengths(65))
    d["restated"] = K.joint_error(*K.lm_track(d["pose"], d["offsets"], d["init"], iters=TRACK_ITERS)[:3], d["pose"])
    return d


def check_jacobian(J, ref, what):
    J = J.double().cpu()
    err = (J[:, :, K.LIVE] - ref[:, :, K.LIVE]).abs().max().item()
    print("FIGURE %s: largest |J - autograd| over the live columns %.4g m/deg (bound %.4g)" % (what, err, K.JAC_TOL))
    assert bool(torch.isfinite(J).all())
    assert bool((J[:, :, K.DEAD + K.STILL] == 0).all()), "%s: a column that must be exactly 0 is not" % what
    assert err <= K.JAC_TOL, what


# ---- a. dhaug_fk_jacobian -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 63, 64, 65, PERIOD])
def test_jacobian_matches_autograd(L, jac_batch, N):
    a, bl = dev(jac_batch["a"][:N]), dev(jac_batch["bl"][:N])
    J = jacobian(L, a, bl, N)
    check_jacobian(J, jac_batch["ref"][:N], "fk_jacobian N=%d" % N)
    assert same_bits(J, jacobian(L, a, bl, N))


def test_jacobian_second_trip(L, jac_batch):
    """one pose more than a full pass of the grid (DHAUG_FK_JACOBIAN_MAX_BLOCKS workgroups of 64): rows repeat with period 251, so
    every row has the reference of row n mod 251; rows behind the first period are compared by bits with their first copy"""
    N = L.FK_JACOBIAN_MAX_BLOCKS * 64 + 1
    idx = torch.arange(N) % PERIOD
    a, bl = dev(jac_batch["a"][idx]), dev(jac_batch["bl"][idx])
    J = jacobian(L, a, bl, N)
    check_jacobian(J[:PERIOD], jac_batch["ref"], "fk_jacobian first period of N=%d" % N)
    first = J[:PERIOD].contiguous().view(torch.int32)
    assert bool(torch.equal(J.view(torch.int32), first[idx.cuda()]))


def test_jacobian_transposed_is_fk_backward(L, jac_batch):
    """J^T g = the angle gradient of dhaug_fk_backward for a random g, on the 31 live slots, within that entry's tolerance (1e-4 of
    the largest gradient, tests/test_cpu_boundary.py::test_hostcheck_fk_math_matches_oracle)"""
    N = 193
    a, bl = dev(jac_batch["a"][:N]), dev(jac_batch["bl"][:N])
    g = torch.randn(N, 48, generator=torch.Generator().manual_seed(12))
    ga, gb, gr = Out(N, 37), Out(N, 15), Out(N, 3)
    L.call("dhaug_fk_backward", ptr(a), ptr(bl), ptr(dev(g)), ga.ptr, gb.ptr, gr.ptr, N, stream())
    back = ga.rows().double().cpu()
    jtg = torch.einsum("nrc,nr->nc", jacobian(L, a, bl, N).double().cpu(), g.double())
    err = (jtg[:, K.LIVE] - back[:, K.LIVE]).abs().max().item()
    print("FIGURE J^T g against fk_backward: %.4g (largest gradient %.4g)" % (err, back.abs().max().item()))
    assert err <= 1e-4 * back.abs().max().item()


@pytest.fixture(scope="module")
def slot_batch():
    """row i: the base pose with live slot LIVE[i] alone moved by 3 degrees"""
    g = torch.Generator().manual_seed(13)
    base, bl = K.trial_angles(1, g), K.trial_lengths(1, g)
    a = base.repeat(len(K.LIVE), 1)
    for i, s in enumerate(K.LIVE):
        a[i, s] += 3.0
    bl = bl.repeat(len(K.LIVE), 1)
    return {"a": a, "bl": bl, "ref": K.jacobian64(a, bl), "base_a": base, "base": K.jacobian64(base, bl[:1])[0]}


@pytest.mark.parametrize("i", range(len(K.LIVE)))
def test_jacobian_single_slot(L, slot_batch, i):
    """one launch of one pose per live slot: the whole matrix against autograd, and the GPU's own change from the base pose against
    autograd's change, so that the one column set the move reaches (none at all for slots 27 and 32) is what changed"""
    s = K.LIVE[i]
    bl = dev(slot_batch["bl"][i:i + 1])
    J = jacobian(L, dev(slot_batch["a"][i:i + 1]), bl, 1)
    check_jacobian(J, slot_batch["ref"][i:i + 1], "fk_jacobian slot %d + 3 deg" % s)
    Jb = jacobian(L, dev(slot_batch["base_a"]), bl, 1)
    d_gpu = (J.double().cpu()[0] - Jb.double().cpu()[0])[:, K.LIVE]
    d_ref = (slot_batch["ref"][i] - slot_batch["base"])[:, K.LIVE]
    assert (d_gpu - d_ref).abs().max().item() <= 2 * K.JAC_TOL
    if s in K.STILL:
        assert same_bits(J, Jb)


# ---- b. dhaug_ik_fit ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", FIT_NS)
def test_warm_start_fit(L, fit_batch, N):
    """the trial's inputs (first N rows of one seeded batch), 12 steps from 5 degrees off: at most 0.5 % of the poses not converged,
    and the fp64 restatement meets the same cap on the same rows; the reported residual is the measured one within 1e-5 m"""
    pose, init = dev(fit_batch["pose"][:N]), dev(fit_batch["init"][:N])
    got = ik_fit(L, pose, init, N)
    err = measured(got, pose)
    bad, bad_ref = K.not_converged(err), K.not_converged(fit_batch["restated"][:N])
    print("FIGURE ik_fit N=%d: not converged %d (restatement %d); error median %.3g max %.3g m (restatement max %.3g)"
          % (N, bad, bad_ref, err.median().item(), err.max().item(), fit_batch["restated"][:N].max().item()))
    assert bad_ref <= 0.005 * N
    assert bad <= 0.005 * N
    assert (got[3].double().cpu() - err).abs().max().item() <= 1e-5


def exact_properties(got, pose, init, lo, hi, what):
    ang, bl, root, res = [t.cpu() for t in got]
    pose_c = pose.cpu()
    assert bool(torch.isfinite(ang).all() and torch.isfinite(bl).all() and torch.isfinite(res).all()), what
    assert bool((ang.double() >= lo).all() and (ang.double() <= hi).all()), what
    assert bool((ang[:, K.DEAD] == 0).all()), what
    assert same_bits(root, pose_c.reshape(-1, 16, 3)[:, 0].contiguous()), what
    want = K.bone_lengths64(pose_c).float()
    ulps = (bl.view(torch.int32) - want.view(torch.int32)).abs().max().item()
    print("FIGURE %s: bone lengths within %d ulp of the rounded fp64 distance" % (what, ulps))
    assert ulps <= 2, what
    # accept / reject never lets the fp32 cost rise.  Measured in fp64 the two costs carry the FK's fp32 error (1e-5 m per joint
    # coordinate at most, README): d(cost) <= 2 sqrt(cost) sqrt(45) 1e-5
    start = torch.minimum(torch.maximum(init.cpu().double(), lo), hi)
    start[:, K.DEAD] = 0.0
    c0, c1 = K.cost64(start, bl, root, pose_c), K.cost64(ang, bl, root, pose_c)
    slack = 2 * c0.sqrt() * (45 ** 0.5) * 1e-5 + 1e-10
    assert bool((c1 <= c0 + slack).all()), (what, (c1 - c0 - slack).max().item())
    return c0, c1


def test_fit_exact_properties(L, fit_batch):
    g = torch.Generator().manual_seed(14)
    N = 193
    init = dev(fit_batch["init"][:N])
    for what, pose in (("on the manifold", fit_batch["pose"][:N]), ("5 mm off the manifold", K.off_manifold(fit_batch["pose"][:N], g))):
        pose = dev(pose)
        got = ik_fit(L, pose, init, N)
        c0, c1 = exact_properties(got, pose, init, K.LO, K.HI, "ik_fit " + what)
        print("FIGURE ik_fit %s: cost %.3g -> %.3g (medians), residual median %.3g m"
              % (what, c0.median().item(), c1.median().item(), got[3].median().item()))
        again = ik_fit(L, pose, init, N)
        assert all(same_bits(x, y) for x, y in zip(got, again)), what
        for n in (1, 65):                                       # poses are independent lanes: a prefix gives the same bits
            part = ik_fit(L, pose, init, n)
            assert all(same_bits(x, y[:n]) for x, y in zip(part, got)), (what, n)
        one = ik_fit(L, pose, init, N, iters=1)
        assert bool((one[0] != init).any(dim=1).all()), "%s: a single step left a pose at its start" % what
    # the T-pose start (init = NULL) is the same as an explicit row of zeros
    pose = dev(fit_batch["pose"][:65])
    assert all(same_bits(x, y) for x, y in zip(ik_fit(L, pose, None, 65, iters=3), ik_fit(L, pose, torch.zeros(65, 37, device="cuda"), 65, iters=3)))


def test_fit_second_trip(L, fit_batch):
    """one pose more than a full pass of the grid (DHAUG_IK_MAX_BLOCKS workgroups of 64 poses), rows repeating with period 251: every
    row must carry the bits of its first copy, and the first period those of a call of its own"""
    N = L.IK_MAX_BLOCKS * 64 + 1
    idx = torch.arange(N) % PERIOD
    pose, init = dev(fit_batch["pose"][idx]), dev(fit_batch["init"][idx])
    got = ik_fit(L, pose, init, N, iters=4)
    alone = ik_fit(L, pose, init, PERIOD, iters=4)
    for x, y in zip(got, alone):
        assert same_bits(x[:PERIOD].contiguous(), y)
        assert same_bits(x, y[idx.cuda()])


def test_fit_limits(L, fit_batch):
    """the knee of the right leg (slot 3, one hinge that alone sets the hip-ankle distance) is limited to [-40, 0] while every target
    bends it by 63 degrees or more: the answer sits on the boundary and the residual is finite and honest"""
    N = 65
    lo, hi = K.LO.clone(), K.HI.clone()
    lo[3] = -40.0
    assert bool((fit_batch["truth"][:N, 3] < -60).all())
    init = fit_batch["init"][:N].clone()
    init[:, 3] = -20.0
    pose, init = dev(fit_batch["pose"][:N]), dev(init)
    got = ik_fit(L, pose, init, N, lo=dev(lo.float()), hi=dev(hi.float()))
    exact_properties(got, pose, init, lo, hi, "ik_fit with a narrowed knee")
    assert bool((got[0][:, 3] == -40.0).all())
    err = measured(got, pose)
    assert bool(torch.isfinite(got[3]).all()) and err.min().item() > K.CONVERGED_M
    assert (got[3].double().cpu() - err).abs().max().item() <= 1e-5


# ---- c. dhaug_ik_track ----------------------------------------------------------------------------------------------------------------
def test_tracking(L, track_batch):
    """the trial's sequences (at most 3 degrees per slot and frame, 8 steps per frame), ragged, a length of 1 among them, at S = 1, 3
    and 65: at most 1 % of the frames not converged, with the restatement held to the same cap on the same frames"""
    off, pose, init = track_batch["offsets"], dev(track_batch["pose"]), dev(track_batch["init"])
    full = ik_track(L, pose, off, init)
    exact_properties(full, pose, full[0], K.LO, K.HI, "ik_track")          # (limits, dead slots, root, lengths)
    for S in (1, 3, 65):
        T = off[S]
        got = ik_track(L, pose, off[:S + 1], init)
        err = measured(got, pose[:T])
        bad, bad_ref = K.not_converged(err), K.not_converged(track_batch["restated"][:T])
        print("FIGURE ik_track S=%d, %d frames: not converged %d (restatement %d); error median %.3g max %.3g m"
              % (S, T, bad, bad_ref, err.median().item(), err.max().item()))
        assert bad_ref <= 0.01 * T and bad <= 0.01 * T
        assert (got[3].double().cpu() - err).abs().max().item() <= 1e-5
        # a sequence's result does not depend on how many others ride along
        assert all(same_bits(x, y[:T].contiguous()) for x, y in zip(got, full))
    # ... nor on what they hold: sequences 0 and 2 keep their bits when sequence 1 (one frame) becomes another pose
    other = pose.clone()
    other[off[1]:off[2]] = pose[off[3]:off[3] + 1]
    swapped = ik_track(L, other, off[:4], init)
    for x, y in zip(swapped, full):
        assert same_bits(x[:off[1]].contiguous(), y[:off[1]].contiguous()) and same_bits(x[off[2]:off[3]].contiguous(), y[off[2]:off[3]].contiguous())
    # frame 0 of every sequence is ik_fit of that frame from the same start
    first = torch.tensor(off[:-1], device="cuda")
    fit0 = ik_fit(L, pose[first].contiguous(), init, 65, iters=TRACK_ITERS)
    assert all(same_bits(x, y[first].contiguous()) for x, y in zip(fit0, full))
    assert all(same_bits(x, y) for x, y in zip(full, ik_track(L, pose, off, init)))
