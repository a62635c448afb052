"""GPU tests of the staged, joint-weighted inverse-kinematics fit: dhaug_ik_fit_staged through the C-ABI with buffers of its own
(every output has 3 poisoned rows behind it that must be found untouched), and the public surface on top of it
(ops.ik_fit_staged, fit_pose(schedule= / joint_weights= / bone_len=), fit_sequences(cold_start=True)).

    identity with dhaug_ik_fit       test_one_stage_of_ones_is_ik_fit, test_second_trip
    weight 0                         test_zero_weight_is_exact
    a weighted stage against fp64    test_weighted_stage_against_restatement
    stages                           test_every_stage_lowers_its_own_cost
    what it is for                   test_cold_start_halves_the_failures, test_cold_started_sequences
    memory                           test_every_output_element_is_written
    surface                          test_public_surface

References (tests/ik_util.py, tests/ik_staged_util.py): the oracle's FK in fp64 and the fp64 restatement of the weighted, staged solver;
tests/golden/ik_staged.npz holds the restatement's cold-start errors on the 256 poses of the cold-start test.  A solution is judged
by the pose it reproduces (converged = every joint of the fp64 FK of the returned fp32 angles, lengths and root within 1e-4 m).
Cost comparisons in fp64 allow 2 sqrt(cost) sqrt(45) 1e-5 for the fp32 FK's error on both sides, cost = the start's, as
tests/test_gpu_ik_kernels.py does."""
import argparse
import ctypes
import os
import sys

import pytest
import torch

import ik_util as K
import ik_staged_util as KS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
POISON = 7.5e37
EXTRA = 3
PERIOD = 251
ONES = [1.0] * 16
# a weight table with nothing regular about it: two joints left out (6 and 12, an ankle and a wrist), weights below and above 1
MIXED = [0.0, 1.0, 0.5, 2.0, 1.0, 0.25, 0.0, 1.5, 1.0, 1.0, 0.7, 3.0, 0.0, 1.0, 1.25, 0.3]


@pytest.fixture(scope="module")
def L():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    sys.path.insert(0, ROOT)
    import dhaug_amd
    dhaug_amd._lib.lib()
    return dhaug_amd._lib


@pytest.fixture(scope="module")
def M(L):
    from dhaug_amd import ops
    from dhaug_amd.models_Fk_GAN import forward_kinematics_DH_model as fkm
    args = argparse.Namespace(batch_size=3, random_seed=0, single_or_multi_train_mode="single", architecture="3,3,3")
    return argparse.Namespace(ops=ops, fkm=fkm, fk=fkm.Forward_Kinematics_DH_Model(args, ["S1"], None), lib=L)


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


def all_same_bits(x, y):
    return all(same_bits(a, b) for a, b in zip(x, y))


def dev(t):
    return None if t is None else t.contiguous().cuda()


def outputs(N):
    return [Out(N, 37), Out(N, 15), Out(N, 3), Out(N, 1)]


def ik_fit(L, pose, init, N, iters, lo=None, hi=None, lambda0=K.LAMBDA0):
    o = outputs(N)
    L.call("dhaug_ik_fit", ptr(pose), ptr(init), ptr(lo), ptr(hi), o[0].ptr, o[1].ptr, o[2].ptr, o[3].ptr, N, iters, lambda0, stream())
    return [x.rows() for x in o[:3]] + [o[3].rows().reshape(N)]


def ik_fit_staged(L, pose, init, N, stages, lo=None, hi=None, bone_len=None, lambda0=K.LAMBDA0):
    """stages: (weights16, iters) pairs.  The weight table and the step counts are host arrays."""
    S = len(stages)
    w = (ctypes.c_float * (16 * S))(*[float(v) for row, _ in stages for v in row])
    it = (ctypes.c_int * S)(*[n for _, n in stages])
    o = outputs(N)
    L.call("dhaug_ik_fit_staged", ptr(pose), ptr(init), ptr(lo), ptr(hi), ptr(bone_len), w, it, S, lambda0, o[0].ptr, o[1].ptr, o[2].ptr,
           o[3].ptr, N, stream())
    return [x.rows() for x in o[:3]] + [o[3].rows().reshape(N)]


def clamped(init):
    a = torch.minimum(torch.maximum(init.double(), K.LO), K.HI)
    a[:, K.DEAD] = 0.0
    return a


@pytest.fixture(scope="module")
def batch():
    """the trial's inputs of the cold-start recording: 256 poses with their 5-degree warm starts"""
    return K.trial_fit_inputs(KS.GOLDEN_POSES)


# ---- 1. one stage of weights 1 = dhaug_ik_fit -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 63, 64, 65, 257])
def test_one_stage_of_ones_is_ik_fit(L, batch, N):
    """all four outputs bit for bit, with and without a start, with the generator's and with the caller's limits (a knee narrowed to
    [-40, 0], which every target bends further: the clamp is at work), at one lane, a ragged wave and several workgroups"""
    idx = torch.arange(N) % KS.GOLDEN_POSES
    pose, init = dev(batch["pose"][idx]), dev(batch["init"][idx])
    lo, hi = K.LO.clone(), K.HI.clone()
    lo[3] = -40.0
    lo, hi = dev(lo.float()), dev(hi.float())
    for k, start, lim in ((5, None, (None, None)), (5, init, (None, None)), (3, None, (lo, hi)), (3, init, (lo, hi)), (1, init, (None, None))):
        want = ik_fit(L, pose, start, N, k, *lim)
        got = ik_fit_staged(L, pose, start, N, [(ONES, k)], *lim)
        assert all_same_bits(got, want), (N, k, start is not None, lim[0] is not None)
    assert bool((got[0] != init).any(dim=1).all()), "a step left a pose at its start: nothing was compared"


def test_second_trip(L, batch):
    """one pose more than a full pass of the grid (DHAUG_IK_MAX_BLOCKS workgroups of 64 poses), rows repeating with period 251: every
    row carries the bits of its first copy, and the first period those of a call of its own"""
    N = L.IK_MAX_BLOCKS * 64 + 1
    idx = torch.arange(N) % PERIOD
    pose, init = dev(batch["pose"][idx]), dev(batch["init"][idx])
    stages = [(MIXED, 2), (ONES, 2)]
    got = ik_fit_staged(L, pose, init, N, stages)
    alone = ik_fit_staged(L, pose, init, PERIOD, stages)
    for x, y in zip(got, alone):
        assert same_bits(x[:PERIOD].contiguous(), y)
        assert same_bits(x, y[idx.cuda()])


# ---- 2. weight 0 ------------------------------------------------------------------------------------------------------------------------
def test_zero_weight_is_exact(L, batch):
    """joints 2 and 3 (right knee and ankle) are all that unknowns 0..3 move: with weight 0 on both, slots 0..3 come back as the clamped
    start, bit for bit, while the rest of the pose is fitted; and with the lengths given, moving the targets of those two joints by a
    metre changes no bit of any output"""
    N = 65
    pose, init, bl = batch["pose"][:N], batch["init"][:N], batch["bone_len"][:N]
    w = list(ONES)
    w[2] = w[3] = 0.0
    got = ik_fit_staged(L, dev(pose), dev(init), N, [(w, 12)])
    assert same_bits(got[0][:, :4].cpu(), clamped(init)[:, :4].float())
    assert bool((got[0][:, 5:9].cpu() != init[:, 5:9]).any(dim=1).all()), "the other leg did not move: nothing was fitted"
    others = [j for j in range(1, 16) if j not in (2, 3)]
    d = (K.fk64(got[0].cpu(), got[1].cpu(), got[2].cpu()) - pose.double()).norm(dim=2)
    assert d[:, others].max().item() <= K.CONVERGED_M and d[:, [2, 3]].min().item() > K.CONVERGED_M
    assert (got[3].double().cpu() - d[:, others].max(dim=1).values).abs().max().item() <= 1e-5       # the residual leaves them out
    # from the T-pose too (a start of +0: theta - delta must not turn it into -0)
    cold = ik_fit_staged(L, dev(pose), None, N, [(w, 4)])
    assert same_bits(cold[0][:, :4], torch.zeros(N, 4, device="cuda"))
    moved = pose.clone()
    moved[:, [2, 3]] += 1.0
    a = ik_fit_staged(L, dev(pose), dev(init), N, [(w, 8)], bone_len=dev(bl))
    b = ik_fit_staged(L, dev(moved), dev(init), N, [(w, 8)], bone_len=dev(bl))
    assert all_same_bits(a, b)
    assert same_bits(a[1], dev(bl)), "the caller's lengths are returned as given"
    # (without the lengths the moved joints set their bones: the call above is what bone_len is for)
    c = ik_fit_staged(L, dev(moved), dev(init), N, [(w, 8)])
    assert not same_bits(c[1], got[1])


# ---- 3. one weighted stage against the fp64 restatement -----------------------------------------------------------------------------
def test_weighted_stage_against_restatement(L, batch):
    """65 poses, 12 steps from the 5-degree warm start under MIXED: the weighted fp64 cost of what the kernel returns is at most the
    restatement's plus the allowance, and not above the start's; the residual is the largest distance over the weighted joints"""
    N, iters = 65, 12
    pose, init = batch["pose"][:N], batch["init"][:N]
    got = [t.cpu() for t in ik_fit_staged(L, dev(pose), dev(init), N, [(MIXED, iters)])]
    ref = KS.lm_fit_staged(pose, [(MIXED, iters)], init=init)
    c0 = KS.weighted_cost64(clamped(init), got[1], got[2], pose, MIXED)
    c1 = KS.weighted_cost64(got[0], got[1], got[2], pose, MIXED)
    cr = KS.weighted_cost64(*ref[:3], pose, MIXED)
    allow = KS.cost_allowance(c0)
    print("FIGURE weighted stage: cost medians %.3g -> %.3g (restatement %.3g), largest c1 - cr %.3g, allowance there %.3g"
          % (c0.median(), c1.median(), cr.median(), (c1 - cr).max(), allow[(c1 - cr).argmax()]))
    assert bool((c1 <= cr + allow).all())
    assert bool((c1 <= c0).all()), "the cost rose"
    err = KS.joint_error_over(got[0], got[1], got[2], pose, MIXED)
    assert (got[3].double() - err).abs().max().item() <= 1e-5
    assert bool((got[0].double() >= K.LO).all() and (got[0].double() <= K.HI).all() and (got[0][:, K.DEAD] == 0).all())


# ---- 4. stages --------------------------------------------------------------------------------------------------------------------------
def test_every_stage_lowers_its_own_cost(L, batch):
    """the schedule's prefixes from the T-pose: what a prefix returns is where the next stage starts, so the cost under stage s's weights
    after s + 1 stages must not be above its value after s stages (within the allowance of two fp64 costs of fp32 solutions)"""
    N = 65
    pose = batch["pose"][:N]
    start = torch.zeros(N, 37)
    for s in range(len(KS.COARSE_TO_FINE)):
        w = KS.COARSE_TO_FINE[s][0]
        got = [t.cpu() for t in ik_fit_staged(L, dev(pose), None, N, KS.COARSE_TO_FINE[:s + 1])]
        c0 = KS.weighted_cost64(start, got[1], got[2], pose, w)
        c1 = KS.weighted_cost64(got[0], got[1], got[2], pose, w)
        print("FIGURE stage %d: cost under its weights, medians %.3g -> %.3g; largest rise %.3g" % (s, c0.median(), c1.median(), (c1 - c0).max()))
        assert bool((c1 <= c0 + KS.cost_allowance(c0)).all()), s
        assert (got[3].double() - KS.joint_error_over(got[0], got[1], got[2], pose, w)).abs().max().item() <= 1e-5
        start = got[0]


# ---- 5. cold start ------------------------------------------------------------------------------------------------------------------------
def test_cold_start_halves_the_failures(L, batch):
    """the 256 recorded poses from the T-pose: C poses not converged by the coarse-to-fine schedule (40 steps) against P by
    dhaug_ik_fit with 40 steps, in the same run.  Gate: C <= P / 2.  The restatement's R (tests/golden/ik_staged.npz) is printed
    beside C, not gated.  One run on an MI355X, 2026-10-21: C = 7, P = 109, R = 7."""
    N = KS.GOLDEN_POSES
    pose = dev(batch["pose"])
    staged = ik_fit_staged(L, pose, None, N, KS.COARSE_TO_FINE)
    plain = ik_fit(L, pose, None, N, 40)
    err_c = K.joint_error(staged[0].cpu(), staged[1].cpu(), staged[2].cpu(), batch["pose"])
    err_p = K.joint_error(plain[0].cpu(), plain[1].cpu(), plain[2].cpu(), batch["pose"])
    C, P = K.not_converged(err_c), K.not_converged(err_p)
    g = KS.load_golden()
    print("FIGURE cold start, 256 poses, 40 steps: staged C = %d not converged (worst %.3g m), single stage P = %d; restatement R = %d "
          "(single stage %d)" % (C, err_c.max().item(), P, int(g["not_converged"]), int((g["single_err"] > K.CONVERGED_M).sum())))
    assert 2 * C <= P
    assert (staged[3].double().cpu() - err_c).abs().max().item() <= 1e-5
    assert all_same_bits(staged, ik_fit_staged(L, pose, None, N, KS.COARSE_TO_FINE))


# ---- 6. sequences -------------------------------------------------------------------------------------------------------------------------
def test_cold_started_sequences(M):
    """the trial's 65 ragged sequences without a start: frames not converged with cold_start=True at most half of those without, in the
    same run; frame 0 of every sequence is started from the schedule's fit of that frame"""
    d = K.trial_track_inputs(65, K.ragged_lengths(65))
    off, pose = d["offsets"], d["pose"].cuda()
    lengths = [b - a for a, b in zip(off, off[1:])]
    cold = M.fk.fit_sequences(pose, lengths, cold_start=True)
    plain = M.fk.fit_sequences(pose, lengths)
    bad_c = K.not_converged(K.joint_error(cold.angles37.cpu(), cold.bone_len.cpu(), cold.root.cpu(), d["pose"]))
    bad_p = K.not_converged(K.joint_error(plain.angles37.cpu(), plain.bone_len.cpu(), plain.root.cpu(), d["pose"]))
    print("FIGURE sequences without a start, %d frames: not converged %d with cold_start, %d without" % (off[-1], bad_c, bad_p))
    assert 2 * bad_c <= bad_p
    first = pose[torch.tensor(off[:-1], device="cuda")]
    init = M.ops.ik_fit_staged(first, *zip(*M.ops.IK_COARSE_TO_FINE)).angles37
    by_hand = M.ops.ik_track(pose, off, init)
    assert all(torch.equal(x, y) for x, y in zip(cold, by_hand))
    # with a start of the caller's, cold_start changes nothing
    a = M.fk.fit_sequences(pose, lengths, init=d["init"].cuda(), cold_start=True)
    b = M.fk.fit_sequences(pose, lengths, init=d["init"].cuda())
    assert all(torch.equal(x, y) for x, y in zip(a, b))


# ---- 7. unwritten memory ------------------------------------------------------------------------------------------------------------------
def test_every_output_element_is_written(L, batch):
    """N = 65 (a full wave and one lane of the next): no element of the 65 rows keeps the poison, with and without the caller's
    lengths; the rows behind stay poisoned (Out.rows)"""
    N = 65
    pose, bl = dev(batch["pose"][:N]), dev(batch["bone_len"][:N])
    for given in (None, bl):
        for t in ik_fit_staged(L, pose, None, N, [(MIXED, 1), (ONES, 1)], bone_len=given):
            assert bool(torch.isfinite(t).all()) and not bool((t == POISON).any())


# ---- the public surface -------------------------------------------------------------------------------------------------------------------
def test_public_surface(M, L, batch):
    """ops.ik_fit_staged and fit_pose's new arguments give the C-ABI's bits; refused calls do not reach the library"""
    N = 65
    pose, init, bl = batch["pose"][:N].cuda(), batch["init"][:N].cuda(), batch["bone_len"][:N].cuda()
    want = ik_fit_staged(L, pose, None, N, KS.COARSE_TO_FINE)
    got = M.fk.fit_pose(pose, schedule="coarse_to_fine")
    assert type(got).__name__ == "IkFit" and [tuple(t.shape) for t in got] == [(N, 37), (N, 15), (N, 3), (N,)]
    assert all_same_bits(got, want)
    assert all_same_bits(M.fk.fit_pose(pose.cpu().numpy(), schedule=list(M.ops.IK_COARSE_TO_FINE)), want)
    want = ik_fit_staged(L, pose, init, N, [(MIXED, 6)], bone_len=bl)
    assert all_same_bits(M.fk.fit_pose(pose, init=init, iters=6, joint_weights=MIXED, bone_len=bl), want)
    assert all_same_bits(M.ops.ik_fit_staged(pose, torch.tensor([MIXED]), [6], init=init, bone_len=bl), want)
    lo, hi = M.fk.ik_limits("normal")
    fit = M.fk.fit_pose(pose, schedule="coarse_to_fine", limits="normal")
    assert bool((fit.angles37 >= torch.tensor(lo).cuda()).all() and (fit.angles37 <= torch.tensor(hi).cuda()).all())
    # fit_pose with none of the new arguments: ops.ik_fit's bits, as before
    assert all_same_bits(M.fk.fit_pose(pose, init=init, iters=4), ik_fit(L, pose, init, N, 4))
    calls = M.lib.CALLS[0]
    for fn in (lambda: M.ops.ik_fit_staged(pose, [ONES] * 9, [1] * 9), lambda: M.ops.ik_fit_staged(pose, [ONES, [0.0] * 16], [2, 2]),
               lambda: M.ops.ik_fit_staged(pose, [ONES], [0]), lambda: M.ops.ik_fit_staged(pose, [MIXED], [2], bone_len=bl[:64]),
               lambda: M.ops.ik_fit_staged(pose, [ONES], [2], init=init + 500.0),
               lambda: M.fk.fit_pose(pose, schedule="coarse_to_fine", joint_weights=ONES)):
        with pytest.raises(ValueError):
            fn()
    assert M.lib.CALLS[0] == calls, "a refused call reached the library"
    # the entry itself refuses what the binding would have stopped
    o = outputs(N)
    for S, w, it in ((0, ONES, [1]), (9, ONES * 9, [1] * 9), (1, ONES, [0]), (1, [-1.0] + ONES[1:], [1]), (1, ONES[:15] + [float("nan")], [1]),
                     (1, ONES[:15] + [float("inf")], [1]), (2, ONES + [1.0] + [0.0] * 15, [1, 1])):
        with pytest.raises(Exception):
            L.call("dhaug_ik_fit_staged", ptr(pose), None, None, None, None, (ctypes.c_float * len(w))(*w), (ctypes.c_int * len(it))(*it), S,
                   K.LAMBDA0, o[0].ptr, o[1].ptr, o[2].ptr, o[3].ptr, N, stream())
    assert all(bool((x.full == POISON).all()) for x in o), "a refused call launched"
