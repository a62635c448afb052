"""CPU-side checks of the MPJPE criterion: argument errors of dhaug_pose_mpjpe (before any launch) and of its wrapper, and the
self-consistency of tests/golden/posetrain_mpjpe.npz (recorded from the reference's video loops with the reference's mpjpe)."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

import posetrain_util as PU
import posetrain_mpjpe_util as MU

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# test_fixture_is_self_consistent: 10 x the measured difference between the restated kernel arithmetic (fp64 distances, zero
# gradient at zero distance, posetrain_util.restated_loop's clip + Adam) and the reference's final state.  Measured on the CPU:
# 2.682e-7 after the 12 steps on either loop (parameters of magnitude <= 1 moved by 1.18e-2); losses agree to 6.8e-7, norms to
# 7.6e-7 relative.
MEASURED_RESTATEMENT = 2.69e-7
RESTATEMENT_BOUND = 10 * MEASURED_RESTATEMENT


@pytest.fixture(scope="module")
def built():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    ge.build_lib(verbose=False)
    import dhaug_amd
    return dhaug_amd


@pytest.fixture(scope="module")
def G():
    return MU.load_golden()


def test_c_abi_argument_errors(built):
    L = built._lib.lib()
    buf = (ctypes.c_float * 4096)()
    a16 = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)
    mis = ctypes.c_void_p(a16.value + 4)
    N = None
    # dhaug_pose_mpjpe(pred, tgt, joints, poses, grad, loss, meter, workspace, stream)
    assert L.dhaug_pose_mpjpe(a16, a16, -1, 1, a16, a16, N, a16, N) == -1                              # joints < 0
    assert L.dhaug_pose_mpjpe(a16, a16, 16, -1, a16, a16, N, a16, N) == -1                             # poses < 0
    assert L.dhaug_pose_mpjpe(N, a16, 16, 1, a16, a16, N, a16, N) == -1                                # NULL pred
    assert L.dhaug_pose_mpjpe(a16, N, 16, 1, a16, a16, N, a16, N) == -1                                # NULL tgt
    assert L.dhaug_pose_mpjpe(a16, a16, 16, 1, N, a16, N, a16, N) == -1                                # NULL grad
    assert L.dhaug_pose_mpjpe(a16, a16, 16, 1, a16, N, N, a16, N) == -1                                # NULL loss
    assert L.dhaug_pose_mpjpe(a16, a16, 16, 1, a16, a16, N, N, N) == -1                                # NULL workspace
    assert L.dhaug_pose_mpjpe(a16, a16, 0, 1, N, a16, N, a16, N) == -1                                 # ... also for no joints
    assert L.dhaug_pose_mpjpe(a16, a16, 16, 1, a16, a16, mis, a16, N) == -2                            # meter not 8-byte aligned
    assert L.dhaug_pose_mpjpe(a16, a16, 16, 1, a16, a16, N, mis, N) == -2                              # workspace not 8-byte aligned
    assert L.dhaug_pose_mpjpe(N, N, 0, 0, a16, a16, N, a16, N) == 0                                    # no joints: a no-op


def test_wrapper_refuses_bad_shapes_and_cpu_tensors(built):
    from dhaug_amd import ops
    z = torch.zeros
    with pytest.raises(ValueError):
        ops.pose_mpjpe(z(4, 16, 3), z(4, 15, 3), 4)                   # shapes differ
    with pytest.raises(ValueError):
        ops.pose_mpjpe(z(4, 16, 2), z(4, 16, 2), 4)                   # rows are not 3 wide
    with pytest.raises(ValueError):
        ops.pose_mpjpe(z(48), z(48), 1)
    with pytest.raises(ValueError):
        ops.pose_mpjpe(z(4, 16, 3), z(4, 16, 3), -1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.pose_mpjpe(z(4, 16, 3), z(4, 16, 3), 4)


def test_fixture_exercises_clipping_and_zero_distances(G):
    """the conditions the fixture is built for: norms on both sides of max_norm = 1 (the gain of posetrain_mpjpe_util), and one
    joint per pose -- the hip the stub pads with zeros, against root-centred targets -- at distance exactly 0"""
    for loop in MU.LOOPS:
        norms = G[loop + "_norms"]
        assert len(norms) == 12 == len(G[loop + "_losses"])
        assert (norms < 0.85).sum() >= 4 and (norms > 1.08).sum() >= 4, (loop, norms)
        model = PU.load_initial(MU.make_model(loop), G, loop)
        model.train()
        for b3, b2 in PU.batches_of(G, loop):
            for inp, tgt in PU.steps_of_batch(loop, b3, b2):
                with torch.no_grad():
                    e = torch.norm(model(inp) - tgt, dim=-1)
                assert e.shape[-1] == 16 and bool((e[..., 0] == 0).all()) and bool((e[..., 1:] > 0).all())
    # the gain is what the fixture's initial state holds
    torch.manual_seed(0)
    assert np.array_equal(G["gan_init_c.weight"], MU.make_model("gan").c.weight.detach().numpy())
    assert np.array_equal(G["gan_init_c.weight"], (PU.make_model("gan").c.weight.detach() * MU.GAIN).numpy())


def test_fixture_is_self_consistent(G):
    """The arithmetic the kernels implement -- fp64 joint distances, a zero gradient at zero distance, the flat fp32 gradient, one
    global fp64 sum of squares, coef in fp32, Adam -- restated on the CPU and driving the stub posenet reproduces what the
    reference's loops left behind to RESTATEMENT_BOUND.
    The restatement that divides by the distance without the zero guard must fail.  On the stub alone it cannot: the 0 / 0 of the
    hip lands on the constant zeros the stub pads with and reaches no parameter (measured: the same 2.682e-7).  So both
    restatements also drive the stub with a learnable hip offset initialised to zero (posetrain_mpjpe_util.LearnableHip): with
    the guard the offset stays exactly 0 and the stub inside reproduces the fixture as before; without it the state is NaN."""
    torch.set_num_threads(1)
    for loop in MU.LOOPS:
        model = PU.load_initial(MU.make_model(loop), G, loop)
        losses, norms = MU.restated_mpjpe_loop(model, loop, PU.batches_of(G, loop))
        diff = PU.max_state_diff(model, G, loop)
        d_loss, d_norm = np.abs(losses / G[loop + "_losses"] - 1).max(), np.abs(norms / G[loop + "_norms"] - 1).max()
        print(loop, "restated vs fixture: state %.3e loss %.3e norm %.3e" % (diff, d_loss, d_norm))
        assert d_loss <= 1e-5 and d_norm <= 1e-5
        assert diff <= RESTATEMENT_BOUND, (loop, diff)
        moved = max(float(np.abs(G["%s_final_%s" % (loop, k)] - G["%s_init_%s" % (loop, k)]).max())
                    for k in ("a.weight", "b.weight", "c.weight"))
        assert moved >= 100 * RESTATEMENT_BOUND, (loop, moved)
        for guard in (True, False):
            hip = MU.LearnableHip(PU.load_initial(MU.make_model(loop), G, loop))
            h_losses, h_norms = MU.restated_mpjpe_loop(hip, loop, PU.batches_of(G, loop), guard=guard)
            h_diff = PU.max_state_diff(hip.stub, G, loop)
            if guard:
                assert np.array_equal(hip.hip.detach().numpy(), np.zeros(3, np.float32))
                assert h_diff == diff and np.array_equal(h_losses, losses) and np.array_equal(h_norms, norms)
            else:
                assert not h_diff <= RESTATEMENT_BOUND and np.isnan(hip.hip.detach().numpy()).all()
                assert all(np.isnan(a).all() for k, a in PU.state_arrays(hip.stub).items())
                assert np.isnan(h_norms).all()
