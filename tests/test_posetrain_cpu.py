"""CPU-side checks of the posenet training loop: the drop-ins' signatures, argument errors of the wrappers and of the C-ABI
(before any launch), and the fixture's self-consistency (tests/golden/posetrain.npz, recorded from the reference's loops)."""
import ctypes
import inspect
import os
import sys

import numpy as np
import pytest
import torch

import posetrain_util as PU

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# test_fixture_is_self_consistent: 10 x the measured difference between the restated fused arithmetic and the reference's final
# state (1.7e-6 on the single-frame loop, 1.8e-7 on the clips; 12 Adam steps, parameters of magnitude <= 1 moved by 1.2e-2)
RESTATEMENT_BOUND = 2e-5


@pytest.fixture(scope="module")
def built():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    ge.build_lib(verbose=False)
    import dhaug_amd
    return dhaug_amd


@pytest.fixture(scope="module")
def G():
    return PU.load_golden()


def test_drop_in_signatures_match_the_reference(built, G):
    from dhaug_amd.function_aug import model_pos_train as T
    from dhaug_amd.models_Fk_GAN import video_mode_operate as V
    for f in (T.train_posenet, V.video_mode_train_posenet, V.GAN_dataSet_video_mode_train_posenet):
        assert str(inspect.signature(f)) == str(G["sig_" + f.__name__][0]), f.__name__
    assert list(inspect.signature(T.posenet_optimizer).parameters) == ["model_pos", "lr"]


def test_wrappers_refuse_bad_shapes_and_cpu_tensors(built):
    from dhaug_amd import ops
    z = torch.zeros
    with pytest.raises(ValueError):
        ops.pair_batch(z(4, 16, 2), z(4, 16, 2))                      # 3D rows are not (16, 3)
    with pytest.raises(ValueError):
        ops.pair_batch(z(4, 16, 3), z(5, 16, 2))                      # row counts differ
    with pytest.raises(ValueError):
        ops.pair_batch(z(4, 16, 3), z(4, 16, 2), n=5)                 # more rows than there are
    with pytest.raises(ValueError):
        ops.pair_batch(z(4, 16, 3), z(4, 16, 2), idx=z(2, dtype=torch.int32))
    with pytest.raises(ValueError):
        ops.pose_mse(z(4, 16, 3), z(4, 15, 3), 4)
    with pytest.raises(ValueError):
        ops.adam_clip_step(z(8), z(7), z(8), z(8), z(1, dtype=torch.int32), None, 1.0)
    with pytest.raises(ValueError):
        ops.grad_sumsq(z(2, 4))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.pair_batch(z(4, 16, 3), z(4, 16, 2))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.pose_mse(z(4, 16, 3), z(4, 16, 3), 4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.grad_sumsq(z(8))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.adam_clip_step(z(8), z(8), z(8), z(8), z(1, dtype=torch.int32), None, 1.0)
    with pytest.raises(ValueError):
        ops.adam_clip_step(z(8), z(8), z(8), z(8), z(1, dtype=torch.int32), None, 0.0)


def test_posenet_adam_on_the_host(built):
    """construction, defaults and state_dict are host logic; a step needs the GPU and says so"""
    from dhaug_amd.function_aug.model_pos_train import posenet_optimizer, train_posenet
    from dhaug_amd.optim import FusedAdam, PosenetAdam
    net = PU.StubPosenet()
    opt = posenet_optimizer(net, 2e-3)
    assert isinstance(opt, PosenetAdam) and isinstance(opt, FusedAdam)
    g = opt.param_groups[0]
    assert g["lr"] == 2e-3 and tuple(g["betas"]) == (0.9, 0.999) and g["eps"] == 1e-8
    assert PosenetAdam(PU.StubPosenet().parameters()).param_groups[0]["lr"] == 1e-3
    assert all(p.data_ptr() >= opt.flat_param.data_ptr() for p in net.parameters()) and opt._packs is None
    sd = opt.state_dict()
    assert sd["dhaug_flat"]["step_count"] == 0
    opt.load_state_dict(sd)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        opt.clip_step(1.0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        train_posenet(net, [], opt, torch.nn.MSELoss(), torch.device("cpu"), PU.loop_args())


def test_c_abi_argument_errors(built):
    L = built._lib.lib()
    buf = (ctypes.c_float * 4096)()
    a16 = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)
    mis = ctypes.c_void_p(a16.value + 4)
    N = None
    # dhaug_pair_batch(p3, p2, M, F3, F2, idx, n, flip, playback, tgt, inp, tgt_flip, inp_flip, inp_back, inp_flip_back, stream)
    assert L.dhaug_pair_batch(a16, a16, 4, 1, 1, N, -1, 0, 0, a16, a16, N, N, N, N, N) == -1        # negative count
    assert L.dhaug_pair_batch(a16, a16, -4, 1, 1, N, 1, 0, 0, a16, a16, N, N, N, N, N) == -1
    assert L.dhaug_pair_batch(a16, a16, 4, 0, 1, N, 1, 0, 0, a16, a16, N, N, N, N, N) == -1         # no frames
    assert L.dhaug_pair_batch(N, a16, 4, 1, 1, N, 1, 0, 0, a16, a16, N, N, N, N, N) == -1           # tgt asked for, p3 NULL
    assert L.dhaug_pair_batch(a16, a16, 4, 1, 1, N, 1, 0, 0, N, N, N, N, N, N, N) == -1             # no output at all
    assert L.dhaug_pair_batch(a16, a16, 4, 1, 1, N, 1, 0, 0, a16, a16, a16, N, N, N, N) == -1       # tgt_flip without flip
    assert L.dhaug_pair_batch(a16, a16, 4, 1, 1, N, 1, 1, 0, a16, a16, a16, a16, a16, N, N) == -1   # inp_back without playback
    assert L.dhaug_pair_batch(a16, a16, 4, 1, 1, N, 5, 0, 0, a16, a16, N, N, N, N, N) == -1         # n > M without idx
    assert L.dhaug_pair_batch(a16, a16, 4, 1, 1, N, 0, 0, 0, a16, a16, N, N, N, N, N) == 0          # empty batch
    assert L.dhaug_pair_batch(a16, mis, 4, 1, 1, N, 1, 0, 0, a16, a16, N, N, N, N, N) == -2
    assert L.dhaug_pair_batch(a16, a16, 1 << 40, 1, 9, N, (1 << 31) // 48 // 9, 0, 0, a16, a16, N, N, N, N, N) == -3
    # dhaug_pose_mse(pred, tgt, numel, poses, grad, loss, meter, workspace, stream)
    assert L.dhaug_pose_mse(a16, a16, -1, 1, a16, a16, N, a16, N) == -1
    assert L.dhaug_pose_mse(a16, a16, 8, -1, a16, a16, N, a16, N) == -1
    assert L.dhaug_pose_mse(N, a16, 8, 1, a16, a16, N, a16, N) == -1
    assert L.dhaug_pose_mse(a16, a16, 8, 1, N, a16, N, a16, N) == -1
    assert L.dhaug_pose_mse(a16, a16, 8, 1, a16, N, N, a16, N) == -1
    assert L.dhaug_pose_mse(a16, a16, 8, 1, a16, a16, N, N, N) == -1
    assert L.dhaug_pose_mse(a16, a16, 0, 0, a16, a16, N, a16, N) == 0
    assert L.dhaug_pose_mse(a16, a16, 8, 1, a16, a16, mis, a16, N) == -2                                # meter not 8-byte aligned
    # dhaug_grad_sumsq(grad, n, grad_scale, workspace, step_counter, stream)
    assert L.dhaug_grad_sumsq(a16, -1, 1.0, a16, N, N) == -1
    assert L.dhaug_grad_sumsq(N, 8, 1.0, a16, N, N) == -1
    assert L.dhaug_grad_sumsq(a16, 8, 1.0, N, N, N) == -1
    assert L.dhaug_grad_sumsq(a16, 0, 1.0, a16, N, N) == 0
    # dhaug_adam_clip_step(p, g, m, v, n, lr, b1, b2, eps, step_dev, grad_scale, max_norm, workspace, norm_out, stream)
    step = lambda n, max_norm, p=a16, sd=a16, ws=a16: L.dhaug_adam_clip_step(p, a16, a16, a16, n, 1e-3, 0.9, 0.999, 1e-8, sd, 1.0,
                                                                               max_norm, ws, N, N)
    assert step(-1, 1.0) == -1
    assert step(8, 0.0) == -1 and step(8, -1.0) == -1 and step(8, float("nan")) == -1
    assert step(0, float("nan")) == -1                                                                  # also for an empty vector
    assert step(8, 1.0, p=N) == -1 and step(8, 1.0, sd=N) == -1 and step(8, 1.0, ws=N) == -1
    assert step(0, 1.0) == 0 and step(0, float("inf")) == 0


def test_fixture_is_self_consistent(G):
    """The arithmetic the kernels implement -- flat fp32 gradient, one global fp64 sum of squares, coef in fp32, Adam -- restated
    on the CPU (posetrain_util.restated_loop) and driving the stub posenet reproduces what the reference's loops left behind.
    Measured: the largest difference of any parameter or BatchNorm buffer is 1.7e-6 (train_posenet) and 1.8e-7 (the two clip
    loops) after 12 steps; the bound is 2e-5.  The two wrong restatements (coef not clamped: 3.9e-3 / 2.0e-3; every tensor clipped
    by its own norm: 5.8e-3 / 5.6e-3) must miss that bound by at least 10 x, and the recorded norms must lie on both sides of
    max_norm, or the fixture would pin nothing about clipping."""
    torch.set_num_threads(1)
    for loop in PU.LOOPS:
        norms = G[loop + "_norms"]
        assert len(norms) == 12 and (norms < 0.8).sum() >= 4 and (norms > 2.0).sum() >= 4, (loop, norms)
        diff = {}
        for variant in ("fused", "noclamp", "pertensor"):
            model = PU.load_initial(PU.make_model(loop), G, loop)
            losses, got_norms = PU.restated_loop(model, loop, PU.batches_of(G, loop), variant)
            diff[variant] = PU.max_state_diff(model, G, loop)
            if variant == "fused":
                assert np.abs(losses / G[loop + "_losses"] - 1).max() <= 1e-5
                assert np.abs(got_norms / norms - 1).max() <= 1e-5
        print(loop, diff)
        assert diff["fused"] <= RESTATEMENT_BOUND, (loop, diff)
        assert diff["noclamp"] >= 10 * RESTATEMENT_BOUND and diff["pertensor"] >= 10 * RESTATEMENT_BOUND, (loop, diff)
        moved = max(float(np.abs(G["%s_final_%s" % (loop, k)] - G["%s_init_%s" % (loop, k)]).max())
                    for k in ("a.weight", "b.weight", "c.weight"))
        assert moved >= 100 * RESTATEMENT_BOUND, (loop, moved)
