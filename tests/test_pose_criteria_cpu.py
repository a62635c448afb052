"""CPU-side checks of the N-MPJPE / weighted / per-joint criteria: the fp64 restatement of tests/pose_criteria_util.py against the
reference's own gradients (tests/golden/pose_criteria.npz), the fp64 part of the N-MPJPE bound against an extended-precision
evaluation, the argument errors of the three entry points (before any launch), and the dispatch rules of utils.loss and
StepRunner decided from attributes alone."""
import ctypes
import os
import sys
import types

import numpy as np
import pytest
import torch
import torch.nn as nn

import pose_criteria_util as CU

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EALIGN, EUNSUP = -1, -2, -3


@pytest.fixture(scope="module")
def built():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    ge.build_lib(verbose=False)
    import dhaug_amd
    return dhaug_amd


@pytest.fixture(scope="module")
def G():
    return CU.load_golden()


def kernel_test_inputs():
    """the (pred, target) pairs the GPU kernel test draws, at its smaller sizes (the same generator and seeds)"""
    for P in (1, 3, 63, 64, 65, 257):
        case = CU.make_case((P, 1, 16, 3), 1000 + P)
        yield case["pred"], case["target"]


# ------------------------------------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize("k", range(len(CU.SHAPES)))
def test_restatement_equals_the_reference_gradients(G, k):
    """the three formulas in fp64 against the reference's functions and torch's autograd of them, both in fp64 on the same
    inputs: equal to roundoff -- 1e-12 relative to the largest gradient element is thousands of fp64 roundings"""
    g = lambda name: G["a%d_%s" % (k, name)]
    y, x = g("pred"), g("target")
    assert y.dtype == np.float32 and y.shape == CU.SHAPES[k]

    def close(got, want, what):
        got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
        err = float(np.abs(got - want).max() / np.abs(want).max())
        print("restatement %s case %d: %.3e of the largest element" % (what, k, err))
        assert got.shape == want.shape and err <= 1e-12, what

    loss, grad, _ = CU.nmpjpe(y, x)
    close(loss, g("n_value"), "n value")
    close(grad, g("n_grad"), "n grad")
    for c, w in (("wp", g("w_pose")), ("wj", g("w_joint")), ("w16", g("w16"))):
        loss, grad = CU.wmpjpe(y, x, w)
        close(loss, g(c + "_value"), c + " value")
        close(grad, g(c + "_grad"), c + " grad")
        assert CU.weighted_sum_survives(y, x, w)
    value, grad = CU.byjoint(y, x, g("cot"))
    close(value, g("bj_value"), "bj value")
    close(grad, g("bj_grad"), "bj grad")
    assert (np.sign(g("w_joint")) < 0).any() and (np.sign(g("w_joint")) > 0).any()          # signs mixed


def test_fp64_part_of_the_nmpjpe_bound_holds_without_the_kernel():
    """the N-MPJPE gradient evaluated in np.longdouble stays within the ABSOLUTE term alone (K u T_k / J) of its fp64 evaluation,
    on the inputs the kernel test uses and on the golden's: the bound's fp64 part, with no kernel and no fp32 rounding in play"""
    if np.finfo(np.longdouble).eps >= np.finfo(np.float64).eps:
        pytest.skip("np.longdouble is no wider than fp64 on this platform")
    worst = 0.0
    pairs = list(kernel_test_inputs()) + [(c["pred"], c["target"]) for c in (CU.make_case(s, 40 + k) for k, s in enumerate(CU.SHAPES))]
    for y, x in pairs:
        poses = y.size // 48
        l64, g64, T = CU.nmpjpe(y, x)
        lld, gld, _ = CU.nmpjpe(y, x, np.longdouble)
        term = CU.nmpjpe_abs_term(T, poses)
        share = float((np.abs((gld - g64.astype(np.longdouble)).astype(np.float64)) / term).max())
        worst = max(worst, share)
        assert np.isfinite(term).all() and share <= 1.0
        assert abs(float(lld) - float(l64)) <= 16 * poses * CU.U53 * float(l64) + 1e-300
    print("longdouble against fp64: largest share of the absolute term %.4f" % worst)


def test_zero_residual_rule_of_the_restatement():
    """p = 2 t: s = 0.5 and r = 0 exactly, a zero gradient and a zero loss; a single coincident joint gets a zero gradient in
    the weighted and per-joint forms"""
    case = CU.make_case((3, 2, 16, 3), 7)
    x = case["target"]
    loss, grad, _ = CU.nmpjpe(2 * x, x)
    assert loss == 0 and not grad.any()
    y = case["pred"].copy()
    y[1, 0, 5] = x[1, 0, 5]
    _, gw = CU.wmpjpe(y, x, case["w_joint"])
    _, gb = CU.byjoint(y, x, case["cot"])
    for g in (gw, gb):
        assert not g[1, 0, 5].any() and np.isfinite(g).all() and (np.abs(g).sum(-1) > 0).sum() == 3 * 2 * 16 - 1


# ------------------------------------------------------------------------------------------------------- argument errors
def test_argument_errors_come_before_any_launch(built):
    """the three entry points (csrc/dhaug_pose_criteria.hip): a bad argument comes back as the documented code before any launch
    -- every pointer here is a valid HOST address, so a call that got as far as a launch would return a HIP error -- and an empty
    batch is a no-op that looks at no pointer"""
    L = built._lib.lib()
    buf = (ctypes.c_float * 8192)()
    base = (ctypes.addressof(buf) + 15) & ~15
    a, b, c, d, e = (ctypes.c_void_p(base + 4096 * i) for i in range(5))
    w = ctypes.c_void_p(base + 4096 * 5)
    ws, meter = ctypes.c_void_p(base + 4096 * 6), ctypes.c_void_p(base + 4096 * 7)
    odd2, odd4 = ctypes.c_void_p(base + 2), ctypes.c_void_p(base + 4)

    def n(pred=a, tgt=b, P=4, poses=4, grad=c, loss=d, meter=meter, ws=ws):
        return L.dhaug_pose_nmpjpe(pred, tgt, P, poses, grad, loss, meter, ws, None)

    def wm(pred=a, tgt=b, P=4, w=w, mode=1, poses=4, grad=c, loss=d, meter=meter, ws=ws):
        return L.dhaug_pose_wmpjpe(pred, tgt, P, w, mode, poses, grad, loss, meter, ws, None)

    for f in (n, wm):
        assert f(P=-1) == EINVAL and f(poses=-1) == EINVAL
        assert f(grad=None) == EINVAL and f(loss=None) == EINVAL and f(ws=None) == EINVAL
        assert f(pred=None) == EINVAL and f(tgt=None) == EINVAL
        assert f(P=1 << 31) == EUNSUP
        assert f(pred=odd2) == EALIGN and f(tgt=odd2) == EALIGN and f(grad=odd2) == EALIGN and f(loss=odd2) == EALIGN
        assert f(ws=odd4) == EALIGN and f(meter=odd4) == EALIGN
        assert f(P=0, pred=None, tgt=None) == 0                   # a no-op that looks at no pointer
    assert wm(w=None) == EINVAL and wm(w=None, P=0) == EINVAL
    for mode in (0, 4, -1):
        assert wm(mode=mode) == EINVAL and wm(mode=mode, P=0) == EINVAL
    assert wm(w=odd2, mode=1) == EALIGN and wm(w=odd2, mode=3) == EALIGN
    assert wm(w=odd4, mode=2) == EALIGN                           # the per-joint weights are read as float4

    def bj(pred=a, tgt=b, rows=4, cols=16, cot=e, grad=c):
        return L.dhaug_pose_byjoint_backward(pred, tgt, rows, cols, cot, grad, None)

    assert bj(rows=-1) == EINVAL and bj(cols=-1) == EINVAL
    assert bj(pred=None) == EINVAL and bj(tgt=None) == EINVAL and bj(cot=None) == EINVAL and bj(grad=None) == EINVAL
    assert bj(rows=1 << 31) == EUNSUP and bj(cols=1 << 31) == EUNSUP
    assert bj(pred=odd2) == EALIGN and bj(tgt=odd2) == EALIGN and bj(cot=odd2) == EALIGN and bj(grad=odd2) == EALIGN
    assert bj(rows=0, pred=None, grad=None) == 0 and bj(cols=0, cot=None) == 0


def test_binding_and_constants(built):
    from dhaug_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "dhaug.h")).read()
    for name, value in (("PER_POSE", _lib.WMPJPE_PER_POSE), ("PER_JOINT", _lib.WMPJPE_PER_JOINT), ("SHARED", _lib.WMPJPE_SHARED)):
        assert "#define DHAUG_WMPJPE_%s %d\n" % (name, value) in hdr
    for name in ("dhaug_pose_nmpjpe", "dhaug_pose_wmpjpe", "dhaug_pose_byjoint_backward"):
        assert name in _lib.SIGNATURES and ("int %s(" % name) in hdr
    # the partials of the criteria kernels fit the training workspace
    src = open(os.path.join(os.path.dirname(_lib.__file__), "csrc", "dhaug_pose_criteria.hip")).read()
    assert "constexpr int kMaxGrid = 2048;" in src and _lib.POSETRAIN_WORKSPACE_BYTES == 2048 * 8


# ------------------------------------------------------------------------------------------------------------- dispatch
def _stub(is_cuda=True, dtype=torch.float32, requires_grad=True):
    return types.SimpleNamespace(is_cuda=is_cuda, dtype=dtype, requires_grad=requires_grad)


def test_dispatch_is_decided_from_attributes_alone(built):
    """utils.loss.takes_criterion_kernel: an fp32 device tensor that requires grad, gradients enabled, no other operand asking
    for a gradient, the shape limits holding -- and nothing else"""
    from dhaug_amd.utils import loss as L
    take = L.takes_criterion_kernel
    quiet = _stub(requires_grad=False)
    with torch.enable_grad():
        assert take(_stub(), (quiet,)) and take(_stub(), (quiet, quiet)) and take(_stub(), (np.zeros(3),))
        assert not take(_stub(is_cuda=False), (quiet,))                              # host inputs
        assert not take(_stub(dtype=torch.float64), (quiet,))                        # fp64
        assert not take(_stub(dtype=torch.float16), (quiet,))
        assert not take(_stub(requires_grad=False), (quiet,))                        # no gradient asked for
        assert not take(_stub(), (_stub(),)) and not take(_stub(), (quiet, _stub()))  # target or w asks for one
        assert not take(_stub(), (quiet,), within_limits=False)                      # the metric kernel's shape limits
        assert not take(np.zeros((4, 16, 3), np.float32), ())
        with torch.no_grad():
            assert not take(_stub(), (quiet,))
    # host tensors that require grad keep what they did: the plain-torch expression, with a grad_fn, no GPU touched
    p = torch.randn(4, 2, 16, 3, requires_grad=True)
    t = torch.randn(4, 2, 16, 3)
    for v in (L.n_mpjpe(p, t), L.weighted_mpjpe(p, t, torch.rand(4, 2, 1)), L.mpjpe_byjoint(p, t)):
        assert v.grad_fn is not None and not v.is_cuda
    with pytest.raises(ValueError, match="B, F, 16, 3"):
        L.n_mpjpe(p[0], t[0])


def test_joint_weighted_mpjpe_object(built):
    from dhaug_amd.utils import loss as L
    w = L.JointWeightedMpjpe(CU.LOOP_W16)
    assert w.weights.dtype == torch.float32 and tuple(w.weights.shape) == (16,) and not w.weights.is_cuda
    assert torch.equal(w.weights, torch.from_numpy(CU.LOOP_W16))
    assert w.buffer("cpu") is w.buffer(torch.device("cpu"))
    for bad in (np.ones(15), np.ones((2, 16)), []):
        with pytest.raises(ValueError, match="sixteen"):
            L.JointWeightedMpjpe(bad)
    # a host prediction that requires grad: weighted_mpjpe's plain-torch expression with the expanded weights
    p = torch.randn(3, 2, 16, 3, requires_grad=True)
    t = torch.randn(3, 2, 16, 3)
    v = w(p, t)
    assert v.grad_fn is not None and torch.equal(v, CU.torch_weighted_mpjpe(p, t, w.weights.expand(3, 2, 16)))
    with pytest.raises(ValueError, match="16, 3"):
        w(p[..., :2], t[..., :2])


def test_step_runner_classifies_the_criterion_from_the_object(built):
    from dhaug_amd.function_aug import model_pos_train as T
    from dhaug_amd.utils import loss as L
    f = T.fused_criterion
    assert f(nn.MSELoss(reduction="mean")) == "mse" and f(L.mpjpe) == "mpjpe" and f(L.n_mpjpe) == "n_mpjpe"
    assert f(L.JointWeightedMpjpe(np.ones(16))) == "wmpjpe"
    for other in (nn.MSELoss(reduction="sum"), nn.L1Loss(), lambda a, b: L.n_mpjpe(a, b), L.weighted_mpjpe, L.mpjpe_byjoint,
                  L.mean_velocity_error, CU.torch_n_mpjpe, L.JointWeightedMpjpe):
        assert f(other) is None
    from dhaug_amd import ops
    per_pose, per_joint, shared = 1, 2, 3
    assert ops.wmpjpe_mode((5, 3, 1), (5, 3, 16)) == per_pose and ops.wmpjpe_mode((5, 3, 16), (5, 3, 16)) == per_joint
    assert ops.wmpjpe_mode((16,), (5, 3, 16)) == shared and ops.wmpjpe_mode((16,), (16,)) == per_joint
    assert ops.wmpjpe_mode((5, 1, 16), (5, 3, 16)) is None and ops.wmpjpe_mode((5,), (5, 3, 16)) is None
