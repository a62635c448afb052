"""CPU-only checks of the detailed pose errors (mpjpe_byjoint, weighted_mpjpe, n_mpjpe, mean_velocity_error): the fixture
tests/golden/pose_eval_detail.npz, recorded from the reference, is what the fp64 formulas of tests/eval_detail_util.py give;
every ValueError is raised before anything touches a GPU; both C entries return their argument errors; the binding's
constants are the header's."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

import eval_detail_util as DU

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def built():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    ge.build_lib(verbose=False)
    import dhaug_amd
    return dhaug_amd


@pytest.fixture(scope="module")
def G():
    z = np.load(os.path.join(ROOT, "tests", "golden", "pose_eval_detail.npz"))
    return {k: z[k] for k in z.files}


def test_fixture_holds_the_fp64_formulas(G):
    """the reference's fp64 results are the four formulas: mean over the first axis only, broadcast weights, the per-frame
    scale, np.diff along axis 0 -- to the roundoff bounds of eval_detail_util (two fp64 evaluations of the same formula)"""
    assert list(G["cases"]) == ["noisy", "similarity", "millimetres", "kilometres"]
    for case in G["cases"]:
        for k, (ref, bound) in DU.fixture_restated(G, case).items():
            r32, r64 = G["%s_%s_ref32" % (case, k)], G["%s_%s_ref64" % (case, k)]
            assert r32.dtype == np.float32 and r64.dtype == np.float64 and r32.shape == r64.shape == np.shape(ref)
            assert np.all(np.isfinite(r32)) and np.all(np.isfinite(r64))
            err = np.abs(r64 - ref)
            print(case, k, "max |ref64 - formula| / bound = %.3g" % float(np.max(err / bound)))
            assert np.all(err <= bound), (case, k)
    assert G["noisy_bj3_ref64"].shape == (16,) and G["noisy_bj4_ref64"].shape == (4, 16)
    assert str(G["sig_weighted_mpjpe"][0]) == "(predicted, target, w)"
    for f in ("mpjpe_byjoint", "n_mpjpe", "mean_velocity_error"):
        assert str(G["sig_" + f][0]) == "(predicted, target)"
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "pose_eval_detail.npz")) < 400 * 1024


def test_signatures_are_the_reference_s(built, G):
    import inspect
    from dhaug_amd.utils import loss
    for f in ("mpjpe_byjoint", "weighted_mpjpe", "n_mpjpe", "mean_velocity_error"):
        assert str(inspect.signature(getattr(loss, f))) == str(G["sig_" + f][0])


def test_bad_shapes_raise_before_any_launch(built):
    """every ValueError of the four functions, on a machine without a GPU: nothing is uploaded or launched before the checks"""
    from dhaug_amd.utils import loss as L
    z = lambda *s: torch.zeros(*s)
    for f in (L.mpjpe_byjoint, L.n_mpjpe, L.mean_velocity_error):
        with pytest.raises(ValueError):
            f(z(4, 2, 16, 3), z(4, 3, 16, 3))                     # shapes differ
        with pytest.raises(ValueError):
            f(z(4, 2, 17, 3), z(4, 2, 17, 3))                     # not 16 joints
        with pytest.raises(ValueError):
            f(np.zeros((4, 2, 16, 2), np.float32), np.zeros((4, 2, 16, 2), np.float32))
    with pytest.raises(ValueError):
        L.weighted_mpjpe(z(4, 17, 3), z(4, 17, 3), z(4, 1))
    with pytest.raises(ValueError):
        L.weighted_mpjpe(z(4, 16, 3), z(5, 16, 3), z(4, 1))
    # n_mpjpe: exactly 4-D
    for s in ((8, 16, 3), (16, 3), (2, 2, 2, 16, 3)):
        with pytest.raises(ValueError):
            L.n_mpjpe(z(*s), z(*s))
    # weighted_mpjpe: torch broadcasting against predicted.shape[:-1], first dimensions equal, no enlargement
    p = z(6, 5, 16, 3)
    for w in (z(6), z(6, 5), z(5, 16), z(1, 5, 16), z(()), z(6, 5, 16, 1), z(6, 5, 3)):
        with pytest.raises(ValueError):
            L.weighted_mpjpe(p, p, w)
    with pytest.raises(ValueError):
        L.weighted_mpjpe(z(6, 1, 16, 3), z(6, 1, 16, 3), z(6, 5, 16))    # would enlarge the result
    with pytest.raises(ValueError):
        L.weighted_mpjpe(z(8, 16, 3), z(8, 16, 3), z(8))
    # mean_velocity_error: a frame axis in front of the pose
    with pytest.raises(ValueError):
        L.mean_velocity_error(np.zeros((16, 3), np.float32), np.zeros((16, 3), np.float32))
    # more columns than the kernel takes
    from dhaug_amd import _lib
    wide = z(2, _lib.COLERR_MAX_COLS // 16 + 1, 16, 3)
    with pytest.raises(ValueError):
        L.mpjpe_byjoint(wide, wide)
    with pytest.raises(ValueError):
        L.mean_velocity_error(wide, wide)


def test_one_frame_velocity_is_nan_without_a_launch(built):
    from dhaug_amd import _lib
    from dhaug_amd.utils import loss as L
    calls = _lib.CALLS[0]
    a32, a64 = np.zeros((1, 16, 3), np.float32), np.zeros((1, 4, 16, 3), np.float64)
    r = L.mean_velocity_error(a32, a32)
    assert isinstance(r, np.float32) and np.isnan(r)
    r = L.mean_velocity_error(a64, a64)
    assert isinstance(r, np.float64) and np.isnan(r)
    r = L.mean_velocity_error(torch.zeros(1, 16, 3), torch.zeros(1, 16, 3, dtype=torch.float64))
    assert isinstance(r, np.float64) and np.isnan(r)
    assert _lib.CALLS[0] == calls


def test_ops_refuse_cpu_tensors(built):
    from dhaug_amd import ops
    p = torch.zeros(4, 16, 3)
    with pytest.raises(RuntimeError):
        ops.pose_column_errors(p, p, col_sums=torch.zeros(16, dtype=torch.float64))
    with pytest.raises(RuntimeError):
        ops.pose_scaled_errors(p, p)
    with pytest.raises(ValueError):
        ops.pose_column_errors(p, p)                              # nothing asked for
    with pytest.raises(ValueError):
        ops.pose_column_errors(torch.zeros(4, 6, 3), torch.zeros(4, 6, 3), col_sums=torch.zeros(6, dtype=torch.float64))
    with pytest.raises(ValueError):
        ops.pose_scaled_errors(p, p, w=torch.zeros(5))


def test_argument_errors_are_returned_not_thrown(built):
    """both entries validate before any device work: every pointer here is a HOST address, so a call that got as far as a launch
    would return a HIP error, not -1 / -2 / -3"""
    L = built._lib.lib()
    EINVAL, EALIGN, EUNSUPPORTED = -1, -2, -3
    buf = (ctypes.c_double * 1024)()
    base = (ctypes.addressof(buf) + 15) & ~15
    a = ctypes.c_void_p(base)
    off = lambda n: ctypes.c_void_p(base + n)
    col = L.dhaug_pose_column_errors
    assert col(a, a, -1, 16, 0, a, a, a, None) == EINVAL
    assert col(a, a, 4, -16, 0, a, a, a, None) == EINVAL
    assert col(a, a, 4, 16, 0, None, None, a, None) == EINVAL          # neither col_sums nor vel_sum
    assert col(a, a, 4, 16, 0, a, a, None, None) == EINVAL             # no workspace
    assert col(a, a, 4, 20, 1, a, a, a, None) == EINVAL                # centring needs whole poses
    assert col(None, a, 4, 16, 0, a, a, a, None) == EINVAL
    assert col(a, None, 4, 16, 0, a, None, a, None) == EINVAL
    assert col(a, a, 4, built._lib.COLERR_MAX_COLS + 16, 0, a, a, a, None) == EUNSUPPORTED
    assert col(a, a, 4, 18, 0, a, a, a, None) == EUNSUPPORTED          # columns move as quads
    assert col(a, a, 1 << 31, 16, 0, a, a, a, None) == EUNSUPPORTED
    assert col(off(4), a, 4, 16, 0, a, a, a, None) == EALIGN
    assert col(a, off(8), 4, 16, 0, a, a, a, None) == EALIGN
    assert col(a, a, 4, 16, 0, off(4), a, a, None) == EALIGN
    assert col(a, a, 4, 16, 0, a, off(4), a, None) == EALIGN
    assert col(a, a, 4, 16, 0, a, a, off(4), None) == EALIGN
    assert col(None, None, 0, 16, 0, a, None, a, None) == 0            # zero-sized calls look at no pointer
    assert col(None, None, 4, 0, 1, None, a, a, None) == 0
    sc = L.dhaug_pose_scaled_errors
    assert sc(a, a, -1, 0, None, 0, a, a, None) == EINVAL
    assert sc(a, a, 4, 0, None, 0, None, a, None) == EINVAL
    assert sc(a, a, 4, 0, None, 0, a, None, None) == EINVAL
    assert sc(None, a, 4, 0, None, 0, a, a, None) == EINVAL
    assert sc(a, None, 4, 1, a, 1, a, a, None) == EINVAL
    assert sc(a, a, 1 << 31, 0, None, 0, a, a, None) == EUNSUPPORTED
    assert sc(off(8), a, 4, 0, None, 0, a, a, None) == EALIGN
    assert sc(a, off(4), 4, 0, None, 0, a, a, None) == EALIGN
    assert sc(a, a, 4, 0, off(4), 1, a, a, None) == EALIGN             # per-joint weights move as float4
    assert sc(a, a, 4, 0, off(2), 0, a, a, None) == EALIGN
    assert sc(a, a, 4, 0, None, 0, off(4), a, None) == EALIGN
    assert sc(a, a, 4, 0, None, 0, a, off(4), None) == EALIGN
    assert sc(None, None, 0, 1, None, 0, a, a, None) == 0


def test_constants_mirror_the_header(built):
    """a short workspace is an out-of-bounds write on the device: the binding's sizes and caps are the header's"""
    lib = built._lib
    hdr = open(os.path.join(ROOT, "include", "dhaug.h")).read()
    defs = dict(re.findall(r"#define\s+(DHAUG_(?:COLERR|SCALEDERR)_\w+)\s+(.+)", hdr))

    def value(name):
        expr = re.sub(r"DHAUG_\w+", lambda m: "(%s)" % defs[m.group(0)], defs[name])
        expr = re.sub(r"DHAUG_\w+", lambda m: "(%s)" % defs[m.group(0)], expr)
        assert re.fullmatch(r"[0-9 ()*+]+", expr), expr
        return eval(expr)

    assert sorted(defs) == ["DHAUG_COLERR_MAX_BLOCKS", "DHAUG_COLERR_MAX_COLS", "DHAUG_COLERR_MIN_STEPS",
                            "DHAUG_COLERR_WORKSPACE_BYTES", "DHAUG_SCALEDERR_MAX_BLOCKS", "DHAUG_SCALEDERR_WORKSPACE_BYTES"]
    for name in defs:
        assert value(name) == getattr(lib, name[len("DHAUG_"):]), name
    assert lib.COLERR_MAX_COLS >= 16 * 243
    # the workspace holds a velocity partial per workgroup and a column partial per (slab, column): a workgroup covers at most
    # 1024 columns of its slab
    assert lib.COLERR_WORKSPACE_BYTES == 8 * (lib.COLERR_MAX_BLOCKS + lib.COLERR_MAX_BLOCKS * 1024)
    assert lib.SCALEDERR_WORKSPACE_BYTES == 8 * 2 * lib.SCALEDERR_MAX_BLOCKS
    src = open(os.path.join(os.path.dirname(lib.__file__), "csrc", "dhaug_eval_detail.hip")).read()
    for line in ("constexpr int kColMaxBlocks = DHAUG_COLERR_MAX_BLOCKS;", "constexpr int kColMinSteps = DHAUG_COLERR_MIN_STEPS;",
                 "constexpr int kPoseMaxGrid = DHAUG_SCALEDERR_MAX_BLOCKS;", "a.col_part = a.vel_part + kColMaxBlocks;"):
        assert src.count(line) == 1, line
