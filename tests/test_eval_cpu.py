"""CPU checks of the device-side posenet evaluation (no GPU needed): argument errors raise before any launch, the C-ABI
returns DHAUG_EINVAL for bad counts, the drop-ins keep the reference's signatures (recorded in tests/golden/pose_eval.npz),
and the fixture's recorded values agree with each other."""
import ctypes
import inspect
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1


@pytest.fixture(scope="module")
def G():
    z = np.load(os.path.join(ROOT, "tests", "golden", "pose_eval.npz"))
    return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def M():
    sys.path.insert(0, ROOT)
    from dhaug_amd.utils import loss
    from dhaug_amd.function_aug import model_pos_eval
    from dhaug_amd.models_Fk_GAN import video_mode_operate
    return loss, model_pos_eval, video_mode_operate


def test_shape_errors_raise_value_error(M):
    L = M[0]
    a, b = np.zeros((4, 16, 3), np.float32), np.zeros((4, 17, 3), np.float32)
    for f in (L.p_mpjpe, L.mpjpe):
        with pytest.raises(ValueError):
            f(a, b)
        with pytest.raises(ValueError):
            f(b, b)
    for f in (L.compute_PCK, L.compute_AUC):
        with pytest.raises(ValueError):
            f(a, b)
        with pytest.raises(ValueError):
            f(np.zeros((4, 14, 3)), np.zeros((4, 14, 3)))
    with pytest.raises(ValueError):
        L.compute_PCK(a, a, eval_joints=[0, 16])
    from dhaug_amd import ops
    with pytest.raises(ValueError):
        ops.pose_metrics(torch.zeros(2, 16, 3), torch.zeros(2, 15, 3), per_pose=True)
    with pytest.raises(ValueError):
        ops.pose_metrics(torch.zeros(2, 16, 3), torch.zeros(2, 16, 3), thresholds=range(33), per_pose=True)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.pose_metrics(torch.zeros(2, 16, 3), torch.zeros(2, 16, 3), per_pose=True)


def test_c_abi_returns_einval_for_bad_counts():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    ge.build_lib(verbose=False)
    import dhaug_amd
    L = dhaug_amd._lib.lib()
    f = L.dhaug_pose_metrics
    buf = (ctypes.c_float * 256)()
    a = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)
    thr = (ctypes.c_double * 40)(*range(40))
    bad = (ctypes.c_int32 * 16)(*([1] * 15 + [-1]))
    big = (ctypes.c_int32 * 16)(*([1] * 15 + [1025]))
    ok = (ctypes.c_int32 * 16)(*([2] * 16))
    # (pred, target, P, center, thresholds, nthr, multiplicity, mpjpe, pmpjpe, totals, workspace, stream); nothing launches
    assert f(a, a, -1, 0, thr, 1, None, a, None, None, None, None) == EINVAL
    assert f(a, a, 0, 0, thr, 33, None, a, None, None, None, None) == EINVAL
    assert f(a, a, 0, 0, thr, -1, None, a, None, None, None, None) == EINVAL
    assert f(a, a, 0, 0, None, 3, None, a, None, None, None, None) == EINVAL
    assert f(a, a, 0, 0, thr, 3, bad, a, None, None, None, None) == EINVAL
    assert f(a, a, 0, 0, thr, 3, big, a, None, None, None, None) == EINVAL
    assert f(a, a, 0, 0, thr, 3, None, None, None, None, None, None) == EINVAL      # no output
    assert f(a, a, 0, 0, thr, 3, None, None, None, a, None, None) == EINVAL         # totals without a workspace
    assert f(None, None, 4, 0, thr, 3, None, a, None, None, None, None) == EINVAL
    assert f(a, a, 0, 1, thr, 32, ok, a, a, a, a, None) == 0                         # P = 0: valid, nothing to do


def test_signatures_match_the_reference(M, G):
    L, E, V = M
    for name, f in (("mpjpe", L.mpjpe), ("p_mpjpe", L.p_mpjpe), ("compute_PCK", L.compute_PCK),
                    ("compute_AUC", L.compute_AUC), ("evaluate", E.evaluate), ("evaluate_posenet", E.evaluate_posenet),
                    ("video_mode_evaluate", V.video_mode_evaluate),
                    ("video_mode_evaluate_posenet", V.video_mode_evaluate_posenet)):
        assert str(inspect.signature(f)) == str(G["sig_" + name][0]), name


def test_fixture_is_self_consistent(G):
    import eval_util as EU
    cases = sorted(k[2:-5] for k in G if k.startswith("m_") and k.endswith("_pred"))
    assert set(cases) == set(EU.metric_cases())
    for c in cases:
        k = "m_" + c
        y, x = G[k + "_pred"], G[k + "_target"]
        assert y.dtype == np.float32 and y.shape == x.shape and y.shape[1:] == (16, 3) and 64 <= len(y) <= 256
        assert float(G[k + "_pcks"][30]) == float(G[k + "_pck"])
        assert abs(np.mean(G[k + "_pcks"]) - float(G[k + "_auc"])) <= 1e-12 * max(1.0, float(G[k + "_auc"]))
        assert np.all(np.isfinite(G[k + "_pp64"]))
        np.testing.assert_allclose(G[k + "_pp32"], G[k + "_pp64"], rtol=1e-3, atol=1e-6 * np.abs(x).max())
        np.testing.assert_allclose(float(G[k + "_p2"]), G[k + "_pp64"].mean(), rtol=1e-4, atol=1e-6 * np.abs(x).max())
        # the reference's PCK at 150 from the stored inputs, recomputed the numpy way
        e = np.sqrt(np.sum(np.power(y - x, 2), 2)) * 1000
        assert float(np.mean(e < 150) * 100) == pytest.approx(float(G[k + "_pck"]), abs=1e-9)
    assert np.array_equal(np.isnan(G["z_pp64"]), G["z_raised"] == 1) and G["z_raised"][:8].all() and not G["z_raised"][8:].any()
    assert np.allclose(G["m_millimetres_pp64"] / 1000, G["m_kilometres_pp64"] * 1000, rtol=1e-5)
    assert G["m_similarity_pp64"].max() < 1e-5
    assert list(G["w_steps"]) == [7] * 8 and len(G["w_names"]) == 8
    assert np.allclose(G["ep_result"], np.concatenate([G["e_s1000_noflip_0"][:2], G["e_s700_flip_1"]]))
    assert G["v_b3d"].shape[0] == sum(EU.VIDEO_LENGTHS) and G["v_sizes"].sum() == sum(EU.VIDEO_LENGTHS)
