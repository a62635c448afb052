"""The three criteria entry points on the GPU through the C-ABI -- dhaug_pose_nmpjpe, dhaug_pose_wmpjpe and
dhaug_pose_byjoint_backward -- against the fp64 restatement and the bounds of tests/pose_criteria_util.py.  Outputs are pre-filled
with NaN, with a guard word on either side of grad."""
import argparse
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

import pose_criteria_util as CU

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

GUARD = 12345.0
# 2048 * 64 + 1 poses: the grid (2048 workgroups of 64 poses) takes a second trip with one ragged workgroup
POSES = [1, 3, 63, 64, 65, 257, 2048 * 64 + 1]
BYJOINT = [(1, 16), (3, 4), (7, 16 * 3), (5, 16 * 243), (1029, 16), (3, 5), (1, 1)]     # the last two: a rows * cols % 4 tail


@pytest.fixture(scope="module")
def M():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    sys.path.insert(0, ROOT)
    import dhaug_amd
    from dhaug_amd import ops
    return argparse.Namespace(L=dhaug_amd._lib.lib(), ops=ops)


def ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def place(a, off):
    """the fp32 array on the device, `off` floats past a 16-byte boundary"""
    a = np.ascontiguousarray(a, dtype=np.float32)
    buf = torch.empty(a.size + 4, dtype=torch.float32, device="cuda")
    t = buf[off:off + a.size].view(a.shape)
    t.copy_(torch.from_numpy(a))
    assert t.data_ptr() % 16 == 4 * off
    return t


class Out:
    """grad (NaN-filled, `off` floats past a 16-byte boundary, a guard word on either side) and loss (NaN)"""

    def __init__(self, shape, off):
        n = int(np.prod(shape))
        self.buf = torch.full((n + 12,), float("nan"), device="cuda")
        self.lo, self.hi = 4 + off - 1, 4 + off + n
        self.buf[self.lo] = GUARD
        self.buf[self.hi] = GUARD
        self.grad = self.buf[self.lo + 1:self.hi].view(shape)
        assert self.grad.data_ptr() % 16 == 4 * off
        self.loss = torch.full((1,), float("nan"), device="cuda")

    def check(self):
        assert float(self.buf[self.lo]) == GUARD and float(self.buf[self.hi]) == GUARD
        assert bool(torch.isnan(self.buf[:self.lo]).all()) and bool(torch.isnan(self.buf[self.hi + 1:]).all())
        return self.grad.cpu().double().numpy(), float(self.loss.cpu().double()[0])


def run_n(M, y, x, off, poses=None, meter=None, ws=None):
    P = y.numel() // 48
    out = Out(tuple(y.shape), off)
    ws = M.ops.posetrain_workspace() if ws is None else ws
    rc = M.L.dhaug_pose_nmpjpe(ptr(y), ptr(x), P, P if poses is None else poses, ptr(out.grad), ptr(out.loss), ptr(meter), ptr(ws),
                               stream())
    assert rc == 0
    return out


def run_w(M, y, x, w, mode, off, poses=None, meter=None, ws=None):
    P = y.numel() // 48
    out = Out(tuple(y.shape), off)
    ws = M.ops.posetrain_workspace() if ws is None else ws
    rc = M.L.dhaug_pose_wmpjpe(ptr(y), ptr(x), P, ptr(w), mode, P if poses is None else poses, ptr(out.grad), ptr(out.loss),
                               ptr(meter), ptr(ws), stream())
    assert rc == 0
    return out


def run_bj(M, y, x, cot, off):
    out = Out(tuple(y.shape), off)
    cols = int(np.prod(y.shape[1:-1]))
    rc = M.L.dhaug_pose_byjoint_backward(ptr(y), ptr(x), y.shape[0], cols, ptr(cot), ptr(out.grad), stream())
    assert rc == 0
    return out


_cases = {}


def case_of(P):
    """inputs and fp64 references of P poses, made once and only read (test_pose_criteria_cpu.py evaluates the same inputs in
    extended precision)"""
    if P not in _cases:
        c = CU.make_case((P, 1, 16, 3), 1000 + P)
        c["n"] = CU.nmpjpe(c["pred"], c["target"])
        _cases[P] = c
    return _cases[P]


WEIGHTS = ((1, "w_pose"), (2, "w_joint"), (3, "w16"))


# ------------------------------------------------------------------------------------------------- against the restatement
@pytest.mark.parametrize("P", POSES)
def test_nmpjpe_against_fp64(M, P):
    """every gradient element within 1 ulp32 + K u T_k / J of the fp64 formula, the loss within 1 ulp32; the float4 path and the
    scalar one give the same bits"""
    c = case_of(P)
    l64, g64, T = c["n"]
    bound = CU.nmpjpe_bound(g64, T, P)
    got = []
    for off in (0, 1):
        grad, loss = run_n(M, place(c["pred"], off), place(c["target"], off), off).check()
        err = np.abs(grad - g64)
        share, ulps = float((err / bound).max()), float((err / CU.ulp32(g64)).max())
        lerr = abs(loss - float(l64)) / float(CU.ulp32(l64))
        print("pose_nmpjpe P=%d off=%d: grad %.3f of the bound (%.3f ulp32), loss %.3f ulp32" % (P, off, share, ulps, lerr))
        assert share <= 1.0 and lerr <= 1.0
        got.append((grad, loss))
    assert np.array_equal(got[0][0], got[1][0]) and got[0][1] == got[1][1]


@pytest.mark.parametrize("P", POSES)
def test_wmpjpe_against_fp64(M, P):
    """every w_mode: gradient and loss within 1 ulp32 of the fp64 formula"""
    c = case_of(P)
    for mode, key in WEIGHTS:
        l64, g64 = CU.wmpjpe(c["pred"], c["target"], c[key])
        assert CU.weighted_sum_survives(c["pred"], c["target"], c[key])
        for off in (0, 1):
            w = place(c[key], 0 if mode == 2 else off)            # the per-joint weights are 16-byte aligned by contract
            grad, loss = run_w(M, place(c["pred"], off), place(c["target"], off), w, mode, off).check()
            err = float((np.abs(grad - g64) / CU.ulp32(g64)).max())
            lerr = abs(loss - float(l64)) / float(CU.ulp32(l64))
            print("pose_wmpjpe P=%d mode=%d off=%d: grad %.3f ulp32, loss %.3f ulp32" % (P, mode, off, err, lerr))
            assert err <= 1.0 and lerr <= 1.0


@pytest.mark.parametrize("rows,cols", BYJOINT)
def test_byjoint_backward_against_fp64(M, rows, cols):
    rng = np.random.default_rng(rows * 7919 + cols)
    x = rng.normal(0, 1, (rows, cols, 3)).astype(np.float32)
    y = (x + rng.normal(0, 0.4, x.shape)).astype(np.float32)
    cot = rng.normal(0, 1, (cols,)).astype(np.float32)
    _, g64 = CU.byjoint(y, x, cot)
    for off in (0, 1):
        grad, _ = run_bj(M, place(y, off), place(x, off), place(cot, off), off).check()
        err = float((np.abs(grad - g64) / CU.ulp32(g64)).max())
        print("pose_byjoint_backward rows=%d cols=%d off=%d: %.3f ulp32" % (rows, cols, off, err))
        assert err <= 1.0


# --------------------------------------------------------------------------------------------------------- zero residuals
def test_exact_fit_up_to_scale_gets_zero_rows(M):
    """p = 2 t: s = 0.5 and r = 0 exactly -- all-zero gradient rows for those poses, finite values everywhere, and the other poses
    within their bound"""
    c = case_of(257)
    y, x = c["pred"][:70].copy(), c["target"][:70].copy()
    fit = [0, 5, 63, 64, 69]
    y[fit] = 2 * x[fit]
    l64, g64, T = CU.nmpjpe(y, x)
    for off in (0, 1):
        grad, loss = run_n(M, place(y, off), place(x, off), off).check()
        assert not grad[fit].any() and np.isfinite(grad).all() and np.isfinite(loss)
        rest = np.setdiff1d(np.arange(70), fit)
        assert (np.abs(grad - g64)[rest] <= CU.nmpjpe_bound(g64, T, 70)[rest]).all() and (np.abs(grad[rest]).sum((1, 2, 3)) > 0).all()
        assert abs(loss - float(l64)) <= float(CU.ulp32(l64))


def test_coincident_joint_gets_an_exact_zero(M):
    """a single joint at distance zero in the weighted and per-joint kernels: exact zeros there, nonzero elsewhere"""
    c = case_of(65)
    y, x = c["pred"].copy(), c["target"].copy()
    y[17, 0, 9] = x[17, 0, 9]
    y[64, 0, 15] = x[64, 0, 15]
    zero = np.zeros((65, 1, 16), dtype=bool)
    zero[17, 0, 9] = zero[64, 0, 15] = True
    cot = np.linspace(-1.0, 1.0, 16).astype(np.float32) + np.float32(0.03)
    for off in (0, 1):
        outs = [run_w(M, place(y, off), place(x, off), place(c[key], 0 if mode == 2 else off), mode, off).check()[0]
                for mode, key in WEIGHTS]
        outs.append(run_bj(M, place(y, off), place(x, off), place(cot, off), off).check()[0])
        for grad in outs:
            assert not grad[zero].any() and np.isfinite(grad).all() and (np.abs(grad[~zero]).sum(-1) > 0).all()


# ------------------------------------------------------------------------------------------------------ NaN containment
def test_nan_and_all_zero_pose_stay_in_their_pose_or_joint(M):
    c = case_of(257)
    for off in (0, 1):
        for what in ("nan", "zero"):
            y, x = c["pred"][:70].copy(), c["target"][:70].copy()
            if what == "nan":
                y[17, 0, 6, 1] = np.nan
            else:
                y[40] = 0.0
            pose = 17 if what == "nan" else 40
            # N-MPJPE: the pose's 48 values and the loss, nothing else
            grad, loss = run_n(M, place(y, off), place(x, off), off).check()
            want = np.zeros(grad.shape, dtype=bool)
            want[pose] = True
            assert np.array_equal(np.isnan(grad), want) and np.isnan(loss)
            # the other two: the joint's 3 values (an all-zero predicted pose is an ordinary input there)
            want[:] = False
            if what == "nan":
                want[17, 0, 6] = True
            for mode, key in WEIGHTS:
                grad, loss = run_w(M, place(y, off), place(x, off), place(c[key][:70], 0 if mode == 2 else off), mode, off).check()
                assert np.array_equal(np.isnan(grad), want) and np.isnan(loss) == (what == "nan")
            grad, _ = run_bj(M, place(y, off), place(x, off), place(np.ones(16, np.float32), off), off).check()
            assert np.array_equal(np.isnan(grad), want)


# ---------------------------------------------------------------------------------------------------------------- meter
def test_meter_is_exact_and_reproducible(M):
    """30 calls of varying size, N-MPJPE and every weight mode in turn, into one meter: exactly the sum of (double)loss * poses in
    call order; the same call sequence again gives the same bits in meter, losses and gradients"""
    ws = M.ops.posetrain_workspace()
    big = case_of(2048 * 64 + 1)
    calls = []
    for k in range(30):
        P = 17 + 31 * k
        lo = 97 * k
        sl = lambda key: big[key][lo:lo + P]
        kind = k % 4
        off = k % 2
        y, x = place(sl("pred") * np.float32(1 + k % 5), off), place(sl("target"), off)
        w = None if kind == 0 else place(big["w16"] if kind == 3 else sl(WEIGHTS[kind - 1][1]), 0 if kind == 2 else off)
        calls.append((kind, y, x, w, off, 3 * P + k))               # the meter's count is the caller's, not P
    records = []
    for _ in range(2):
        meter = M.ops.loss_meters(1)[0]
        outs = [run_n(M, y, x, off, poses, meter, ws) if kind == 0 else run_w(M, y, x, w, kind, off, poses, meter, ws)
                for kind, y, x, w, off, poses in calls]
        res = [o.check() for o in outs]
        records.append((meter.cpu().numpy().copy(), res))
    rec, res = records[0]
    want = 0.0
    for (_, loss), call in zip(res, calls):
        want += loss * call[5]
    got = float(rec[0:1].view(np.float64)[0])
    print("meter", got, want)
    assert got == want and rec[1] == sum(call[5] for call in calls) and rec[2] == 30
    assert np.array_equal(records[0][0], records[1][0])
    for (g0, l0), (g1, l1) in zip(res, records[1][1]):
        assert np.array_equal(g0, g1) and l0 == l1


# ------------------------------------------------------------------------------------------------------ scale invariance
@pytest.mark.parametrize("P", [65, 257])
def test_nmpjpe_gradient_is_orthogonal_to_the_prediction(M, P):
    """N-MPJPE does not change when a pose's prediction is rescaled, so its exact gradient g* has sum_k g*_k p_k = 0 per pose.  The
    kernel's g differs from g* by at most the gradient's bound b_k per element, hence |sum_k g_k p_k| <= sum_k b_k |p_k| (the
    sum itself is formed here in extended precision)"""
    c = case_of(P)
    _, g64, T = c["n"]
    grad, _ = run_n(M, place(c["pred"], 0), place(c["target"], 0), 0).check()
    p = c["pred"].astype(np.longdouble).reshape(P, 48)
    dot = np.abs((grad.astype(np.longdouble).reshape(P, 48) * p).sum(1)).astype(np.float64)
    lim = (CU.nmpjpe_bound(g64, T, P).reshape(P, 48) * np.abs(p).astype(np.float64)).sum(1)
    print("scale invariance P=%d: largest share of the summed bound %.3f" % (P, float((dot / lim).max())))
    assert (dot <= lim).all()
