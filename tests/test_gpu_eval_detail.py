"""The detailed pose errors on the GPU: dhaug_pose_column_errors and dhaug_pose_scaled_errors through the C-ABI, and
mpjpe_byjoint / weighted_mpjpe / n_mpjpe / mean_velocity_error / PoseDetailAccumulator of utils.loss built on them.

References: the fp64 restatements of tests/eval_detail_util.py computed here from the same fp32 inputs, and the fixture
tests/golden/pose_eval_detail.npz recorded from the reference's own functions.

Bounds (none measured on the code under test; the derivation is the module docstring of tests/eval_detail_util.py):
  against the restatement   a sum of n non-negative distances: (n + 8) 2^-52 |ref|; terms with cancellation (velocity,
                            s p - t, signed weights) add 8 * 2^-52 * A, A the sum of the absolute values entering the cancelling
                            differences (sum |w| e for signed weights); a result returned in fp32 adds 2^-24 |ref|.  The two
                            preconditions of the derivation are asserted on the inputs: sum S |p| <= 3.5 sum |t| for the scale,
                            |ref| >= 0.9 A for the signed weights chosen here.
  against the fixture       |got - ref64| <= max(4 N, the bound above), N = |ref32 - ref64| from the fixture: the distance of
                            the reference's own fp32 evaluation from its fp64 one.

Sizes.  The column kernel cuts the rows into at most MAX_BLOCKS / CC slabs of at least MIN_STEPS steps of RG rows (RG = max(1,
1024 / cols), CC = ceil(cols / 1024), MAX_BLOCKS = 1024, MIN_STEPS = 4): up to (MAX_BLOCKS / CC) * MIN_STEPS * RG rows every
slab has MIN_STEPS steps, one row more and the slabs grow past one "grid pass".  That row count is 262 145 for 16 columns,
86 017 for 48, 8 193 for 432 and 1 025 for 3 888 (rows_past() computes it from the binding's constants).  The scaled kernel
strides a grid of at most 2 048 workgroups of 64 poses: 131 073 poses is one past a grid pass."""
import os
import sys

import numpy as np
import pytest
import torch

import eval_detail_util as DU

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

CASES = ["noisy", "similarity", "millimetres", "kilometres"]


@pytest.fixture(scope="module")
def M():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    sys.path.insert(0, ROOT)
    import dhaug_amd
    dhaug_amd._lib.lib()
    from dhaug_amd import ops
    from dhaug_amd.utils import loss
    return dhaug_amd._lib, ops, loss


@pytest.fixture(scope="module")
def G():
    z = np.load(os.path.join(ROOT, "tests", "golden", "pose_eval_detail.npz"))
    return {k: z[k] for k in z.files}


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(a):
    return np.asarray(a, dtype=np.float64).view(np.int64)


def poses(rng, shape, noise=0.04):
    """(pred, target) fp32 of the given (..., 3) shape: joints around a root at depth 3-6 m, the prediction a noisy copy"""
    x = (rng.standard_normal(shape, dtype=np.float32) * np.float32(0.25))
    x[..., 2] += np.float32(4.5)
    y = x + rng.standard_normal(shape, dtype=np.float32) * np.float32(noise)
    return y, x


def rows_past(lib, cols):
    q = cols // 4
    rg, cc = max(1, 256 // q), (q + 255) // 256
    return (lib.COLERR_MAX_BLOCKS // cc) * lib.COLERR_MIN_STEPS * rg + 1


def column_call(lib, ops, y, x, center, want_col, want_vel, col0=0.0, vel0=0.0, ws=None):
    """one dhaug_pose_column_errors call on device tensors (rows, cols, 3) -> (col_sums, vel_sum) as numpy"""
    rows, cols = y.shape[0], y.shape[1]
    col = torch.full((cols,), col0, dtype=torch.float64, device="cuda")
    vel = torch.full((1,), vel0, dtype=torch.float64, device="cuda")
    if ws is None:
        ws = torch.empty(lib.COLERR_WORKSPACE_BYTES // 8, dtype=torch.float64, device="cuda")
    lib.call("dhaug_pose_column_errors", y.data_ptr(), x.data_ptr(), rows, cols, int(center), col.data_ptr() if want_col else None,
             vel.data_ptr() if want_vel else None, ws.data_ptr(), ops._stream())
    return col.cpu().numpy(), vel.cpu().numpy()


def scaled_call(lib, ops, y, x, center, w=None, per_joint=False, sums0=(0.0, 0.0)):
    """one dhaug_pose_scaled_errors call on device tensors (P, 16, 3) -> sums as numpy"""
    sums = torch.tensor(sums0, dtype=torch.float64, device="cuda")
    ws = torch.empty(lib.SCALEDERR_WORKSPACE_BYTES // 8, dtype=torch.float64, device="cuda")
    lib.call("dhaug_pose_scaled_errors", y.data_ptr(), x.data_ptr(), y.shape[0], int(center), None if w is None else w.data_ptr(),
             int(per_joint), sums.data_ptr(), ws.data_ptr(), ops._stream())
    return sums.cpu().numpy()


def centred(a, center):
    """what the kernels see: (rows, cols, 3) with every group of 16 columns root-centred in fp32"""
    if not center:
        return a
    return DU.center32(a.reshape(a.shape[0], -1, 16, 3)).reshape(a.shape)


@pytest.mark.parametrize("cols", [16, 48, 432, 3888])
def test_column_kernel_matches_fp64(M, cols):
    """rows 1, 2, 3, 63, 64, 65 and one row past a grid pass (module docstring), centring on and off; col_sums only, vel_sum
    only and both give the same bits, each within the bounds of the fp64 restatement; one row leaves vel_sum as it was"""
    lib, ops, _ = M
    assert cols <= lib.COLERR_MAX_COLS and (cols != 3888 or cols == lib.COLERR_MAX_COLS)
    past = rows_past(lib, cols)
    assert past == {16: 262145, 48: 86017, 432: 8193, 3888: 1025}[cols]
    rng = np.random.default_rng(cols)
    for rows in (1, 2, 3, 63, 64, 65, past):
        y, x = poses(rng, (rows, cols, 3))
        yd, xd = dev(y), dev(x)
        for center in (False, True):
            yc, xc = centred(y, center), centred(x, center)
            ref_c, b_c = DU.column_sums(yc, xc)
            both_c, both_v = column_call(lib, ops, yd, xd, center, True, True, vel0=-7.5)
            only_c, keep_v = column_call(lib, ops, yd, xd, center, True, False, vel0=-7.5)
            keep_c, only_v = column_call(lib, ops, yd, xd, center, False, True, col0=3.25, vel0=-7.5)
            assert np.array_equal(bits(both_c), bits(only_c)) and np.array_equal(bits(both_v), bits(only_v))
            assert np.all(keep_c == 3.25) and keep_v[0] == -7.5                   # an output not asked for is not touched
            err = np.abs(both_c - ref_c)
            moved = b_c > 0                                                       # (a centred root column is exactly 0)
            assert np.all(moved) or (center and np.array_equal(np.flatnonzero(~moved), np.arange(0, cols, 16)))
            fig = "cols %d rows %d center %d: col max err / bound %.3g" % (cols, rows, center, float(np.max(err[moved] / b_c[moved])))
            if rows == 1:
                assert both_v[0] == -7.5                                          # no row pair: vel_sum untouched
            else:
                ref_v, b_v = DU.velocity_sum(yc, xc)
                ev = abs(both_v[0] - (-7.5 + ref_v))
                b_v = b_v + 2.0 ** -52 * (7.5 + ref_v)                            # the preset's own add
                fig += ", vel err / bound %.3g" % (ev / b_v)
            print(fig)
            assert np.all(err <= b_c), fig
            assert rows == 1 or ev <= b_v, fig


def signed_weights(rng, shape):
    """fp32 weights, one in eight negative and small, so that |sum w e| >= 0.9 sum |w| e (asserted where they are used)"""
    w = rng.uniform(0.5, 2.0, size=shape)
    neg = rng.uniform(size=shape) < 0.125
    w[neg] = -rng.uniform(2.0 ** -10, 2.0 ** -9, size=shape)[neg]
    return w.astype(np.float32)


@pytest.mark.parametrize("P", [1, 2, 15, 16, 17, 255, 257, 131073])
def test_scaled_kernel_matches_fp64(M, P):
    """P around a wave's 16 poses, whole workgroups of 64 poses and one past a grid pass; centring on and off; no weights
    (sums[1] untouched), one per pose, one per joint, negative ones included"""
    lib, ops, _ = M
    assert P != 131073 or P == lib.SCALEDERR_MAX_BLOCKS * 64 + 1
    rng = np.random.default_rng(P)
    y, x = poses(rng, (P, 16, 3))
    y *= rng.uniform(0.8, 1.25, size=(P, 1, 1)).astype(np.float32)                 # a scale for N-MPJPE to find
    wp, wj = signed_weights(rng, (P, 1)), signed_weights(rng, (P, 16))
    if P == 1:
        wp[:] = -0.75                                                             # a single negative weight
    yd, xd, wpd, wjd = dev(y), dev(x), dev(wp), dev(wj)
    for center in (False, True):
        yc, xc = centred(y, center), centred(x, center)
        ref_n, b_n, Sy, ax = DU.scaled_sum(yc, xc)
        assert Sy <= 3.5 * ax
        none = scaled_call(lib, ops, yd, xd, center, sums0=(0.0, 11.5))
        assert none[1] == 11.5                                                    # w == NULL: sums[1] untouched
        fig = "P %d center %d: n-mpjpe err / bound %.3g" % (P, center, abs(none[0] - ref_n) / b_n)
        for w, wdv, per_joint in ((wp, wpd, False), (wj, wjd, True)):
            ref_w, b_w, A = DU.weighted_sum(yc, xc, w)
            assert abs(ref_w) >= 0.9 * A
            got = scaled_call(lib, ops, yd, xd, center, wdv, per_joint)
            assert bits(got[0]) == bits(none[0])
            fig += ", weighted (per %s) err / bound %.3g" % ("joint" if per_joint else "pose", abs(got[1] - ref_w) / b_w)
            assert abs(got[1] - ref_w) <= b_w, fig
        print(fig)
        assert abs(none[0] - ref_n) <= b_n, fig


def test_zero_prediction_gives_nan_scale(M):
    """an all-zero predicted pose: 0 / 0 in the scale, NaN as in the reference; the weighted sum does not use the scale"""
    lib, ops, _ = M
    rng = np.random.default_rng(3)
    y, x = poses(rng, (70, 16, 3))
    y[41] = 0.0
    w = dev(np.ones((70, 1), np.float32))
    got = scaled_call(lib, ops, dev(y), dev(x), False, w, False)
    assert np.isnan(got[0]) and np.isfinite(got[1])
    keep = np.arange(70) != 41
    got = scaled_call(lib, ops, dev(y[keep]), dev(x[keep]), False)
    ref, b, _, _ = DU.scaled_sum(y[keep], x[keep])
    assert np.isfinite(got[0]) and abs(got[0] - ref) <= b


def test_sums_accumulate_and_repeat_bit_for_bit(M):
    """totals are accumulated: a second call adds the same sum again (twice the first, exactly), a preset value is kept (one
    fp64 add); the same calls give the same bits"""
    lib, ops, _ = M
    rng = np.random.default_rng(4)
    y, x = poses(rng, (3000, 48, 3))
    yd, xd = dev(y), dev(x)
    ws = torch.empty(lib.COLERR_WORKSPACE_BYTES // 8, dtype=torch.float64, device="cuda")
    col = torch.zeros(48, dtype=torch.float64, device="cuda")
    vel = torch.zeros(1, dtype=torch.float64, device="cuda")
    call = lambda: lib.call("dhaug_pose_column_errors", yd.data_ptr(), xd.data_ptr(), 3000, 48, 1, col.data_ptr(), vel.data_ptr(),
                            ws.data_ptr(), ops._stream())
    call()
    c1, v1 = col.cpu().numpy(), vel.cpu().numpy()
    call()
    assert np.array_equal(bits(col.cpu().numpy()), bits(2.0 * c1)) and np.array_equal(bits(vel.cpu().numpy()), bits(2.0 * v1))
    again_c, again_v = column_call(lib, ops, yd, xd, True, True, True)
    assert np.array_equal(bits(again_c), bits(c1)) and np.array_equal(bits(again_v), bits(v1))
    pre_c, pre_v = column_call(lib, ops, yd, xd, True, True, True, col0=1234.5, vel0=-0.125)
    assert np.array_equal(bits(pre_c), bits(1234.5 + c1)) and np.array_equal(bits(pre_v), bits(-0.125 + v1))

    yp, xp = dev(y.reshape(-1, 16, 3)), dev(x.reshape(-1, 16, 3))
    w = dev(signed_weights(rng, (9000, 16)))
    s1 = scaled_call(lib, ops, yp, xp, True, w, True)
    assert np.array_equal(bits(scaled_call(lib, ops, yp, xp, True, w, True)), bits(s1))
    sums = torch.zeros(2, dtype=torch.float64, device="cuda")
    for _ in range(2):
        ops.pose_scaled_errors(yp, xp, center=True, w=w, sums=sums)
    assert np.array_equal(bits(sums.cpu().numpy()), bits(2.0 * s1))
    pre = scaled_call(lib, ops, yp, xp, True, w, True, sums0=(-3.5, 77.0))
    assert np.array_equal(bits(pre), bits(np.array([-3.5, 77.0]) + s1))


@pytest.mark.parametrize("rows,cols", [(65, 16), (131, 48), (9, 432), (5, 3888)])
def test_no_read_outside_the_inputs(M, rows, cols):
    """the inputs embedded in larger NaN-filled buffers: a read past either end would turn a sum into NaN; the sums are those of
    a stand-alone copy, bit for bit"""
    lib, ops, _ = M
    rng = np.random.default_rng(rows)
    y, x = poses(rng, (rows, cols, 3))
    n, pad = y.size, 4096

    def embedded(a):
        buf = torch.full((n + 2 * pad,), float("nan"), dtype=torch.float32, device="cuda")
        buf[pad:pad + n] = dev(a).reshape(-1)
        v = buf[pad:pad + n].view(rows, cols, 3)
        assert v.data_ptr() % 16 == 0
        return v

    ye, xe = embedded(y), embedded(x)
    for center in (False, True):
        c, v = column_call(lib, ops, ye, xe, center, True, True)
        assert np.all(np.isfinite(c)) and np.isfinite(v[0])
        c0, v0 = column_call(lib, ops, dev(y), dev(x), center, True, True)
        assert np.array_equal(bits(c), bits(c0)) and np.array_equal(bits(v), bits(v0))
        yc, xc = centred(y, center), centred(x, center)
        ref, b = DU.column_sums(yc, xc)
        assert np.all(np.abs(c - ref) <= b)
    P = rows * cols // 16
    w = signed_weights(rng, (P, 16))
    wbuf = torch.full((P * 16 + 2 * pad,), float("nan"), dtype=torch.float32, device="cuda")
    wbuf[pad:pad + P * 16] = dev(w).reshape(-1)
    for per_joint, wv in ((True, wbuf[pad:pad + P * 16]), (False, wbuf[pad:pad + P])):
        s = scaled_call(lib, ops, ye.view(P, 16, 3), xe.view(P, 16, 3), True, wv, per_joint)
        assert np.all(np.isfinite(s))
        s0 = scaled_call(lib, ops, dev(y).view(P, 16, 3), dev(x).view(P, 16, 3), True, wv.clone(), per_joint)
        assert np.array_equal(bits(s), bits(s0))


def test_misaligned_views_give_the_aligned_bits(M):
    """ops clones an input whose base is not 16-byte aligned (the C entries return DHAUG_EALIGN for it)"""
    lib, ops, _ = M
    rng = np.random.default_rng(5)
    y, x = poses(rng, (77, 32, 3))
    w = signed_weights(rng, (77 * 2, 16))

    def shifted(a):
        buf = torch.empty(a.size + 1, dtype=torch.float32, device="cuda")
        buf[1:] = dev(a).reshape(-1)
        v = buf[1:].view(a.shape)
        assert v.data_ptr() % 16 == 4
        return v

    ys, xs, ws = shifted(y), shifted(x), shifted(w)
    with pytest.raises(RuntimeError, match="DHAUG_EALIGN"):
        column_call(lib, ops, ys, xs, False, True, True)
    with pytest.raises(RuntimeError, match="DHAUG_EALIGN"):
        scaled_call(lib, ops, dev(y).view(-1, 16, 3), dev(x).view(-1, 16, 3), False, ws, True)
    new = lambda n: torch.zeros(n, dtype=torch.float64, device="cuda")
    a = ops.pose_column_errors(dev(y), dev(x), center=True, col_sums=new(32), vel_sum=new(1))
    b = ops.pose_column_errors(ys, xs, center=True, col_sums=new(32), vel_sum=new(1))
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and float(a[1]) > 0
    a = ops.pose_scaled_errors(dev(y).view(-1, 16, 3), dev(x).view(-1, 16, 3), w=dev(w))
    b = ops.pose_scaled_errors(ys.view(-1, 16, 3), xs.view(-1, 16, 3), w=ws)
    assert torch.equal(a, b) and float(a[0]) > 0


def loss_results(L, G, F, conv):
    """record name -> what utils.loss returns for inputs converted by conv"""
    t = conv
    (y3, x3), (y4, x4) = F["3"], F["4"]
    out = {"bj3": L.mpjpe_byjoint(t(y3), t(x3)), "bj4": L.mpjpe_byjoint(t(y4), t(x4)), "n4": L.n_mpjpe(t(y4), t(x4))}
    for k in DU.FIXTURE_WEIGHTS:
        y, x = F[k[-1]]
        out[k.replace("_", "")] = L.weighted_mpjpe(t(y), t(x), t(G[k]))
    return out


@pytest.mark.parametrize("case", CASES)
def test_loss_functions_match_fixture_and_formula(M, G, case):
    """host inputs: CPU tensors of the input dtype out (a numpy scalar for mean_velocity_error), shapes predicted.shape[1:-1] and
    0-d; within max(4 N, bound) of the fixture's ref64 and within the bound of the fp64 formula, fp32 results with their
    2^-24 |ref| rounding"""
    L = M[2]
    F, R = DU.fixture_forms(G, case), DU.fixture_restated(G, case)
    got = loss_results(L, G, F, torch.from_numpy)
    (y3, x3), (y4, x4) = F["3"], F["4"]
    got["v3"], got["v4"] = L.mean_velocity_error(y3, x3), L.mean_velocity_error(torch.from_numpy(y4), torch.from_numpy(x4))
    assert isinstance(got["v3"], np.float32) and isinstance(got["v4"], np.float32)
    assert isinstance(L.mean_velocity_error(y3.astype(np.float64), x3), np.float64)
    for k, v in got.items():
        ref, bound = R[k]
        if not k.startswith("v"):
            assert torch.is_tensor(v) and not v.is_cuda and v.dtype == torch.float32 and tuple(v.shape) == np.shape(ref), k
            v = v.numpy()
        r32, r64 = G["%s_%s_ref32" % (case, k)], G["%s_%s_ref64" % (case, k)]
        v = np.asarray(v, dtype=np.float64)
        bound = bound + DU.E24 * np.abs(ref)
        e_fix, e_for = np.abs(v - r64), np.abs(v - ref)
        lim = np.maximum(4 * np.abs(r32.astype(np.float64) - r64), bound)
        print("%s %s: |got - ref64| / max(4N, bound) %.3g, |got - formula| / bound %.3g, N / bound %.3g"
              % (case, k, float(np.max(e_fix / lim)), float(np.max(e_for / bound)),
                 float(np.max(np.abs(r32.astype(np.float64) - r64) / bound))))
        assert np.all(e_fix <= lim), (case, k)
        assert np.all(e_for <= bound), (case, k)


def test_loss_functions_on_device_tensors(M, G):
    """device tensors in: device tensors out (0-d, or predicted.shape[1:-1]), the host results' values; fp64 device inputs keep
    their dtype; a prediction that requires grad takes the plain-torch expression and carries a grad_fn"""
    L = M[2]
    F, R = DU.fixture_forms(G, "noisy"), DU.fixture_restated(G, "noisy")
    host = loss_results(L, G, F, torch.from_numpy)
    devr = loss_results(L, G, F, dev)
    for k, v in devr.items():
        assert v.is_cuda and v.dtype == torch.float32 and v.shape == host[k].shape, k
        assert torch.equal(v.cpu(), host[k]), k
    (y3, x3), (y4, x4) = F["3"], F["4"]
    v = L.mean_velocity_error(dev(y4), dev(x4))
    assert v.is_cuda and v.dim() == 0 and v.dtype == torch.float32 and float(v) == float(L.mean_velocity_error(y4, x4))
    v = L.mean_velocity_error(dev(y3[:1]), dev(x3[:1]))
    assert v.is_cuda and v.dim() == 0 and bool(torch.isnan(v))
    d64 = L.n_mpjpe(dev(y4).double(), dev(x4).double())
    assert d64.dtype == torch.float64 and abs(float(d64) - R["n4"][0]) <= R["n4"][1]
    b64 = L.mpjpe_byjoint(torch.from_numpy(y4).double(), torch.from_numpy(x4).double())
    assert b64.dtype == torch.float64 and not b64.is_cuda and np.all(np.abs(b64.numpy() - R["bj4"][0]) <= R["bj4"][1])
    one = L.mpjpe_byjoint(dev(y3[0]), dev(x3[0]))                                # one pose: the first axis is the joints
    assert one.is_cuda and one.dim() == 0 and float(one) == pytest.approx(float(DU.distances(y3[0], x3[0]).mean()), rel=1e-6)
    # training code: the reference's expression in plain torch, differentiable
    p = dev(y4).requires_grad_(True)
    for k, v in (("bj4", L.mpjpe_byjoint(p, dev(x4))), ("wp4", L.weighted_mpjpe(p, dev(x4), dev(G["w_p4"]))),
                 ("n4", L.n_mpjpe(p, dev(x4)))):
        assert v.grad_fn is not None and v.is_cuda, k
        np.testing.assert_allclose(v.detach().cpu().numpy(), R[k][0], rtol=2e-5, atol=1e-7)
        (g,) = torch.autograd.grad(v.sum(), p)
        assert g.shape == p.shape and bool(torch.isfinite(g).all()) and float(g.abs().sum()) > 0
    with torch.no_grad():
        assert L.n_mpjpe(p, dev(x4)).grad_fn is None
        assert torch.equal(L.n_mpjpe(p, dev(x4)).cpu(), host["n4"])


def test_accumulator_equals_one_call_on_the_concatenation(M, G):
    """PoseDetailAccumulator over several batches (4-D and 3-D, a host one among them) and three sequences: the per-joint and
    N-MPJPE sums of all poses at once, the velocity sum of one call per sequence -- within the bounds of the fp64 formulas on the
    concatenation; one host read in result(), none in add()"""
    L = M[2]
    rng = np.random.default_rng(6)
    seqs = [poses(rng, (n, 16, 3)) for n in (40, 1, 25)] + [poses(rng, (12, 3, 16, 3))]
    batches = [poses(rng, (64, 16, 3)), poses(rng, (7, 5, 16, 3)), poses(rng, (130, 16, 3))]
    for center in (True, False):
        acc = L.PoseDetailAccumulator(center=center)
        assert acc.result() == dict(poses=0, mpjpe_byjoint=[0.0] * 16, n_mpjpe=0.0, velocity=0.0, velocity_pairs=0)
        reads = []
        orig = torch.Tensor.cpu
        torch.Tensor.cpu = lambda self, *a, **k: (reads.append(1) if self.is_cuda else None, orig(self, *a, **k))[1]
        try:
            for i, (y, x) in enumerate(batches):
                acc.add(dev(y), dev(x)) if i != 1 else acc.add(torch.from_numpy(y), torch.from_numpy(x))
            for y, x in seqs:
                acc.add(dev(y), dev(x), sequence=True)
            assert reads == []
            r = acc.result()
            assert len(reads) == 1
        finally:
            torch.Tensor.cpu = orig
        c = lambda a: DU.center32(a) if center else a
        ally = np.concatenate([c(y).reshape(-1, 16, 3) for y, _ in batches + seqs])
        allx = np.concatenate([c(x).reshape(-1, 16, 3) for _, x in batches + seqs])
        n = len(ally)
        assert r["poses"] == n == 64 + 35 + 130 + 66 + 36
        ref, b = DU.column_sums(ally, allx)
        slack = 8 * DU.E52 * ref                                                  # the batches' sums are added one by one
        assert np.all(np.abs(np.array(r["mpjpe_byjoint"]) * n - ref) <= b + slack)
        ref, b, Sy, ax = DU.scaled_sum(ally, allx)
        assert Sy <= 3.5 * ax and abs(r["n_mpjpe"] * 16 * n - ref) <= b + 8 * DU.E52 * ref
        pairs, ref, b = 0, 0.0, 0.0
        for y, x in seqs:
            if len(y) > 1:
                rv, bv = DU.velocity_sum(c(y), c(x))
                pairs, ref, b = pairs + (len(y) - 1) * (y[0].size // 3), ref + rv, b + bv
        assert r["velocity_pairs"] == pairs == 39 * 16 + 24 * 16 + 11 * 48
        assert abs(r["velocity"] * pairs - ref) <= b + 8 * DU.E52 * ref
        # the accumulated velocity is that of mean_velocity_error per sequence
        if not center:
            per = sum(float(L.mean_velocity_error(y.astype(np.float64), x.astype(np.float64))) * (len(y) - 1) * (y[0].size // 3)
                      for y, x in seqs if len(y) > 1)
            assert abs(r["velocity"] * pairs - per) <= 2 * (b + 8 * DU.E52 * ref)
        assert acc.zero().result()["poses"] == 0
