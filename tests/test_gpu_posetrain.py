"""The posenet training loop on the GPU: dhaug_pair_batch, dhaug_pose_mse, dhaug_grad_sumsq + dhaug_adam_clip_step through the
C-ABI against torch / fp64 restatements, PosenetAdam, and the three drop-in loops end to end against
tests/golden/posetrain.npz (recorded from the reference's own loops on the CPU) and against a stock-torch run of the same
loops on the same device."""
import ctypes
import itertools
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn

import posetrain_util as PU

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

# The floor of the end-to-end comparison, measured on an MI355X (MEASURED_ON): the stock-torch restatement of the reference's
# loops (posetrain_util.stock_loop: criterion, clip_grad_norm_, torch.optim.Adam; no code of this package) on the GPU against the
# CPU-recorded fixture.  N_PARAM: largest absolute difference of any parameter / BatchNorm buffer after the 12 steps; N_LOSS,
# N_NORM: largest relative difference of a step's loss / gradient norm.  The drop-ins must agree with the fixture to 4 x these
# and with the stock-torch run on the same device to max(N, SAME_DEVICE_FLOOR).
MEASURED_ON = "2026-10-16, MI355X (gfx950), ROCm PyTorch; two runs, the same figures (rounded up to three digits)"
N_PARAM = dict(single=1.20e-07, video=4.48e-08, gan=4.48e-08)         # measured 1.1921e-07, 4.4703e-08
N_LOSS = dict(single=1.23e-07, video=1.99e-07, gan=1.99e-07)          # measured 1.2246e-07, 1.9875e-07
N_NORM = dict(single=1.28e-07, video=1.66e-07, gan=1.66e-07)          # measured 1.2721e-07, 1.6519e-07
SAME_DEVICE_FLOOR = 2e-5            # the bound of test_posetrain_cpu.test_fixture_is_self_consistent: fused against torch arithmetic
CHAOS_LIMIT = 1e-3                  # a tenth of how far the fixture's parameters move


@pytest.fixture(scope="module")
def M():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    sys.path.insert(0, ROOT)
    import dhaug_amd
    L = dhaug_amd._lib.lib()
    from dhaug_amd import ops, optim
    from dhaug_amd.function_aug import model_pos_train
    from dhaug_amd.models_Fk_GAN import video_mode_operate
    fns = dict(single=model_pos_train.train_posenet, video=video_mode_operate.video_mode_train_posenet,
               gan=video_mode_operate.GAN_dataSet_video_mode_train_posenet)
    import argparse
    return argparse.Namespace(L=L, ops=ops, optim=optim, T=model_pos_train, V=video_mode_operate, fns=fns, lib=dhaug_amd._lib)


@pytest.fixture(scope="module")
def G():
    return PU.load_golden()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def ulp32(ref64):
    """the spacing of fp32 at |ref|"""
    return np.spacing(np.abs(np.asarray(ref64, dtype=np.float64)).astype(np.float32)).astype(np.float64)


# ---------------------------------------------------------------------------------------------------------- 4. pair batch
@pytest.mark.parametrize("F", [1, 9, (1, 9)])
@pytest.mark.parametrize("n", [1, 2, 96, 1024])
def test_pair_batch_equals_the_torch_expressions(M, F, n):
    F3, F2 = F if isinstance(F, tuple) else (F, F)
    g = torch.Generator().manual_seed(100 * n + F3 + F2)
    rows = n + 37
    p3 = (torch.randn(rows, F3, 16, 3, generator=g) * 2).cuda()
    p2 = torch.randn(rows, F2, 16, 2, generator=g).cuda()
    p3[0, 0, 3, 1] = 0.0                                         # a zero keeps its sign through the flip
    perm = torch.randperm(rows, generator=g)[:n].cuda()
    for idx, flip, playback in itertools.product((None, perm), (0, 1), (0, 1)):
        s3, s2 = (p3[:n], p2[:n]) if idx is None else (p3[idx], p2[idx])
        want = dict(tgt=s3 - s3[:, :, :1, :], inp=s2)
        if flip:
            want.update(tgt_flip=PU.flip(want["tgt"]), inp_flip=PU.flip(s2))
        if playback:
            want.update(inp_back=torch.flip(s2, dims=[1]))
            if flip:
                want.update(inp_flip_back=torch.flip(want["inp_flip"], dims=[1]))
        got = {k: torch.full_like(v, float("nan")) for k, v in want.items()}
        o = lambda k: ptr(got.get(k))
        rc = M.L.dhaug_pair_batch(ptr(p3), ptr(p2), rows, F3, F2, ptr(idx), n, flip, playback, o("tgt"), o("inp"), o("tgt_flip"),
                                  o("inp_flip"), o("inp_back"), o("inp_flip_back"), stream())
        assert rc == 0
        for k in want:
            assert torch.equal(got[k], want[k]), (k, idx is not None, flip, playback)
    # the wrapper: shapes with and without a frame axis, every output of the flags
    out = M.ops.pair_batch(p3[:, 0], p2[:, 0], idx=perm, flip=True, playback=True)
    assert sorted(out) == ["inp", "inp_back", "inp_flip", "inp_flip_back", "tgt", "tgt_flip"]
    assert out["tgt"].shape == (n, 1, 16, 3) and out["inp"].shape == (n, 1, 16, 2)
    s3 = p3[perm][:, 0]
    assert torch.equal(out["tgt"][:, 0], s3 - s3[:, :1]) and torch.equal(out["inp_flip"][:, 0], PU.flip(p2[perm][:, 0]))


# ---------------------------------------------------------------------------------------------------------------- 5. MSE
def _mse(M, pred, tgt, poses, meter, ws):
    grad = torch.full_like(pred, float("nan"))
    loss = torch.full((1,), float("nan"), device="cuda")
    rc = M.L.dhaug_pose_mse(ptr(pred), ptr(tgt), pred.numel(), poses, ptr(grad), ptr(loss), ptr(meter), ptr(ws), stream())
    assert rc == 0
    return grad, loss


@pytest.mark.parametrize("shape", [(96, 16, 3), (1024, 16, 3), (40, 1, 16, 3), (7, 5), (3,)])
def test_pose_mse_gradient_and_loss(M, shape):
    g = torch.Generator().manual_seed(sum(shape))
    ws = M.ops.posetrain_workspace()
    for off in (0, 1):                                           # 16-byte aligned and not
        numel = int(np.prod(shape))
        pred = (torch.randn(numel + 1, generator=g) * 3).cuda()[off:off + numel]
        tgt = (torch.randn(numel + 1, generator=g) * 3).cuda()[off:off + numel]
        grad, loss = _mse(M, pred, tgt, shape[0], None, ws)
        p64, t64 = pred.cpu().double().numpy(), tgt.cpu().double().numpy()
        g64 = 2.0 * (p64 - t64) / numel
        err = np.abs(grad.cpu().double().numpy() - g64) / ulp32(g64)
        l64 = float(np.mean((p64 - t64) ** 2))
        lerr = abs(float(loss.cpu().double()[0]) - l64) / float(ulp32(l64))
        print("pose_mse", shape, off, "grad err %.3f ulp, loss err %.3f ulp" % (err.max(), lerr))
        assert err.max() <= 2.0 and lerr <= 1.0
    # against torch's own forward / backward
    x = (torch.randn(shape, generator=g)).cuda().requires_grad_(True)
    t = torch.randn(shape, generator=g).cuda()
    ref = nn.MSELoss(reduction="mean")(x, t)
    ref.backward()
    loss, grad = M.ops.pose_mse(x, t, shape[0])
    assert torch.allclose(grad, x.grad, rtol=1e-6, atol=0) and torch.allclose(loss[0], ref, rtol=1e-6)


def test_pose_mse_meter_is_exact_and_reproducible(M):
    ws = M.ops.posetrain_workspace()
    g = torch.Generator().manual_seed(9)
    calls = []
    for k in range(30):
        n = 17 + 31 * k
        calls.append(((torch.randn(n, 16, 3, generator=g) * (1 + k % 5)).cuda(), torch.randn(n, 16, 3, generator=g).cuda(), n))
    records = []
    for _ in range(2):
        meter = M.ops.loss_meters(1)[0]
        losses = [_mse(M, p, t, n, meter, ws)[1] for p, t, n in calls]
        records.append(meter.cpu().numpy().copy())
    rec = records[0]
    want = float(np.sum([float(l.cpu().double()[0]) * n for l, (_, _, n) in zip(losses, calls)], dtype=np.float64))
    got = float(rec[0:1].view(np.float64)[0])
    print("meter", got, want, abs(got / want - 1))
    assert abs(got / want - 1) <= 1e-12
    assert rec[1] == sum(n for _, _, n in calls) and rec[2] == 30
    assert np.array_equal(records[0], records[1])


# ------------------------------------------------------------------------------------------------------- 6. gradient norm
def _norm(M, g, scale, ws, counter=None):
    """the norm dhaug_adam_clip_step stores, from a step with lr = 0 on scratch vectors"""
    n = g.numel()
    p, m, v = (torch.zeros(n + 1, device="cuda")[1:] for _ in range(3))          # deliberately not 16-byte aligned
    step = torch.ones(1, dtype=torch.int32, device="cuda")
    norm = torch.full((1,), float("nan"), device="cuda")
    assert M.L.dhaug_grad_sumsq(ptr(g), n, scale, ptr(ws), ptr(counter), stream()) == 0
    assert M.L.dhaug_adam_clip_step(ptr(p), ptr(g), ptr(m), ptr(v), n, 0.0, 0.9, 0.999, 1e-8, ptr(step), scale, 1.0, ptr(ws),
                                    ptr(norm), stream()) == 0
    return norm


@pytest.mark.parametrize("n", [1, 255, 4097, 8400000])
def test_grad_norm_against_fp64(M, n):
    ws = M.ops.posetrain_workspace()
    g = torch.Generator().manual_seed(n)
    base = (torch.randn(n + 3, generator=g) * 0.37).cuda()
    for off in (0, 1, 2, 3):
        for scale in (1.0, 0.5, 1.0 / 3.0):
            v = base[off:off + n]
            got = _norm(M, v, scale, ws)
            bits = ws.clone()
            again = _norm(M, v, scale, ws)
            scaled = (v * torch.tensor(scale, dtype=torch.float32)).double()     # the fp32 product, as the kernels form it
            want = float(torch.sqrt((scaled * scaled).sum()).cpu())
            rel = abs(float(got.cpu().double()[0]) / want - 1)
            if off == 0 or scale == 1.0:
                print("grad norm n=%d off=%d scale=%.3f rel err %.3e" % (n, off, scale, rel))
            assert rel <= 2.0 ** -23
            assert torch.equal(got, again) and torch.equal(bits, ws)
    counter = torch.full((1,), 41, dtype=torch.int32, device="cuda")
    _norm(M, base[:n], 1.0, ws, counter)
    assert int(counter.cpu()[0]) == 42


# ------------------------------------------------------------------------------------------------------ 7. clip + Adam
def _state(n, seed, moments=True):
    g = torch.Generator().manual_seed(seed)
    p = torch.randn(n, generator=g).cuda()
    grad = torch.randn(n, generator=g).cuda()
    m = (torch.randn(n, generator=g) * 0.01).cuda() if moments else torch.zeros(n, device="cuda")
    v = (torch.rand(n, generator=g) * 1e-4).cuda() if moments else torch.zeros(n, device="cuda")
    return p, grad, m, v


def _clip_step(M, p, g, m, v, step, lr, scale, max_norm, ws):
    norm = torch.full((1,), float("nan"), device="cuda")
    n = p.numel()
    assert M.L.dhaug_grad_sumsq(ptr(g), n, scale, ptr(ws), ptr(step), stream()) == 0
    assert M.L.dhaug_adam_clip_step(ptr(p), ptr(g), ptr(m), ptr(v), n, lr, 0.9, 0.999, 1e-8, ptr(step), scale, max_norm, ptr(ws),
                                    ptr(norm), stream()) == 0
    return norm


@pytest.mark.parametrize("scale", [1.0, 0.5, 1.0 / 3.0])
@pytest.mark.parametrize("n", [10007, 4096, 3])
def test_unclipped_step_is_adam_step_dev_bit_for_bit(M, n, scale):
    """(i) norm 0.5 < max_norm 1: coef == 1, and the parameters and both moments are dhaug_adam_step_dev's bits, step after step"""
    ws = M.ops.posetrain_workspace()
    p, g, m, v = _state(n, n)
    g = g * (0.5 / (g * scale).norm())
    a = [t.clone() for t in (p, m, v)]
    b = [t.clone() for t in (p, m, v)]
    sa, sb = (torch.zeros(1, dtype=torch.int32, device="cuda") for _ in range(2))
    for k in range(3):
        gk = g * (1.0 + 0.25 * k)                                   # norms 0.5, 0.625, 0.75
        norm = _clip_step(M, a[0], gk, a[1], a[2], sa, 1e-3, scale, 1.0, ws)
        assert float(norm.cpu()[0]) < 0.99
        M.ops.adam_step_dev(b[0], gk, b[1], b[2], sb, 1e-3, (0.9, 0.999), 1e-8, scale)
        for x, y, name in zip(a, b, ("param", "exp_avg", "exp_avg_sq")):
            assert torch.equal(x, y), (name, k)
    assert int(sa.cpu()[0]) == 3 == int(sb.cpu()[0])
    # max_norm = +inf: no clipping whatever the norm
    big = g * 100.0
    _clip_step(M, a[0], big, a[1], a[2], sa, 1e-3, scale, float("inf"), ws)
    M.ops.adam_step_dev(b[0], big, b[1], b[2], sb, 1e-3, (0.9, 0.999), 1e-8, scale)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


@pytest.mark.parametrize("case", [dict(norm=7.3, max_norm=1.0, scale=0.5), dict(norm=3e-5, max_norm=1e-5, scale=1.0)])
def test_clipped_step_against_fp64(M, case):
    """(ii) fp64 restatement from the fp32 inputs, first step (zero moments, so exp_avg is linear and exp_avg_sq quadratic in coef
    with nothing to cancel against): norm to 2^-23, both moments to 4 ulp, |p - p64| <= ulp(p) + 1e-5 lr"""
    n, lr = 10007, 1e-3
    f32, f64 = np.float32, np.float64
    ws = M.ops.posetrain_workspace()
    p, g, m, v = _state(n, 77, moments=False)
    scale, max_norm = case["scale"], case["max_norm"]
    g = g * (case["norm"] / (g * scale).norm())
    p0 = p.clone()
    step = torch.zeros(1, dtype=torch.int32, device="cuda")
    norm = _clip_step(M, p, g, m, v, step, lr, scale, max_norm, ws)
    gs = (g.cpu().numpy() * f32(scale)).astype(f64)
    norm64 = np.sqrt(np.sum(gs * gs))
    got_norm = float(norm.cpu().double()[0])
    # coef as the interface defines it: the norm rounded to fp32, then min(1, max_norm / (norm + 1e-6)) in fp32
    coef = f64(min(f32(1.0), f32(max_norm) / (f32(norm64) + f32(1e-6))))
    assert coef < 0.5 and abs(coef / (max_norm / norm64) - 1) > (0.02 if case["norm"] < 1e-3 else 0)   # the 1e-6 matters
    b1, b2, eps = f64(f32(0.9)), f64(f32(0.999)), f64(f32(1e-8))
    gi = gs * coef
    m64 = gi * (1.0 - b1)
    v64 = gi * gi * (1.0 - b2)
    p64 = p0.cpu().double().numpy() - (lr / (1.0 - b1)) * (m64 / (np.sqrt(v64) / np.sqrt(1.0 - b2) + eps))
    em = (np.abs(m.cpu().double().numpy() - m64) / ulp32(m64)).max()
    ev = (np.abs(v.cpu().double().numpy() - v64) / ulp32(v64)).max()
    dp = np.abs(p.cpu().double().numpy() - p64)
    print("clip step", case, "norm rel %.3e exp_avg %.2f ulp exp_avg_sq %.2f ulp param excess %.3e of lr"
          % (abs(got_norm / norm64 - 1), em, ev, (np.maximum(dp - ulp32(p64), 0) / lr).max()))
    assert abs(got_norm / norm64 - 1) <= 2.0 ** -23
    assert em <= 4.0 and ev <= 4.0
    assert (dp <= ulp32(p64) + 1e-5 * lr).all()
    assert int(step.cpu()[0]) == 1


@pytest.mark.parametrize("bad", [float("nan"), float("inf")])
def test_nonfinite_gradients_behave_as_torch(M, bad):
    """(iii) error_if_nonfinite=False: a NaN gradient makes every parameter NaN; an inf gradient makes coef 0, that element's
    update NaN and leaves the others where they are"""
    n = 1000
    ws = M.ops.posetrain_workspace()
    p, g, m, v = _state(n, 5, moments=False)
    g[123] = bad
    ref = nn.Parameter(p.clone())
    ref.grad = g.clone()
    opt = torch.optim.Adam([ref], lr=1e-3)
    nn.utils.clip_grad_norm_([ref], max_norm=1)
    opt.step()
    step = torch.zeros(1, dtype=torch.int32, device="cuda")
    norm = _clip_step(M, p, g, m, v, step, 1e-3, 1.0, 1.0, ws)
    got_nan, ref_nan = torch.isnan(p), torch.isnan(ref.detach())
    assert torch.equal(got_nan, ref_nan)
    assert int(got_nan.sum().cpu()) == (n if bad != bad else 1)
    assert torch.equal(p[~got_nan], ref.detach()[~ref_nan])
    assert (torch.isnan(norm) if bad != bad else torch.isinf(norm)).all()


def test_posenet_adam_follows_a_lambda_lr(M):
    """(iv) five clip_steps with torch's LambdaLR attached against clip_grad_norm_ + torch.optim.Adam under the same schedule;
    step() without clipping keeps working; state_dict round trip"""
    torch.manual_seed(4)
    net_a, net_b = PU.StubPosenet().cuda(), PU.StubPosenet().cuda()
    net_b.load_state_dict(net_a.state_dict())
    oa = M.optim.PosenetAdam(net_a.parameters(), lr=1e-3)
    ob = torch.optim.Adam(net_b.parameters(), lr=1e-3)
    decay = lambda e: 0.5 ** e
    sa, sb = torch.optim.lr_scheduler.LambdaLR(oa, decay), torch.optim.lr_scheduler.LambdaLR(ob, decay)
    x, t = torch.randn(64, 16, 2).cuda(), torch.randn(64, 16, 3).cuda() * 3
    for k in range(5):
        for net, opt in ((net_a, oa), (net_b, ob)):
            opt.zero_grad()
            nn.MSELoss()(net(x), t).backward()
        na = oa.clip_step(1.0)
        nb = nn.utils.clip_grad_norm_(net_b.parameters(), max_norm=1)
        ob.step()
        sa.step(), sb.step()
        assert oa.param_groups[0]["lr"] == pytest.approx(1e-3 * 0.5 ** (k + 1))
        assert torch.allclose(na[0], nb, rtol=1e-5)
        # (the bound of the same comparison in the end-to-end test; a step at the unscheduled lr would be off by ~ lr / 2)
        for pa, pb in zip(net_a.parameters(), net_b.parameters()):
            assert (pa - pb).abs().max().item() <= SAME_DEVICE_FLOOR, k
    before = [p.detach().clone() for p in net_a.parameters()]
    for net, opt in ((net_a, oa), (net_b, ob)):
        opt.zero_grad()
        nn.MSELoss()(net(x), t * 0.01).backward()
        opt.step()                                                  # no clipping
    for pa, pb, p0 in zip(net_a.parameters(), net_b.parameters(), before):
        assert (pa - pb).abs().max().item() <= SAME_DEVICE_FLOOR and (pa - p0).abs().max().item() > 0
    sd = oa.state_dict()
    assert sd["dhaug_flat"]["step_count"] == 6
    oa.load_state_dict(sd)
    assert int(oa.step_dev.cpu()[0]) == 6


# ------------------------------------------------------------------------------------------------------ 8 / 9. end to end
def _run_drop_in(M, G, loop, optimizer="fused", criterion=None, numpy_batches=False):
    """one of the three loops on the fixture's model and batches: (model, per-step losses, norms, meters)"""
    model = PU.load_initial(PU.make_model(loop), G, loop).cuda()
    opt = M.T.posenet_optimizer(model, PU.LR) if optimizer == "fused" else torch.optim.Adam(model.parameters(), lr=PU.LR)
    if numpy_batches:                                             # what the reference's ChunkedGenerator yields
        batches = [(b3.double().numpy(), b2.double().numpy()) for b3, b2 in PU.batches_of(G, loop)]
    else:
        batches = PU.batches_of(G, loop, dev if loop == "video" else (lambda a: torch.from_numpy(np.ascontiguousarray(a))))
    fn = M.fns[loop]
    fn(model, PU.loader_of(loop, batches), opt, criterion if criterion is not None else nn.MSELoss(reduction="mean"),
       torch.device("cuda"), PU.loop_args())
    trace = fn.last_trace.cpu().double().numpy()
    return model, trace[:, 0], trace[:, 1], fn.last_meters


def _run_stock(G, loop):
    model = PU.load_initial(PU.make_model(loop), G, loop).cuda()
    losses, norms = PU.stock_loop(model, loop, PU.batches_of(G, loop, dev), torch.optim.Adam(model.parameters(), lr=PU.LR),
                                  nn.MSELoss(reduction="mean"))
    return model, losses.cpu().double().numpy(), norms.cpu().double().numpy()


def _state_diff(a, b):
    sa, sb = PU.state_arrays(a), PU.state_arrays(b)
    return max(float(np.abs(sa[k] - sb[k]).max()) for k in sa)


def _rel(a, b):
    return float(np.abs(np.asarray(a) / np.asarray(b) - 1).max())


@pytest.mark.parametrize("loop", PU.LOOPS)
def test_stock_torch_floor_on_this_device(G, loop):
    """the floor itself: stock torch on this GPU against the CPU-recorded fixture stays at the recorded constants' scale and far
    below the chaos limit (otherwise the fixture would pin nothing)"""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    model, losses, norms = _run_stock(G, loop)
    n_param, n_loss, n_norm = PU.max_state_diff(model, G, loop), _rel(losses, G[loop + "_losses"]), _rel(norms, G[loop + "_norms"])
    print("FLOOR %s N_param %.3e N_loss %.3e N_norm %.3e" % (loop, n_param, n_loss, n_norm))
    assert n_param <= CHAOS_LIMIT
    assert n_param <= 4 * N_PARAM[loop] and n_loss <= 4 * N_LOSS[loop] and n_norm <= 4 * N_NORM[loop]


@pytest.mark.parametrize("loop", PU.LOOPS)
def test_drop_in_loops_end_to_end(M, G, loop):
    """train_posenet / video_mode_train_posenet / GAN_dataSet_video_mode_train_posenet with PosenetAdam, flip and playback on:
    final parameters, BatchNorm buffers, per-step losses and norms against the fixture to 4 N, and against the stock-torch run on
    this device to max(N, 2e-5)"""
    model, losses, norms, meters = _run_drop_in(M, G, loop)
    stock, s_losses, s_norms = _run_stock(G, loop)
    assert len(losses) == 12 == meters["steps"]
    d_fix = (PU.max_state_diff(model, G, loop), _rel(losses, G[loop + "_losses"]), _rel(norms, G[loop + "_norms"]))
    d_dev = (_state_diff(model, stock), _rel(losses, s_losses), _rel(norms, s_norms))
    print("E2E %s vs fixture: param %.3e loss %.3e norm %.3e | vs stock torch here: param %.3e loss %.3e norm %.3e"
          % ((loop,) + d_fix + d_dev))
    assert d_fix[0] <= 4 * N_PARAM[loop] and d_fix[1] <= 4 * N_LOSS[loop] and d_fix[2] <= 4 * N_NORM[loop]
    assert d_dev[0] <= max(N_PARAM[loop], SAME_DEVICE_FLOOR)
    assert d_dev[1] <= max(N_LOSS[loop], SAME_DEVICE_FLOOR) and d_dev[2] <= max(N_NORM[loop], SAME_DEVICE_FLOOR)
    # the meters: pose-weighted means of the recorded losses; the flip meter holds the PLAIN losses (the reference's quirk)
    sizes = [len(b3) for b3, _ in PU.batches_of(G, loop)]
    per = 2 if loop == "single" else 4
    ref = G[loop + "_losses"].reshape(-1, per)
    mean = lambda col: float(np.sum(ref[:, col] * sizes) / np.sum(sizes))
    assert meters["loss"] == pytest.approx(mean(0), rel=1e-4) and meters["flip_loss"] == meters["loss"]
    assert meters["loss_poses"] == sum(sizes) == meters["flip_loss_poses"]
    if loop != "single":
        assert meters["back_loss"] == pytest.approx(mean(1), rel=1e-4)
        assert meters["back_flip_loss"] == pytest.approx(mean(3), rel=1e-4)
    if loop == "video":                                           # host numpy batches (the reference's generators): the same bits
        again, l2, n2, _ = _run_drop_in(M, G, loop, numpy_batches=True)
        assert _state_diff(model, again) == 0 and np.array_equal(losses, l2) and np.array_equal(norms, n2)


@pytest.mark.parametrize("loop", PU.LOOPS)
def test_fallbacks(M, G, loop):
    """a stock torch.optim.Adam and a criterion that is not nn.MSELoss take the reference's calls piece by piece"""
    stock, s_losses, s_norms = _run_stock(G, loop)
    model, losses, norms, meters = _run_drop_in(M, G, loop, optimizer="stock")            # fused loss, torch's clip + Adam
    d = (_state_diff(model, stock), _rel(losses, s_losses), _rel(norms, s_norms))
    print("FALLBACK %s MSELoss + stock Adam vs stock torch: param %.3e loss %.3e norm %.3e" % ((loop,) + d))
    assert d[0] <= N_PARAM[loop] and d[1] <= N_LOSS[loop] and d[2] <= N_NORM[loop]
    for optimizer in ("stock", "fused"):
        model, losses, norms, meters = _run_drop_in(M, G, loop, optimizer=optimizer, criterion=nn.L1Loss())
        assert len(losses) == 12 and np.isfinite(losses).all() and np.isfinite(norms).all() and (norms > 0).all()
        assert all(np.isfinite(a).all() for a in PU.state_arrays(model).values())
        sizes = [len(b3) for b3, _ in PU.batches_of(G, loop)]
        per = 2 if loop == "single" else 4
        assert meters["loss"] == pytest.approx(float(np.sum(losses.reshape(-1, per)[:, 0] * sizes) / np.sum(sizes)), rel=1e-6)
        assert meters["loss_steps"] == len(sizes)


# ------------------------------------------------------------------------------------------------------- 10. host reads
class _Count:
    """counts Tensor.item / .cpu / .tolist / .numpy and torch.cuda.synchronize calls; device_only: only those on GPU tensors"""

    def __init__(self, device_only=False):
        self.n = 0
        self.saved = []
        self.device_only = device_only

    def __enter__(self):
        T = torch.Tensor
        for obj, name in ((T, "item"), (T, "cpu"), (T, "tolist"), (T, "numpy"), (torch.cuda, "synchronize")):
            orig = getattr(obj, name)
            self.saved.append((obj, name, orig))

            def wrap(*a, _orig=orig, **k):
                if not (self.device_only and a and torch.is_tensor(a[0]) and not a[0].is_cuda):
                    self.n += 1
                return _orig(*a, **k)
            setattr(obj, name, wrap)
        return self

    def __exit__(self, *exc):
        for obj, name, orig in self.saved:
            setattr(obj, name, orig)


@pytest.mark.parametrize("optimizer, criterion", [("fused", "mse"), ("fused", "l1"), ("stock", "l1")])
def test_host_reads_do_not_grow_with_batches(M, G, optimizer, criterion):
    """3 and 30 batches cost the same number of host reads, at most 2 (the meters' one .cpu() and its .tolist()).  With a stock
    torch.optim.Adam only reads of GPU tensors are counted: that optimizer keeps its step counts in CPU tensors and calls
    .item() on them at every step, which reads nothing from the device."""
    t3, i2 = dev(G["s_t3d"]), dev(G["s_i2d"])
    model = PU.load_initial(PU.make_model("single"), G, "single").cuda()
    opt = M.T.posenet_optimizer(model, 1e-4) if optimizer == "fused" else torch.optim.Adam(model.parameters(), lr=1e-4)
    crit = nn.MSELoss(reduction="mean") if criterion == "mse" else nn.L1Loss()
    n = []
    for nb in (3, 30):
        batches = [(t3[(16 * b) % 480:(16 * b) % 480 + 32], i2[(16 * b) % 480:(16 * b) % 480 + 32], None, None) for b in range(nb)]
        M.T.train_posenet(model, batches, opt, crit, torch.device("cuda"), PU.loop_args())   # warm-up
        with _Count(device_only=(optimizer == "stock")) as c:
            M.T.train_posenet(model, batches, opt, crit, torch.device("cuda"), PU.loop_args())
        assert M.T.train_posenet.last_meters["steps"] == 2 * nb
        n.append(c.n)
    print("host reads", optimizer, criterion, n)
    assert n[0] == n[1] and n[0] <= 2, n


# ------------------------------------------------------------------------------------------- 11. the GAN epoch's product
class _Summary:
    def __init__(self, epoch=0):
        self.epoch, self.train_iter_num, self.train_discrim_iter_num = epoch, 0, 0

    def summary_train_iter_num_update(self):
        self.train_iter_num += 1


class _Recording(nn.Module):
    """a posenet that keeps (on the device) which pairs it was shown: the payload's first coordinate is the pair's index"""

    def __init__(self, inner):
        super().__init__()
        self.inner, self.seen = inner, []

    def forward(self, x):
        self.seen.append(x.detach().reshape(x.shape[0], -1)[:, 0].clone())
        return self.inner(x)


def test_fake_pair_buffer_trains_the_posenet(M, G):
    """one iteration of the existing GAN loop fills a FakePairBuffer; train_posenet consumes it (one permutation, one
    dhaug_pair_batch launch per batch) and visits every pair exactly once"""
    import golden_util as GU
    from dhaug_amd.function_aug.config import get_parse_args
    from dhaug_amd.models_Fk_GAN import forward_kinematics_DH_model as fkm, model_fk_gan_train as train
    B = 128
    args = get_parse_args(["--batch_size", str(B), "--Gen_DenseDim", "64", "--Dis_DenseDim_3D", "64", "--Dis_DenseDim_2D", "64"])
    fk = fkm.Forward_Kinematics_DH_Model(args, ["S1"], None)
    torch.manual_seed(3)
    d = train.my_get_poseFk_model(args, None, fk)
    cam = np.load(os.path.join(ROOT, "tests", "golden", "camera_128.npz"))
    q, t, c9 = cam["R"][0].tolist(), cam["t"][0].tolist(), cam["cam"][0].tolist()
    a, bl, rt = GU.synth_fk_inputs(B, 40)
    world = M.ops.fk_forward((a * 0.25).cuda(), bl.cuda(), (rt * 0.2).cuda())
    c3, p2 = M.ops.world_to_camera_project(world, q, t, c9)
    cp = torch.zeros(B, 16)
    cp[:, 9:13], cp[:, 13:16] = torch.tensor(q), torch.tensor(t)
    data = dict(train_gt2d3d_loader=[(c3.cpu(), None, None, cp)], target_2d_loader=[p2.cpu()], target_3d_loader=[None])
    s = _Summary()
    train.GAN_solutions_FK_generator(args, d, data, None, s, None, ["S1", "S5"])
    assert s.train_iter_num == 1
    buf = data["train_fake2d3d_loader"]
    assert isinstance(buf, train.FakePairBuffer) and buf.tensors()[0].shape == (B, 16, 3)
    buf.batch_size = 48                                           # 48 + 48 + 32
    model = _Recording(PU.StubPosenet()).cuda()
    opt = M.T.posenet_optimizer(model, 1e-3)
    before = [p.detach().clone() for p in model.parameters()]
    pa = PU.loop_args()
    M.T.train_posenet(model, buf, opt, nn.MSELoss(reduction="mean"), torch.device("cuda"), pa)
    m = M.T.train_posenet.last_meters
    assert m["steps"] == 6 and m["loss_poses"] == B and np.isfinite(m["loss"])
    assert all(torch.isfinite(p).all().item() and not torch.equal(p, q0) for p, q0 in zip(model.parameters(), before))
    # the same buffer with an index-valued payload: every pair once in the plain steps, once (negated x) in the flipped ones
    buf.p2 = [torch.arange(1, B + 1, device="cuda", dtype=torch.float32).view(B, 1, 1).expand(B, 16, 2).contiguous()]
    model.seen = []
    M.T.train_posenet(model, buf, opt, nn.MSELoss(reduction="mean"), torch.device("cuda"), pa)
    plain, flipped = torch.cat(model.seen[0::2]), torch.cat(model.seen[1::2])
    want = torch.arange(1, B + 1, device="cuda", dtype=torch.float32)
    assert torch.equal(plain.sort().values, want) and torch.equal((-flipped).sort().values, want)
    assert torch.equal(plain, -flipped) and not torch.equal(plain, want)          # same order in both steps, and shuffled
    # the clips of the video epoch's product through GAN_dataSet_video_mode_train_posenet: one 3D target per 2D frame row
    R = PU.FRAMES
    vbuf = train.FakePairBuffer(16)
    vbuf.append(torch.randn(40, R, 16, 3).cuda(), torch.randn(40, R, 16, 2).cuda(), [0.0] * 9)

    class PerFrame(nn.Module):                                    # (n, R, 16, 2) -> (n R, 1, 16, 3)
        def __init__(self):
            super().__init__()
            self.net = PU.StubPosenet()

        def forward(self, x):
            return self.net(x.reshape(-1, 16, 2)).view(-1, 1, 16, 3)

    vm = PerFrame().cuda()
    M.V.GAN_dataSet_video_mode_train_posenet(vm, vbuf, M.T.posenet_optimizer(vm, 1e-3), nn.MSELoss(), torch.device("cuda"), pa)
    vmeters = M.V.GAN_dataSet_video_mode_train_posenet.last_meters
    assert vmeters["steps"] == 12 and vmeters["loss_poses"] == 40 and np.isfinite(vmeters["back_flip_loss"])


def test_device_resident_loader_equals_uploaded_batches(M, G):
    """a TensorLoader source (one permutation, index slices into dhaug_pair_batch) leaves the same bits as the same shuffled
    batches handed over as a plain list"""
    from dhaug_amd.function_aug.dataloader_update import TensorLoader
    t3, i2 = dev(G["s_t3d"]), dev(G["s_i2d"])
    n, B = t3.shape[0], 96
    runs = []
    for flat in (True, False):
        model = PU.load_initial(PU.make_model("single"), G, "single").cuda()
        opt = M.T.posenet_optimizer(model, PU.LR)
        torch.manual_seed(11)
        if flat:
            loader = TensorLoader([t3, i2, torch.zeros(n, 9, device="cuda")], B)
        else:
            perm = torch.randperm(n, device="cuda")
            loader = [(t3[perm[i:i + B]], i2[perm[i:i + B]], None, None) for i in range(0, n, B)]
        M.T.train_posenet(model, loader, opt, nn.MSELoss(reduction="mean"), torch.device("cuda"), PU.loop_args())
        runs.append((PU.state_arrays(model), M.T.train_posenet.last_trace.cpu().numpy(), M.T.train_posenet.last_meters))
    (sa, ta, ma), (sb, tb, mb) = runs
    assert ma["steps"] == 12 and ma == mb and np.array_equal(ta, tb)
    assert all(np.array_equal(sa[k], sb[k]) for k in sa)
    assert not np.array_equal(ta[:, 0], G["single_losses"].astype(np.float32))          # (shuffled: not the fixture's order)
