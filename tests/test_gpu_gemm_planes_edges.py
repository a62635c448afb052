"""The planes contract of the layer GEMMs that write their result once more as the next layer's operand (dhaug_gemm_f16x3_planes: two
IEEE-half pieces [hi|lo] of planes_kp >= N columns, the pad [N, planes_kp) zero; dhaug_gemm_bf16x6_planes: three bf16 pieces of N columns), at
the smallest shapes where it can break: one-row batches and a second row block of one row, the shortest plane operand (kp = 64: three
K-tiles), a pad that ends inside the only column tile / at a tile edge / BEYOND the column tiles of N, a piece width that is no power of
two, row pitches wider than the minimum.  Kernel-level tests run on caller-owned buffers poisoned with NaN bit patterns; the Python chain
(autograd_ops._raw_linear, the modules at a DenseDim the fused programs do not cover) runs with every torch.empty buffer poisoned; and an
in-place write to an activation between two layers must not leave the producing layer's planes behind."""
import argparse
import sys

import pytest
import torch

import golden_util as GU

pytestmark = pytest.mark.gpu

NAN = float("nan")


@pytest.fixture(scope="module")
def M():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import dhaug_amd
    from dhaug_amd import autograd_ops, ops
    dhaug_amd._lib.lib()            # fail loudly if the HIP extension is missing
    return argparse.Namespace(ops=ops, lib=sys.modules["dhaug_amd._lib"], A=autograd_ops)


def maxabs(a, b):
    return (a.detach().cpu().double() - b.detach().cpu().double()).abs().max().item()


def bits(t):
    """the tensor's bit patterns as integers of its element size (NaN == NaN, -0.0 != 0.0)"""
    return t.view({2: torch.int16, 4: torch.int32}[t.element_size()])


# ------------------------------------------------------------------------------------------ dhaug_gemm_f16x3_planes, direct calls
def _f16x3_call(M, A, a_planes, B, bias, res, rows, N, kp, planes_kp):
    """one call on poisoned caller-owned outputs with 8 guard columns behind every row: (c_f32 (rows, N + 8), planes as int16 (rows,
    2 planes_kp + 8))"""
    ldp, ldc = 2 * planes_kp + 8, N + 8
    cp = torch.full((rows, ldp), -1, dtype=torch.int16, device="cuda")          # 0xFFFF: a NaN in IEEE half
    cf = torch.full((rows, ldc), NAN, device="cuda")
    M.lib.call("dhaug_gemm_f16x3_planes", A.data_ptr(), A.stride(0), int(a_planes), B.data_ptr(), B.stride(0), bias.data_ptr(), res.data_ptr(),
               res.stride(0), cf.data_ptr(), ldc, cp.data_ptr(), ldp, planes_kp, rows, N, kp, 1, 0.0, M.ops._stream())
    return cf, cp


# (N, planes_kp): no pad at all | pad inside the only tile | the second tile holds 8 real columns, then pad up to its edge | the smallest N
# whose pad outruns the tiles: [768, 1024) has no tile of N's | N on a tile edge: the whole pad without a tile | a piece width that is no
# power of two: one 8-column group beyond the tiles | three whole tiles' worth of pad beyond the grid of N
F16_CASES = [(64, 64), (72, 128), (264, 512), (520, 1024), (768, 1024), (520, 776), (1032, 2048)]


@pytest.mark.parametrize("K", [64, 72])                       # piece width 64 (three K-tiles: an odd count) and 128
@pytest.mark.parametrize("rows", [1, 257])                    # one row; a second row block that holds a single row
@pytest.mark.parametrize("N,planes_kp", F16_CASES)
def test_f16x3_planes_pad_split_and_guards(M, N, planes_kp, rows, K):
    """relu(x W^T + b + res) with the result's planes: (a) the result against fp64, (b) the planes are the split of the kernel's own
    result, computed here with torch on the CPU, bit for bit, (c) the pad columns [N, planes_kp) of both pieces are all-zero bits, (d) the
    guard columns behind every row are untouched, (e) the two-piece and the three-segment form of the activation operand give the same
    bits, (f) a second layer consumes the planes where they lie: same bits as on a split of the result, and right against fp64."""
    ops = M.ops
    g = torch.Generator().manual_seed(1000 * N + 10 * rows + K)
    kp = 64 if K <= 64 else 128
    x = torch.randn(rows, K, generator=g)
    W = torch.randn(N, K, generator=g) / K ** 0.5
    bias, res = torch.randn(N, generator=g), torch.randn(rows, N, generator=g)
    ref = torch.relu(x.double() @ W.double().t() + bias.double() + res.double())
    tol = 3e-6 * max(1.0, ref.abs().max().item())
    x, W, bias, res = x.cuda(), W.cuda(), bias.cuda(), res.cuda()
    B3 = ops.split_f16(W, 1, kp)
    cf, cp = _f16x3_call(M, ops.split_f16(x, 2, kp), 1, B3, bias, res, rows, N, kp, planes_kp)
    cf0, cp0 = _f16x3_call(M, ops.split_f16(x, 0, kp), 0, B3, bias, res, rows, N, kp, planes_kp)
    torch.cuda.synchronize()
    y = cf[:, :N].cpu()
    # (a)
    assert bool(torch.isfinite(y).all())
    assert maxabs(y, ref) <= tol, (maxabs(y, ref), tol)
    # (b)
    hi = y.half()
    lo = (y - hi.float()).half()
    planes = cp.cpu()
    assert torch.equal(planes[:, :N], bits(hi)) and torch.equal(planes[:, planes_kp:planes_kp + N], bits(lo))
    # (c)
    pad = torch.cat((planes[:, N:planes_kp], planes[:, planes_kp + N:2 * planes_kp]), dim=1)
    assert int((pad != 0).sum()) == 0, "%d of %d pad elements are not zero bits" % (int((pad != 0).sum()), pad.numel())
    # (d)
    assert bool((planes[:, 2 * planes_kp:] == -1).all()) and bool(torch.isnan(cf[:, N:]).all())
    # (e)
    assert torch.equal(bits(cf0), bits(cf)) and torch.equal(cp0, cp)
    # (f)
    if planes_kp & (planes_kp - 1) == 0:
        W2 = torch.randn(64, N, generator=g) / N ** 0.5
        ref2 = ref @ W2.double().t()
        B2 = ops.split_f16(W2.cuda(), 1, planes_kp)
        fed = cp.view(torch.float16)[:, :2 * planes_kp]                         # (a strided view: the guard stays outside)
        nxt = ops.gemm_nt_f16x3_planes(fed, B2, 64, planes_kp, True)
        assert torch.equal(nxt, ops.gemm_nt_f16x3_planes(ops.split_f16(cf[:, :N], 2, planes_kp), B2, 64, planes_kp, True))
        assert maxabs(nxt, ref2) <= 3e-6 * max(1.0, ref2.abs().max().item()), maxabs(nxt, ref2)


# ------------------------------------------------------------------------------------------ dhaug_gemm_bf16x6_planes with c_planes
@pytest.mark.parametrize("order", [0, 1, 2])
@pytest.mark.parametrize("rows", [1, 257])
@pytest.mark.parametrize("N", [64, 512, 1024])
def test_bf16x6_planes_out_at_small_shapes(M, N, rows, order):
    """the result's three bf16 pieces [hi|mid|lo] of N columns each (no pad) from the epilogue: plane operand (x_order 0 / 1, piece width 64,
    fp32 residual and fp32 mask: the epilogue that loads per row group) and the six-segment operand of a narrow input layer (x_order 2,
    K = 30 in segments of 32; bias + ReLU: the epilogue without loads); result against fp64, planes against a torch split on the CPU
    (round to nearest even), guards untouched."""
    ops = M.ops
    g = torch.Generator().manual_seed(100 * N + 10 * rows + order)
    K, kp = (30, 32) if order == 2 else (64, 64)
    x = torch.randn(rows, K, generator=g)
    W = torch.randn(N, K, generator=g) / K ** 0.5
    bias, res, msk = torch.randn(N, generator=g), torch.randn(rows, N, generator=g), torch.randn(rows, N, generator=g)
    z = x.double() @ W.double().t() + bias.double()
    if order == 2:
        ref = torch.relu(z)
    else:
        ref = (z + res.double()) * torch.where(msk > 0, 1.0, 0.2).double()
    xd, Wd, bias, res, msk = x.cuda(), W.cuda(), bias.cuda(), res.cuda(), msk.cuda()
    if order == 2:
        A, B6 = ops.split_bf16(xd, 0, 6, kp), ops.split_bf16(Wd, 1, 6, kp)
    else:
        A, B6 = ops.split_bf16(xd, 2, 6, kp), ops.split_bf16(Wd, 1 - order, 6, kp)
    ldp, ldc = 3 * N + 8, N + 8
    cp = torch.full((rows, ldp), -1, dtype=torch.int16, device="cuda")
    cf = torch.full((rows, ldc), NAN, device="cuda")
    if order == 2:
        M.lib.call("dhaug_gemm_bf16x6_planes", A.data_ptr(), A.stride(0), B6.data_ptr(), B6.stride(0), bias.data_ptr(), None, 0, None, 0, 0, 0.0,
                   cf.data_ptr(), ldc, cp.data_ptr(), ldp, rows, N, kp, 2, 1, 0.0, ops._stream())
    else:
        M.lib.call("dhaug_gemm_bf16x6_planes", A.data_ptr(), A.stride(0), B6.data_ptr(), B6.stride(0), bias.data_ptr(), res.data_ptr(), res.stride(0),
                   msk.data_ptr(), msk.stride(0), 2, 0.2, cf.data_ptr(), ldc, cp.data_ptr(), ldp, rows, N, kp, order, 0, 0.0, ops._stream())
    torch.cuda.synchronize()
    y = cf[:, :N].cpu()
    assert bool(torch.isfinite(y).all())
    assert maxabs(y, ref) <= 2e-6 * ref.abs().max().item(), (maxabs(y, ref), ref.abs().max().item())
    hi = y.bfloat16()
    r1 = y - hi.float()
    mid = r1.bfloat16()
    lo = (r1 - mid.float()).bfloat16()
    planes = cp.cpu()
    assert torch.equal(planes[:, :N], bits(hi)) and torch.equal(planes[:, N:2 * N], bits(mid)) and torch.equal(planes[:, 2 * N:3 * N], bits(lo))
    assert bool((planes[:, 3 * N:] == -1).all()) and bool(torch.isnan(cf[:, N:]).all())


# ------------------------------------------------------------------------------------------ the Python chain, every torch.empty poisoned
@pytest.fixture
def poisoned_empty(monkeypatch):
    """every floating-point torch.empty result comes back full of NaN: an element that is consumed but never written cannot depend on what
    the allocator happens to hand out"""
    real = torch.empty

    def empty(*a, **k):
        t = real(*a, **k)
        if t.dtype.is_floating_point and t.numel():
            with torch.no_grad():
                t.fill_(NAN)
        return t
    monkeypatch.setattr(torch, "empty", empty)


@pytest.mark.parametrize("D", [520, 640, 768, 1200])
def test_layer_chain_with_poisoned_buffers(M, D, poisoned_empty, monkeypatch):
    """48 -> D -> D -> D as three F16X3_LAYER layers (ReLU; the first layer's result is the last one's residual), the planes of a
    layer's result handed to the next: finite and right against the fp64 chain, and the bits of the chain that splits in a launch of its
    own per layer.  At these widths the planes' piece width (1 024, 2 048) lies beyond the column tiles of D."""
    A = M.A
    rows = 8
    g = torch.Generator().manual_seed(D)
    x = torch.randn(rows, 48, generator=g)
    Ws = [torch.randn(D, 48, generator=g) / 48 ** 0.5, torch.randn(D, D, generator=g) / D ** 0.5, torch.randn(D, D, generator=g) / D ** 0.5]
    bs = [torch.randn(D, generator=g) for _ in range(3)]
    r1 = torch.relu(x.double() @ Ws[0].double().t() + bs[0].double())
    r2 = torch.relu(r1 @ Ws[1].double().t() + bs[1].double())
    ref = torch.relu(r2 @ Ws[2].double().t() + bs[2].double() + r1)
    xd, Wd, bd = x.cuda(), [w.cuda() for w in Ws], [b.cuda() for b in bs]

    def chain():
        with torch.no_grad():
            h1 = A.linear(xd, Wd[0], bd[0], None, A.ACT_RELU, 0.0, A.F16X3_LAYER)
            h2 = A.linear(h1, Wd[1], bd[1], None, A.ACT_RELU, 0.0, A.F16X3_LAYER)
            return A.linear(h2, Wd[2], bd[2], h1, A.ACT_RELU, 0.0, A.F16X3_LAYER)
    assert A.F16X3_PLANES
    got = chain()
    monkeypatch.setattr(A, "F16X3_PLANES", False)
    split = chain()
    err, err_split = maxabs(got, ref), maxabs(split, ref)
    print("D = %d: planes chain %.3e, split chain %.3e of scale %.3e; differing elements %d" % (
        D, err, err_split, ref.abs().max().item(), int((got != split).sum())))
    assert bool(torch.isfinite(got).all())
    assert err <= 3e-6 * max(1.0, ref.abs().max().item()), err
    assert torch.equal(got, split)


def test_modules_with_poisoned_buffers(M, poisoned_empty, monkeypatch):
    """generator, 3D critic and 2D critic at DenseDim 640 (piece width 1 024 beyond the three column tiles of 640) in "f16x3" without a
    graph: finite, the bits of the pass that splits per layer, and within 1e-4 (relative, as tests/test_gpu_loops.py measures the logits)
    of the same modules in "bf16x6"."""
    from test_gpu_models import make_args
    from dhaug_amd.models_Fk_GAN import Fk_discriminator, Fk_generator, forward_kinematics_DH_model
    A = M.A
    B, D = 8, 640
    args = make_args(batch_size=B, Gen_DenseDim=D, Dis_DenseDim_3D=D, Dis_DenseDim_2D=D)
    fk = forward_kinematics_DH_model.Forward_Kinematics_DH_Model(args, ["S1"], None)
    G = Fk_generator.Fk_Generator(fk, args, "cuda")
    D3, D2 = Fk_discriminator.Fk_3D_Discriminator("cuda", args), Fk_discriminator.Fk_2D_Discriminator(args, 16)
    for net, shapes, seed in ((G, GU.shapes_generator(D), 31), (D3, GU.shapes_d3(D), 32), (D2, GU.shapes_d2(D), 33)):
        net.load_state_dict(GU.seeded_state_dict(shapes, seed))
        net.cuda()
    g = torch.Generator().manual_seed(34)
    z = torch.randn(B, 128, generator=g).cuda()
    scaler = (torch.randint(-200, 200, (B, 8), generator=g).float() / 1000.0).cuda()
    x3 = GU.synth_pose16(B, seed=35)
    x3 = (x3 - x3[:, :1]).cuda()
    x2 = ((torch.rand(B, 16, 2, generator=g) - 0.5) * 1.6).cuda()
    G.GAN_generator_get_bone_length(GU.synth_pose16(B, seed=36).cuda())
    rel = lambda a, b: ((a.detach().double().cpu() - b.detach().double().cpu()).abs()
                        / b.detach().double().cpu().abs().clamp_min(0.1 * b.detach().double().cpu().abs().mean())).max().item()

    def run(prec):
        for net in (G, D3, D2):
            net.precision = prec
        with torch.no_grad():
            return dict(fake=G(z, bone_len_scaler=scaler), l3=D3(x3), l2=D2(x2))
    assert A.F16X3_PLANES
    got = run("f16x3")
    monkeypatch.setattr(A, "F16X3_PLANES", False)
    split = run("f16x3")
    wide = run("bf16x6")
    for k in ("fake", "l3", "l2"):
        print("DenseDim %d %s: %.3e rel of bf16x6; differing elements %d" % (D, k, rel(got[k], wide[k]), int((got[k] != split[k]).sum())))
    assert got["fake"].shape == (B, 48) and got["l3"].shape == (B, 1) and got["l2"].shape == (B, 1)
    for k in ("fake", "l3", "l2"):
        assert bool(torch.isfinite(got[k]).all()), k
        assert torch.equal(got[k], split[k]), k
        assert rel(got[k], wide[k]) <= 1e-4, (k, rel(got[k], wide[k]))


# ------------------------------------------------------------------------------------------ planes must not outlive an in-place write
@pytest.mark.parametrize("write", ["none", "mul_", "zero_columns"])
def test_planes_do_not_outlive_an_in_place_write(M, write, monkeypatch):
    """a layer's planes hang on the activation it returns; after an in-place write to that activation the next layer has to multiply the
    NEW values (as it does for a clone, which carries no planes), and without a write it still takes the planes: no split launch"""
    A = M.A
    rows, D = 8, 256
    g = torch.Generator().manual_seed(17)
    x = torch.randn(rows, 48, generator=g).cuda()
    W1, b1 = (torch.randn(D, 48, generator=g) / 48 ** 0.5).cuda(), torch.randn(D, generator=g).cuda()
    W2, b2 = (torch.randn(D, D, generator=g) / D ** 0.5).cuda(), torch.randn(D, generator=g).cuda()
    calls = []
    real = M.lib.call
    # (dhaug_split_f16's seventh argument is the mode: 1 is the weight side, split anew for a weight that is no nn.Parameter)
    monkeypatch.setattr(M.lib, "call", lambda name, *a: (calls.append((name, a[6] if name == "dhaug_split_f16" else None)), real(name, *a))[1])
    with torch.no_grad():
        h = A.linear(x, W1, b1, None, A.ACT_RELU, 0.0, A.F16X3_LAYER)
        assert getattr(h, "_dhaug_f16_planes", None) is not None
        if write == "mul_":
            h.mul_(0.5)
        elif write == "zero_columns":
            h[:, :8].zero_()
        del calls[:]
        got = A.linear(h, W2, b2, None, A.ACT_RELU, 0.0, A.F16X3_LAYER)
        n_split = sum(1 for name, mode in calls if name == "dhaug_split_f16" and mode != 1)
        want = A.linear(h.clone(), W2, b2, None, A.ACT_RELU, 0.0, A.F16X3_LAYER)
    assert torch.equal(got, want)
    if write == "none":
        assert getattr(h, "_dhaug_f16_planes", None) is not None and n_split == 0
    ref = torch.relu(h.double().cpu() @ W2.double().cpu().t() + b2.double().cpu())
    assert maxabs(got, ref) <= 3e-6 * max(1.0, ref.abs().max().item())
