"""GPU tests of the LayerNorm, attention and GELU kernels (csrc/dhaug_attn.hip) through the C-ABI, each against fp64 torch on the same
inputs.  The bound for all three: the error of a tensor, max|t - ref| / max|ref|, is at most 4 x max(e, 2^-23) with e the error of
torch's own fp32 op on this GPU against the same fp64 reference; both figures are printed ("FIGURE ...") before the assertion.  A
bf16 output equals the same call's fp32 output rounded to nearest-even, bit for bit.  Pitches are wider than the tensors, the
columns behind them poisoned and found untouched."""
import math
import os
import sys

import pytest
import torch
import torch.nn.functional as F

import poseformer_util as FU

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
ONE_ROUNDING = 2.0 ** -23
BF16 = torch.bfloat16
EUNSUPPORTED = -3
POISON = 7.5e37


@pytest.fixture(scope="module")
def L():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    sys.path.insert(0, ROOT)
    import dhaug_amd
    return dhaug_amd._lib


def stream():
    return torch.cuda.current_stream().cuda_stream or None


def rel(t, ref):
    return (t.double() - ref.double()).abs().max().item() / max(ref.double().abs().max().item(), 1e-300)


def check(name, ours, stock, ref):
    e, s = rel(ours, ref), rel(stock, ref)
    print("FIGURE %s ours %.4g torch_fp32 %.4g" % (name, e, s))
    assert torch.isfinite(ours).all(), name
    assert e <= 4 * max(s, ONE_ROUNDING), (name, e, s)


def padded(t, extra=4, dtype=None):
    """t in the first columns of a wider matrix whose other columns are poisoned: (matrix, view of t's columns, pitch)"""
    dtype = t.dtype if dtype is None else dtype
    full = torch.full((t.shape[0], t.shape[1] + extra), POISON, dtype=dtype, device=t.device)
    full[:, :t.shape[1]] = t.to(dtype)
    return full, full[:, :t.shape[1]], full.stride(0)


def blank(M, C, dtype, extra=4):
    full = torch.full((M, C + extra), POISON, dtype=dtype, device="cuda")
    return full, full[:, :C], full.stride(0)


def untouched(full, C):
    return bool((full[:, C:].float() == torch.tensor(POISON, dtype=full.dtype).float().item()).all())


# ------------------------------------------------------------------------------------------------------------ LayerNorm
def ln_forward(L, xv, ldx, gamma, beta, eps, M, C, out_dtype):
    yf, yv, ldy = blank(M, C, out_dtype)
    mean = torch.empty(M, device="cuda")
    rstd = torch.empty(M, device="cuda")
    L.call("dhaug_layernorm_forward", xv.data_ptr(), int(xv.dtype == BF16), ldx, gamma.data_ptr(), beta.data_ptr(), eps, yf.data_ptr(),
           int(out_dtype == BF16), ldy, mean.data_ptr(), rstd.data_ptr(), M, C, stream())
    assert untouched(yf, C)
    return yv, mean, rstd


def ln_backward(L, xv, ldx, gv, ldg, gamma, mean, rstd, M, C, out_dtype=torch.float32):
    df, dv, ldd = blank(M, C, out_dtype)
    dgamma = torch.full((C,), POISON, device="cuda")
    dbeta = torch.full((C,), POISON, device="cuda")
    ws = torch.full((L.layernorm_workspace_doubles(C),), float("nan"), dtype=torch.float64, device="cuda")
    L.call("dhaug_layernorm_backward", xv.data_ptr(), int(xv.dtype == BF16), ldx, gv.data_ptr(), int(gv.dtype == BF16), ldg,
           gamma.data_ptr(), mean.data_ptr(), rstd.data_ptr(), df.data_ptr(), int(out_dtype == BF16), ldd, dgamma.data_ptr(),
           dbeta.data_ptr(), ws.data_ptr(), M, C, stream())
    assert untouched(df, C)
    return dv, dgamma, dbeta


# (M, C): every lane layout (4, 16, 64 lanes a row), ragged row counts, one row; the last two walk the parameter-gradient partials more
# than once per row lane (C <= 32: 8 row lanes, above: 4)
LN_CASES = [(1, 16), (5, 32), (67, 80), (130, 512), (3, 1024), (FU.LN_MAX_BLOCKS * FU.LN_PARTIAL_ROWS + 5, 32),
            (FU.LN_MAX_BLOCKS * FU.LN_PARTIAL_ROWS // 2 + 3, 80)]


@pytest.mark.parametrize("M,C", LN_CASES)
def test_layernorm(L, M, C):
    g = torch.Generator().manual_seed(100 * M + C)
    x = (torch.randn(M, C, generator=g) * 1.5 + 0.5).cuda()
    gamma = (torch.rand(C, generator=g) + 0.5).cuda()
    beta = (torch.rand(C, generator=g) - 0.5).cuda()
    gy = torch.randn(M, C, generator=g).cuda()
    eps = 1e-6
    xf, xv, ldx = padded(x)
    gf, gv, ldg = padded(gy, extra=8)
    y, mean, rstd = ln_forward(L, xv, ldx, gamma, beta, eps, M, C, torch.float32)
    yb, _, _ = ln_forward(L, xv, ldx, gamma, beta, eps, M, C, BF16)
    assert torch.equal(yb, y.to(BF16))

    def torch_run(dtype):
        xx, ga, be = (t.detach().clone().to(dtype).requires_grad_() for t in (x, gamma, beta))
        out = F.layer_norm(xx, (C,), ga, be, eps)
        out.backward(gy.to(dtype))
        return out.detach(), xx.grad, ga.grad, be.grad

    r64, r32 = torch_run(torch.float64), torch_run(torch.float32)
    tag = "layernorm_%dx%d_" % (M, C)
    check(tag + "y", y, r32[0], r64[0])
    check(tag + "mean", mean, x.mean(1), x.double().mean(1))
    check(tag + "rstd", rstd, (x.var(1, unbiased=False) + eps).rsqrt(), (x.double().var(1, unbiased=False) + eps).rsqrt())
    dx, dgamma, dbeta = ln_backward(L, xv, ldx, gv, ldg, gamma, mean, rstd, M, C)
    check(tag + "dx", dx, r32[1], r64[1])
    check(tag + "dgamma", dgamma, r32[2], r64[2])
    check(tag + "dbeta", dbeta, r32[3], r64[3])
    dx2, dgamma2, dbeta2 = ln_backward(L, xv, ldx, gv, ldg, gamma, mean, rstd, M, C)
    assert torch.equal(dx, dx2) and torch.equal(dgamma, dgamma2) and torch.equal(dbeta, dbeta2)
    dxb, _, _ = ln_backward(L, xv, ldx, gv, ldg, gamma, mean, rstd, M, C, BF16)
    assert torch.equal(dxb, dx.to(BF16))
    # bf16 input and cotangent: the kernel's arithmetic on the rounded values
    xb_f, xb, ldxb = padded(x, dtype=BF16)
    gb_f, gb, ldgb = padded(gy, dtype=BF16)
    y16, mean16, rstd16 = ln_forward(L, xb, ldxb, gamma, beta, eps, M, C, torch.float32)
    x16 = x.to(BF16).double().requires_grad_()
    ref16 = F.layer_norm(x16, (C,), gamma.double(), beta.double(), eps)
    ref16.backward(gy.to(BF16).double())
    check(tag + "y_bf16_in", y16, F.layer_norm(x.to(BF16).float(), (C,), gamma, beta, eps), ref16.detach())
    dx16, _, _ = ln_backward(L, xb, ldxb, gb, ldgb, gamma, mean16, rstd16, M, C)
    xs = x.to(BF16).float().requires_grad_()
    F.layer_norm(xs, (C,), gamma, beta, eps).backward(gy.to(BF16).float())
    check(tag + "dx_bf16_in", dx16, xs.grad, x16.grad)
    assert untouched(xf, C) and untouched(gf, C)


def test_layernorm_constant_and_offset_rows(L):
    """a constant row gives beta exactly (mean = the constant, centred values 0); a row of 1 000 + N(0, 1e-3) keeps the variance of
    its centred values (E[x^2] - mean^2 in fp32 would lose it whole: 1e6 against 1e-6)"""
    C = 80
    g = torch.Generator().manual_seed(9)
    gamma = (torch.rand(C, generator=g) + 0.5).cuda()
    beta = (torch.rand(C, generator=g) - 0.5).cuda()
    x = torch.empty(4, C)
    x[0], x[1], x[2] = 0.1, -1234.567, 3.0e-5
    x[3] = 1000.0 + 1e-3 * torch.randn(C, generator=g)
    x = x.cuda()
    for eps in (1e-6, 1e-5):
        y, mean, rstd = ln_forward(L, x, C, gamma, beta, eps, 4, C, torch.float32)
        for r in range(3):
            assert torch.equal(y[r], beta), r
            assert mean[r].item() == x[r, 0].item()
        ref = F.layer_norm(x[3:].double(), (C,), gamma.double(), beta.double(), eps)
        check("layernorm_offset_row_eps%g" % eps, y[3:], F.layer_norm(x[3:], (C,), gamma, beta, eps), ref)
        var = x[3].double().var(unbiased=False).item()
        assert abs(rstd[3].item() * math.sqrt(var + eps) - 1) < 1e-5


# ------------------------------------------------------------------------------------------------------------ attention
ATTN_CASES = [(1, 1, 1, 4), (3, 5, 4, 4), (7, 16, 8, 4), (2, 3, 4, 20), (3, 9, 8, 64), (2, 27, 4, 64), (1, 81, 2, 64)]


def attn_ref(qkv, S, N, H, hd, scale, gout=None):
    """the torch expression the kernel replaces, in qkv's dtype: (out, lse[, dqkv])"""
    C = H * hd
    leaf = qkv.detach().clone().requires_grad_(gout is not None)
    q, k, v = leaf.view(S, N, 3, H, hd).permute(2, 0, 3, 1, 4)
    s = (q @ k.transpose(-2, -1)) * scale
    out = (s.softmax(dim=-1) @ v).transpose(1, 2).reshape(S * N, C)
    lse = torch.logsumexp(s, dim=-1)
    if gout is None:
        return out.detach(), lse.detach()
    out.backward(gout)
    return out.detach(), lse.detach(), leaf.grad


def attn_forward(L, qv, ld, S, N, H, hd, scale, out_dtype):
    C = H * hd
    of, ov, ldo = blank(S * N, C, out_dtype)
    lse = torch.full((S, H, N), POISON, device="cuda")
    L.call("dhaug_attn_forward", qv.data_ptr(), int(qv.dtype == BF16), ld, of.data_ptr(), int(out_dtype == BF16), ldo, lse.data_ptr(),
           S, N, H, hd, scale, stream())
    assert untouched(of, C)
    return ov, lse


def attn_backward(L, qv, ld, ov, ldo, lse, gv, ldg, S, N, H, hd, scale, out_dtype):
    C = H * hd
    df = torch.full((S * N, 3 * C + 8), float("nan"), dtype=out_dtype, device="cuda")
    L.call("dhaug_attn_backward", qv.data_ptr(), int(qv.dtype == BF16), ld, ov.data_ptr(), int(ov.dtype == BF16), ldo, lse.data_ptr(),
           gv.data_ptr(), int(gv.dtype == BF16), ldg, df.data_ptr(), int(out_dtype == BF16), df.stride(0), S, N, H, hd, scale, stream())
    assert torch.isnan(df[:, 3 * C:]).all(), "a column behind 3C was written"
    assert not torch.isnan(df[:, :3 * C]).any(), "an element of the qkv cotangent was left unwritten"
    return df[:, :3 * C]


@pytest.mark.parametrize("S,N,H,hd", ATTN_CASES)
def test_attention(L, S, N, H, hd):
    C = H * hd
    scale = hd ** -0.5
    g = torch.Generator().manual_seed(1000 * S + 10 * N + hd)
    qkv = (torch.randn(S * N, 3 * C, generator=g) * 1.5).cuda()
    gout = torch.randn(S * N, C, generator=g).cuda()
    qf, qv, ld = padded(qkv, extra=8)
    gf, gv, ldg = padded(gout)
    out, lse = attn_forward(L, qv, ld, S, N, H, hd, scale, torch.float32)
    outb, _ = attn_forward(L, qv, ld, S, N, H, hd, scale, BF16)
    assert torch.equal(outb, out.to(BF16))
    r64, r32 = attn_ref(qkv.double(), S, N, H, hd, scale, gout.double()), attn_ref(qkv, S, N, H, hd, scale, gout)
    tag = "attn_%d_%d_%d_%d_" % (S, N, H, hd)
    check(tag + "out", out, r32[0], r64[0])
    check(tag + "lse", lse, r32[1], r64[1])
    of, ov, ldo = padded(out)
    dqkv = attn_backward(L, qv, ld, ov, ldo, lse, gv, ldg, S, N, H, hd, scale, torch.float32)
    for third, name in enumerate(("dq", "dk", "dv")):
        cols = slice(third * C, (third + 1) * C)
        check(tag + name, dqkv[:, cols], r32[2][:, cols], r64[2][:, cols])
    again = attn_backward(L, qv, ld, ov, ldo, lse, gv, ldg, S, N, H, hd, scale, torch.float32)
    out2, lse2 = attn_forward(L, qv, ld, S, N, H, hd, scale, torch.float32)
    assert torch.equal(dqkv, again) and torch.equal(out, out2) and torch.equal(lse, lse2)
    assert torch.equal(attn_backward(L, qv, ld, ov, ldo, lse, gv, ldg, S, N, H, hd, scale, BF16), dqkv.to(BF16))
    # bf16 operands throughout (the 'bf16' mode): the kernel's arithmetic on the rounded values
    qb_f, qb, ldb = padded(qkv, extra=8, dtype=BF16)
    gb_f, gb, ldgb = padded(gout, dtype=BF16)
    ob, lseb = attn_forward(L, qb, ldb, S, N, H, hd, scale, torch.float32)
    q16, g16 = qkv.to(BF16), gout.to(BF16)
    b64, b32 = attn_ref(q16.double(), S, N, H, hd, scale, g16.double()), attn_ref(q16.float(), S, N, H, hd, scale, g16.float())
    check(tag + "out_bf16_in", ob, b32[0], b64[0])
    obf, obv, ldob = padded(ob)
    check(tag + "dqkv_bf16_in", attn_backward(L, qb, ldb, obv, ldob, lseb, gb, ldgb, S, N, H, hd, scale, torch.float32), b32[2], b64[2])
    assert untouched(qf, 3 * C) and untouched(gf, C)


def test_attention_large_and_equal_scores(L):
    """scores of +-80 (exp(80) overflows fp32 products of unnormalised weights; exp(-160) underflows): finite, against fp64; equal
    scores give uniform weights"""
    S, N, H, hd = 2, 9, 2, 4
    C = H * hd
    scale = hd ** -0.5
    g = torch.Generator().manual_seed(4)
    qkv = torch.randn(S * N, 3 * C, generator=g)
    qkv[:, :C] = 0
    qkv[:, 0] = 16.0                                  # q = (16, 0, 0, 0) in head 0: score = 0.5 * 16 * k0 = +-80 at k0 = +-10
    qkv[:, C] = torch.where(torch.arange(S * N) % 2 == 0, 10.0, -10.0)
    qkv[:, C + 1:C + hd] = 0
    qkv = qkv.cuda()
    gout = torch.randn(S * N, C, generator=g).cuda()
    out, lse = attn_forward(L, qkv, 3 * C, S, N, H, hd, scale, torch.float32)
    r64, r32 = attn_ref(qkv.double(), S, N, H, hd, scale, gout.double()), attn_ref(qkv, S, N, H, hd, scale, gout)
    assert r64[1][:, 0].max().item() > 80 and torch.isfinite(out).all() and torch.isfinite(lse).all()
    check("attn_pm80_out", out, r32[0], r64[0])
    check("attn_pm80_lse", lse, r32[1], r64[1])
    dqkv = attn_backward(L, qkv, 3 * C, out.contiguous(), C, lse, gout, C, S, N, H, hd, scale, torch.float32)
    check("attn_pm80_dqkv", dqkv, r32[2], r64[2])
    # equal scores: every key the same row
    qkv = torch.randn(S * N, 3 * C, generator=g)
    qkv[:, C:2 * C] = qkv[0, C:2 * C]
    qkv = qkv.cuda()
    out, lse = attn_forward(L, qkv, 3 * C, S, N, H, hd, scale, torch.float32)
    # weights exactly 1 / N (exp(0) = 1, N exact): what is left is the fp32 sum of the N values and two roundings of the quotient;
    # the score is a four-term fp32 dot product
    u = 2.0 ** -24
    v = qkv[:, 2 * C:].double().view(S, N, C)
    mean_v = v.mean(1, keepdim=True).expand(S, N, C).reshape(S * N, C)
    room = ((N + 1) * u * v.abs().mean(1, keepdim=True)).expand(S, N, C).reshape(S * N, C)
    assert ((out.double() - mean_v).abs() <= room).all()
    terms = qkv[:, :C].double().view(S, N, H, hd) * qkv[0, C:2 * C].double().view(1, 1, H, hd)
    score, size = terms.sum(-1) * scale, terms.abs().sum(-1) * scale                                                  # (S, N, H)
    assert ((lse.double() - (score.permute(0, 2, 1) + math.log(N))).abs() <= (hd + 3) * u * (size.permute(0, 2, 1) + math.log(N))).all()


def test_attention_refuses_what_it_does_not_implement(L):
    """N = 82 and hd = 6 come back as DHAUG_EUNSUPPORTED: the outputs keep their poison (nothing was launched)"""
    lib = L.lib()
    for S, N, H, hd in ((1, 82, 2, 4), (2, 5, 2, 6), (1, 5, 1, 68)):
        C = H * hd
        ld = (3 * C + 3) // 4 * 4
        qkv = torch.zeros(S * N, ld, device="cuda")
        out = torch.full((S * N, ld), POISON, device="cuda")
        lse = torch.full((S, H, N), POISON, device="cuda")
        rc = lib.dhaug_attn_forward(qkv.data_ptr(), 0, ld, out.data_ptr(), 0, ld, lse.data_ptr(), S, N, H, hd, 0.5, stream())
        assert rc == EUNSUPPORTED
        dq = torch.full((S * N, ld), POISON, device="cuda")
        rc = lib.dhaug_attn_backward(qkv.data_ptr(), 0, ld, qkv.data_ptr(), 0, ld, lse.data_ptr(), qkv.data_ptr(), 0, ld, dq.data_ptr(), 0,
                                     ld, S, N, H, hd, 0.5, stream())
        assert rc == EUNSUPPORTED
        torch.cuda.synchronize()
        assert (out == POISON).all() and (lse == POISON).all() and (dq == POISON).all()


# ------------------------------------------------------------------------------------------------------------ GELU
def gelu_ref(z, g=None):
    z = z.double()
    cdf = 0.5 * torch.erfc(-z / math.sqrt(2.0))
    if g is None:
        return z * cdf
    return g.double() * (cdf + z * torch.exp(-0.5 * z * z) / math.sqrt(2.0 * math.pi))


# one element, sizes off the four-element vectors, and one beyond a single pass of the capped grid
GELU_SIZES = [1, 63, 257, 4 * FU.GELU_BLOCK * FU.GELU_MAX_BLOCKS + 259]


@pytest.mark.parametrize("n", GELU_SIZES)
def test_gelu(L, n):
    g = torch.Generator().manual_seed(n)
    z = (torch.rand(n, generator=g) * 60 - 30)
    special = torch.tensor([0.0, -0.0, -30.0, 30.0, -12.5, -8.0, -5.5, 1e-30, -1e-30, 5.0])
    k = min(n, special.numel())
    z[:k] = special[:k]
    if n > 64:
        z[32:64] = torch.randn(32, generator=g)                     # the body of the curve as well as its tails
    z = z.cuda()
    gy = torch.randn(n, generator=g).cuda()
    y = torch.full((n + 3,), POISON, device="cuda")
    L.call("dhaug_gelu_forward", z.data_ptr(), n, y.data_ptr(), 0, n, 1, n, stream())
    assert (y[n:] == POISON).all() and not torch.isnan(y).any()
    check("gelu_%d_y" % n, y[:n], F.gelu(z), gelu_ref(z))
    yb = torch.full((n + 3,), POISON, dtype=BF16, device="cuda")
    L.call("dhaug_gelu_forward", z.data_ptr(), n, yb.data_ptr(), 1, n, 1, n, stream())
    assert torch.equal(yb[:n], y[:n].to(BF16)) and (yb[n:].float() == torch.tensor(POISON, dtype=BF16).float().item()).all()
    # the far negative tail keeps its sign and size: -8 Phi(-8) = -4.98e-15 (1 + erf cancels to 0 there)
    if n >= 6:
        assert abs(y[5].item() / gelu_ref(z[5:6]).item() - 1) < 1e-4 and y[2].item() == 0.0
    dz = torch.full((n + 3,), POISON, device="cuda")
    L.call("dhaug_gelu_backward", z.data_ptr(), n, gy.data_ptr(), 0, n, dz.data_ptr(), 0, n, 1, n, stream())
    zz = z.clone().requires_grad_()
    F.gelu(zz).backward(gy)
    assert (dz[n:] == POISON).all() and not torch.isnan(dz).any()
    check("gelu_%d_dz" % n, dz[:n], zz.grad, gelu_ref(z, gy))
    gb = gy.to(BF16)
    dzb = torch.full((n + 3,), POISON, dtype=BF16, device="cuda")
    dzf = torch.full((n + 3,), POISON, device="cuda")
    L.call("dhaug_gelu_backward", z.data_ptr(), n, gb.data_ptr(), 1, n, dzf.data_ptr(), 0, n, 1, n, stream())
    L.call("dhaug_gelu_backward", z.data_ptr(), n, gb.data_ptr(), 1, n, dzb.data_ptr(), 1, n, 1, n, stream())
    assert torch.equal(dzb[:n], dzf[:n].to(BF16))
    check("gelu_%d_dz_bf16_g" % n, dzf[:n], gelu_ref(z, gb).float(), gelu_ref(z, gb))


def test_gelu_rows_with_a_pitch(L):
    """a (M, C) matrix with wider rows, C off the vector grid: the columns behind C are not touched"""
    M, C = 37, 22
    g = torch.Generator().manual_seed(3)
    z = (torch.randn(M, C, generator=g) * 3).cuda()
    zf, zv, ldz = padded(z, extra=6)
    yf, yv, ldy = blank(M, C, torch.float32, extra=2)
    L.call("dhaug_gelu_forward", zv.data_ptr(), ldz, yf.data_ptr(), 0, ldy, M, C, stream())
    assert untouched(yf, C)
    check("gelu_rows_y", yv, F.gelu(z), gelu_ref(z))
    gy = torch.randn(M, C, generator=g).cuda()
    gf, gv, ldg = padded(gy, extra=2)
    df, dv, ldd = blank(M, C, BF16, extra=10)
    L.call("dhaug_gelu_backward", zv.data_ptr(), ldz, gv.data_ptr(), 0, ldg, df.data_ptr(), 1, ldd, M, C, stream())
    ff, fv, ldf = blank(M, C, torch.float32, extra=6)
    L.call("dhaug_gelu_backward", zv.data_ptr(), ldz, gv.data_ptr(), 0, ldg, ff.data_ptr(), 0, ldf, M, C, stream())
    assert untouched(df, C) and untouched(ff, C) and torch.equal(dv, fv.to(BF16))
    zz = z.clone().requires_grad_()
    F.gelu(zz).backward(gy)
    check("gelu_rows_dz", fv, zz.grad, gelu_ref(z, gy))
