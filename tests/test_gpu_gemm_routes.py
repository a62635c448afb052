"""Every NT / TN GEMM route of csrc/dhaug_gemm.hip and csrc/dhaug_gemm_p8.hip at its smallest edge shapes, with every epilogue the
router may hand the kernel (tests/gemm_cases.py; that each case reaches the kernel it names is pinned on the host by
tests/test_cpu_boundary.py::test_gemm_case_table_reaches_every_route).

Every launch runs in hostile surroundings: the operands are column blocks of wider NaN-filled buffers (nothing outside a row's own
columns may reach the result), the outputs are views of sentinel-filled frames (nothing outside the view's own rows and columns may
be written), the values are compared element by element with an fp64 product of the bf16 operands, and a second identical launch
must give the same bits."""
import pytest
import torch

import gemm_cases as G

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
SENTINEL = 7.0
NAN = float("nan")


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import dhaug_amd
    from dhaug_amd import ops as o
    dhaug_amd._lib.lib()            # fail loudly if the HIP extension is missing
    return o


# ------------------------------------------------------------------------------------------------------------ shared references
_PRODUCTS = {}


def nt_product(M, N, K):
    """bf16 operands (CPU) and their fp64 product, computed once per shape and never modified"""
    key = (M, N, K)
    if key not in _PRODUCTS:
        gen = torch.Generator().manual_seed(1000003 * M + 1009 * N + K)
        A = (torch.randn(M, K, generator=gen) * 0.5).to(BF16)
        B = (torch.randn(N, K, generator=gen) / K ** 0.5).to(BF16)
        _PRODUCTS[key] = (A, B, A.double() @ B.double().t())
    return _PRODUCTS[key]


def hostile(data, ld, dtype):
    """`data` (CPU, rows x width) as the column block [1 : rows + 1, 8 : 8 + width] of a NaN-filled (rows + 2, ld) device buffer: row
    stride ld >= width + 16, 16-byte aligned start (8 elements into a row whose stride is a multiple of 16 bytes)"""
    rows, width = data.shape
    assert ld >= width + 16
    buf = torch.full((rows + 2, ld), NAN, dtype=dtype, device="cuda")
    view = buf[1:rows + 1, 8:8 + width]
    view.copy_(data)
    assert view.data_ptr() % 16 == 0 and view.stride(0) == ld
    return view


def frame(rows, width, ld, dtype):
    """an output view [:rows, :width] of a (rows + 8, ld) buffer filled with the sentinel, ld >= width + 16"""
    assert ld >= width + 16
    buf = torch.full((rows + 8, ld), SENTINEL, dtype=dtype, device="cuda")
    return buf, buf[:rows, :width]


def untouched_outside(buf, rows, cols):
    """every element of the frame outside [0, rows) x [0, cols) still holds the sentinel"""
    return bool((buf[rows:] == SENTINEL).all()) and bool((buf[:rows, cols:] == SENTINEL).all())


def mask_values(M, N, gen):
    """mask entries with an exact zero and a negative zero among them (both count as `not positive`)"""
    m = torch.randn(M, N, generator=gen)
    flat = m.view(-1)
    flat[0] = 0.0
    flat[flat.numel() // 2] = -0.0
    if flat.numel() > 2:
        flat[-1] = 0.0
        flat[flat.numel() // 3] = -0.0
    return m


# ----------------------------------------------------------------------------------------------------------------------- NT
def run_nt(ops, c, monkeypatch):
    import dhaug_amd
    for name in G.SWITCHES:
        monkeypatch.delenv(name, raising=False)
    for name, value in c.env:
        monkeypatch.setenv(name, value)             # (the dispatcher reads the switches on every call)
    M, N, K = c.M, c.N, c.K
    A, B, pre = nt_product(M, N, K)
    gen = torch.Generator().manual_seed(7 * M + 3 * N + K + c.act)
    a, b = hostile(A, c.lda, BF16), hostile(B, c.ldb, BF16)
    ref = pre
    bias = None
    if c.bias:
        bias_buf = torch.full((N + 16,), NAN, device="cuda")
        lead = 4 + c.bias_off // 4                  # 16 bytes into the buffer, plus the case's misalignment
        bias = bias_buf[lead:lead + N]
        bias_cpu = torch.randn(N, generator=gen)
        bias.copy_(bias_cpu)
        assert bias.data_ptr() % 16 == c.bias_off % 16
        ref = ref + bias_cpu.double()
    res = None
    if c.res == "bf16":
        r = torch.randn(M, N, generator=gen).to(BF16)
        res = hostile(r, c.ld_res, BF16)
        ref = ref + r.double()
    elif c.res == "f32":
        r = torch.randn(M, N, generator=gen)
        res = hostile(r, c.ld_res, torch.float32)
        ref = ref + r.double()
    mask = None
    if c.mask is None:
        if c.act == 1:
            ref = torch.relu(ref)
        elif c.act == 2:
            ref = torch.nn.functional.leaky_relu(ref, c.slope)
    else:
        m = mask_values(M, N, gen)
        if c.mask == "bf16":
            m = m.to(BF16)
        mask = hostile(m, c.ld_mask, m.dtype)
        pos = (m.float() > 0).double()
        ref = ref * (pos + (1 - pos) * (0.0 if c.act == 1 else c.slope))
    scale = max(1.0, ref.abs().max().item())
    delta = (3e-5 if (c.bias or c.res or c.mask) else 2e-5) * scale

    def launch():
        fb = frame(M, c.bf16_width, c.ldc_bf16, BF16) if c.out_bf16 else (None, None)
        ff = frame(M, N, c.ldc_f32, torch.float32) if c.out_f32 else (None, None)
        if c.mask == "bf16":
            ops.gemm_nt_dmask(a, b, N, K, mask, c.act, c.slope, res_bf16=res, out=fb[1])
        elif c.mask == "f32":
            ops.gemm_nt_dmask_f32(a, b, N, K, mask, c.act, c.slope, res_f32=res, out=ff[1])
        elif c.bias_off:
            # (ops.gemm_nt moves a bias that is not 16-byte aligned; the C entry point takes it as it is)
            dhaug_amd._lib.call("dhaug_gemm_bf16", a.data_ptr(), c.lda, b.data_ptr(), c.ldb, bias.data_ptr(),
                                res.data_ptr() if c.res == "bf16" else None, c.ld_res if c.res == "bf16" else 0,
                                res.data_ptr() if c.res == "f32" else None, c.ld_res if c.res == "f32" else 0,
                                fb[1].data_ptr() if c.out_bf16 else None, c.ldc_bf16, c.bf16_width if c.out_bf16 else 0,
                                ff[1].data_ptr() if c.out_f32 else None, c.ldc_f32 if c.out_f32 else N, M, N, K, c.act, float(c.slope),
                                torch.cuda.current_stream().cuda_stream or None)
        else:
            ops.gemm_nt(a, b, N, K, bias=bias, res_bf16=res if c.res == "bf16" else None, res_f32=res if c.res == "f32" else None,
                        act=c.act, slope=c.slope, n_pad=c.n_pad, c_bf16=fb[1], c_f32=ff[1])
        torch.cuda.synchronize()
        return fb[0], ff[0]

    bufb, buff = launch()
    figures = []
    if c.out_f32:
        assert buff.stride(0) == c.ldc_f32
        got = buff[:M, :N].cpu()
        assert torch.isfinite(got).all(), "something outside a row's own K columns reached the fp32 result"
        err = (got.double() - ref).abs().max().item()
        figures.append("f32 %.3g of %.3g" % (err, delta))
        assert err <= delta, (c.ident, err, delta)
        assert untouched_outside(buff, M, N), "fp32 store outside rows [0, M) x columns [0, N)"
    if c.out_bf16:
        assert bufb.stride(0) == c.ldc_bf16
        got = bufb[:M, :N].cpu()
        assert torch.isfinite(got.float()).all(), "something outside a row's own K columns reached the bf16 result"
        # one round-to-nearest bf16 rounding of a value within delta of the reference
        excess = ((got.double() - ref).abs() - (2.0 ** -8 * (ref.abs() + delta) + delta)).max().item()
        figures.append("bf16 excess %.3g" % excess)
        assert excess <= 0.0, (c.ident, excess, delta)
        assert untouched_outside(bufb, M, c.bf16_width), "bf16 store outside rows [0, M) x columns [0, max(N, n_pad))"
        if c.bf16_width > N:
            assert bool((bufb[:M, N:c.bf16_width] == 0).all()), "pad columns [N, n_pad) must be zero"
    if c.out_f32 and c.out_bf16:
        assert torch.equal(bufb[:M, :N], buff[:M, :N].to(BF16)), "both outputs of one launch: the bf16 one is the rounded fp32 one"
    print(c.ident, ", ".join(figures))
    # no NT kernel uses atomics: one summation order
    bufb2, buff2 = launch()
    if c.out_f32:
        assert torch.equal(buff, buff2)
    if c.out_bf16:
        assert torch.equal(bufb, bufb2)


@pytest.mark.parametrize("c", G.NT_CASES, ids=lambda c: c.ident)
def test_nt_route(ops, monkeypatch, c):
    run_nt(ops, c, monkeypatch)


# ----------------------------------------------------------------------------------------------------------------------- TN
def tn_operand(M, N, gen):
    """(M, ceil8 N) bf16: columns [N, ceil8 N) zero (the kernels fetch 16-byte chunks), everything around the block NaN -- the columns
    beyond ceil8(N), and a row above and below"""
    p = G.ceil_to(N, 8)
    x = torch.zeros(M, p)
    x[:, :N] = torch.randn(M, N, generator=gen)
    x = x.to(BF16)
    return x, hostile(x, p + 16, BF16)


@pytest.mark.parametrize("c", G.TN_CASES, ids=lambda c: c.ident)
def test_tn_route(ops, c):
    M, N1, N2 = c.M, c.N1, c.N2
    gen = torch.Generator().manual_seed(M + 31 * N1 + N2)
    A, a = tn_operand(M, N1, gen)
    B, b = tn_operand(M, N2, gen)
    ref = A[:, :N1].double().t() @ B[:, :N2].double()
    csref = A[:, :N1].double().sum(0)
    csref_rows = A[:c.colsum_rows, :N1].double().sum(0)
    tol = 1e-4 * max(1.0, ref.abs().max().item())                 # fp32 atomics: order-dependent rounding
    cstol = lambda r: 1e-4 * max(1.0, r.abs().max().item()) + 1e-3
    ldc = G.ceil_to(N2, 4) + 16

    def out_frame(fill=None):
        buf, view = frame(N1, N2, ldc, torch.float32)
        if fill is not None:
            view.copy_(fill)
        return buf, view

    def colsum_frame(fill):
        buf = torch.full((N1 + 16,), SENTINEL, device="cuda")
        buf[:N1] = fill
        return buf, buf[:N1]

    def check(buf, want, bound):
        torch.cuda.synchronize()
        err = (buf[:N1, :N2].cpu().double() - want).abs().max().item()
        assert torch.isfinite(buf[:N1, :N2]).all() and err <= bound, (c.ident, err, bound)
        assert untouched_outside(buf, N1, N2), "store outside the output's own rows and columns"
        return err

    def check_cs(buf, want, bound):
        err = (buf[:N1].cpu().double() - want).abs().max().item()
        assert err <= bound, (c.ident, err, bound)
        assert bool((buf[N1:] == SENTINEL).all()), "column sums written beyond N1"
        return err

    # plain: the output's previous content (the sentinel) is overwritten
    buf, view = out_frame()
    ops.gemm_tn(a, b, N1, N2, out=view)
    e0 = check(buf, ref, tol)
    first = buf[:N1, :N2].clone()
    # accumulate: onto the first result
    buf, view = out_frame(first)
    ops.gemm_tn(a, b, N1, N2, out=view, accumulate=True)
    e1 = check(buf, 2 * ref, 2 * tol)
    # column sums of A from the same launch: overwritten without `accumulate` ...
    buf, view = out_frame()
    csbuf, cs = colsum_frame(3.0)
    ops.gemm_tn(a, b, N1, N2, out=view, colsum=cs)
    check(buf, ref, tol)
    e2 = check_cs(csbuf, csref, cstol(csref))
    # ... and added to what is there with it
    buf, view = out_frame(first)
    csbuf, cs = colsum_frame(csbuf[:N1].clone())
    ops.gemm_tn(a, b, N1, N2, out=view, accumulate=True, colsum=cs)
    check(buf, 2 * ref, 2 * tol)
    check_cs(csbuf, 2 * csref, 2 * cstol(csref))
    # the sums over the leading rows only
    buf, view = out_frame()
    csbuf, cs = colsum_frame(3.0)
    ops.gemm_tn(a, b, N1, N2, out=view, colsum=cs, colsum_rows=c.colsum_rows)
    check(buf, ref, tol)
    e3 = check_cs(csbuf, csref_rows, cstol(csref_rows))
    print(c.ident, "product %.3g, accumulated %.3g of %.3g; colsum %.3g, leading rows %.3g of %.3g" % (e0, e1, tol, e2, e3, cstol(csref)))
