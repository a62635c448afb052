"""GPU tests of the BatchNorm + ReLU + dropout kernels (csrc/dhaug_posenet.hip) through the C-ABI, against the fp64 restatement of
tests/posenet_util.py on the same inputs.  Every test prints its figures ("FIGURE ...") before it asserts.

The scales the errors are expressed in (fp32 ulps of):
    y       ((|z| + |mean|) rstd |gamma| + |beta|) / (1 - p) + |residual|
    dz      |gamma| rstd (|gz| + sum|gz| / M + |xhat| sum|gz xhat| / M) -- sums of MAGNITUDES: xhat is an fp32 value with a relative
            rounding error of its own in every term of sum(gz xhat), so the sum's error follows sum|gz xhat| and not the (often
            cancelling) sum itself; with |sum| in the scale the figure grows with M (15 ulp at M = 1 030) without the kernel
            being any less accurate
    dgamma  sum|gz xhat|,  dbeta  sum|gz|
Measured (MI355X, gfx950, 2026-10-17; the largest figure over all the cases below); the constant is that, rounded up, x 2:
    y 2.495 -> Y_ULPS = 5;  dz 2.115 -> DZ_ULPS = 4.4;  dgamma 1.163, dbeta 0.5 -> DPARAM_ULPS = 2.4
    (statistics: mean 0.5, rstd 0.4999, unbiased variance 0.4999 ulp against the derived bound of 2; fold: 0.5001 / 0.4996 / 0.4999)
"""
import math

import pytest
import torch

import posenet_util as NU

pytestmark = pytest.mark.gpu

Y_ULPS = 5.0
DZ_ULPS = 4.4
DPARAM_ULPS = 2.4
STAT_ULPS = 2.0            # derived (the issue): fp64 accumulation of exact products, one final rounding and one subtraction

BF16 = torch.bfloat16
SHAPES = [(2, 16), (3, 48), (40, 64), (96, 64), (1030, 1024), NU.MULTIPASS]
EPS = 1e-5


@pytest.fixture(scope="module")
def D():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import argparse
    from dhaug_amd import _lib, ops
    return argparse.Namespace(_lib=_lib, ops=ops)


def figure(name, value):
    print("FIGURE %s %.4g" % (name, value))


def ceil16(c):
    return (c + 15) // 16 * 16


def p_(t):
    return None if t is None else t.data_ptr()


def bf16_ulp(x):
    a = x.double().abs().clamp_min(2.0 ** -126)
    return torch.exp2(torch.floor(torch.log2(a)) - 7)


def in_nan_buffer(t, ld):
    """t (M, C) placed in a NaN-filled (M, ld) buffer: a read beyond a row's C columns poisons the result"""
    buf = torch.full((t.shape[0], ld), float("nan"), dtype=t.dtype, device=t.device)
    buf[:, :t.shape[1]] = t
    return buf


def make_case(M, C, dtype, seed):
    """z with column means of 10 standard deviations in half of the columns, gamma of both signs, a residual and a cotangent"""
    g = torch.Generator().manual_seed(seed)
    std = torch.rand(C, generator=g) + 0.5
    z = torch.randn(M, C, generator=g) * std
    z[:, ::2] += 10.0 * std[::2]
    gamma = (torch.rand(C, generator=g) + 0.5) * torch.where(torch.rand(C, generator=g) < 0.25, -1.0, 1.0)
    beta = (torch.rand(C, generator=g) * 2 - 1) * 0.25
    res = torch.randn(M, C, generator=g)
    cot = torch.randn(M, C, generator=g)
    dev = lambda t, d=torch.float32: t.to(d).cuda()
    return dict(z=dev(z, dtype), res=dev(res, dtype), cot=dev(cot, dtype), gamma=dev(gamma), beta=dev(beta))


class Runner:
    """the four training entry points on raw pointers"""

    def __init__(self, D, M, C, dtype):
        self.call, self.M, self.C, self.zb = D._lib.call, M, C, int(dtype == BF16)
        self.ws = D.ops.bn_workspace(C, "cuda")
        self.mean = torch.empty(C, device="cuda")
        self.rstd = torch.empty(C, device="cuda")

    def outputs(self, which="both"):
        """7-filled buffers with guard columns that are never written; which: "both", or "bf16" / "f32" alone (the other NULL)"""
        yb = torch.full((self.M, ceil16(self.C) + 16), 7.0, dtype=BF16, device="cuda") if which != "f32" else None
        yf = torch.full((self.M, (self.C + 3) // 4 * 4 + 4), 7.0, device="cuda") if which != "bf16" else None
        return yb, yf

    def forward(self, z, gamma, beta, res=None, given=False, buffers=(None, None, None), momentum=0.1, p=0.0, rng=(0, 0),
                which="both"):
        yb, yf = self.outputs(which)
        ld = lambda t: 0 if t is None else t.stride(0)
        if not given:
            self.call("dhaug_bn_partials", p_(z), self.zb, z.stride(0), self.M, self.C, p_(self.ws), None)
        self.call("dhaug_bn_act_forward", p_(z), self.zb, z.stride(0), p_(res), ld(res), p_(gamma),
                  p_(beta), p_(self.mean), p_(self.rstd), None if given else p_(self.ws), p_(buffers[0]), p_(buffers[1]),
                  p_(buffers[2]), momentum, EPS, p, rng[0], rng[1], p_(yb), ld(yb), p_(yf), ld(yf), self.M, self.C, None)
        return yb, yf

    def backward(self, z, g, gamma, beta, p=0.0, rng=(0, 0), which="both"):
        dzb, dzf = self.outputs(which)
        ld = lambda t: 0 if t is None else t.stride(0)
        dg, db = torch.empty(self.C, device="cuda"), torch.empty(self.C, device="cuda")
        head = (p_(z), self.zb, z.stride(0), p_(g), g.stride(0), p_(gamma), p_(beta), p_(self.mean), p_(self.rstd), p, rng[0], rng[1])
        self.call("dhaug_bn_act_backward_partials", *head, self.M, self.C, p_(self.ws), None)
        self.call("dhaug_bn_act_backward", *head, p_(self.ws), p_(dzb), ld(dzb), p_(dzf), ld(dzf), p_(dg), p_(db),
                  self.M, self.C, None)
        return dzb, dzf, dg, db


def rows_of(t, C):
    """t (M, C) with rows on the 16-byte grid: as it is when C allows, else in a NaN-filled buffer of the next pitch that does"""
    return t.contiguous() if C % 8 == 0 else in_nan_buffer(t, (C + 7) // 8 * 8)


def check_padded(out_b, out_f, M, C):
    """bf16 pad columns are zero; nothing is written beyond ceil16(C) / C"""
    Cp = ceil16(C)
    assert torch.all(out_b[:, C:Cp] == 0)
    assert torch.all(out_b[:, Cp:] == 7.0) and torch.all(out_f[:, C:] == 7.0)


def check_bf16(out_b, ref64, C, name, slack):
    """the bf16 output is the fp64 result rounded to bf16, within one bf16 ulp (slack: the fp32 result's own bound, which decides
    the rounding where the result is far smaller than its terms)"""
    diff = (out_b[:, :C].double() - ref64.to(BF16).double()).abs()
    err = (diff / (bf16_ulp(ref64) + slack)).max().item()
    figure(name, err)
    assert err <= 1.0, (name, err)


@pytest.mark.parametrize("pad", [0, 16])
@pytest.mark.parametrize("dtype", [torch.float32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("M,C", SHAPES)
def test_batch_statistics_forward_and_backward(D, M, C, dtype, pad):
    c = make_case(M, C, dtype, 1000 * M + C)
    z, res, cot = (in_nan_buffer(c[k], C + pad) for k in ("z", "res", "cot"))
    gamma, beta = c["gamma"], c["beta"]
    R = Runner(D, M, C, dtype)
    rm, rv = torch.full((C,), 3.0, device="cuda"), torch.full((C,), 5.0, device="cuda")
    nbt = torch.zeros((), dtype=torch.int64, device="cuda")
    yb, yf = R.forward(z, gamma, beta, res=res, buffers=(rm, rv, nbt), momentum=1.0)
    torch.cuda.synchronize()
    z64, res64, cot64 = (c[k].double().cpu() for k in ("z", "res", "cot"))
    g64, b64 = gamma.double().cpu(), beta.double().cpu()
    mean64, var64 = NU.bn_stats_ref(z64)
    rstd64 = 1.0 / torch.sqrt(var64 + EPS)

    # statistics: mean, rstd, and (momentum 1: running = the batch's) the unbiased variance
    e_mean = ((R.mean.double().cpu() - mean64).abs() / NU.ulp32(mean64)).max().item()
    e_rstd = ((R.rstd.double().cpu() - rstd64).abs() / NU.ulp32(rstd64)).max().item()
    unb64 = var64 * M / (M - 1)
    e_var = ((rv.double().cpu() - unb64).abs() / NU.ulp32(unb64)).max().item()
    figure("mean_ulp", e_mean), figure("rstd_ulp", e_rstd), figure("var_ulp", e_var)
    assert e_mean <= STAT_ULPS and e_rstd <= STAT_ULPS and e_var <= STAT_ULPS
    assert torch.equal(rm, R.mean) and int(nbt) == 1

    # y against fp64 with the fp64 statistics
    y64, _ = NU.bn_act_ref(z64, mean64, rstd64, g64, b64, residual=res64)
    mag = (z64.abs() + mean64.abs()) * rstd64 * g64.abs() + b64.abs() + res64.abs()
    e_y = ((yf[:, :C].double().cpu() - y64).abs() / NU.ulp32(mag)).max().item()
    figure("y_ulp", e_y)
    assert e_y <= Y_ULPS
    check_padded(yb, yf, M, C)
    check_bf16(yb.cpu(), y64, C, "y_bf16_ulp", Y_ULPS * NU.ulp32(mag))

    # backward with the kernel's own statistics; the active set is read back from a forward pass without the residual
    _, branch = R.forward(z, gamma, beta, given=True)
    active = branch[:, :C].cpu() > 0
    dzb, dzf, dg, db = R.backward(z, cot, gamma, beta)
    torch.cuda.synchronize()
    mean_k, rstd_k = R.mean.double().cpu(), R.rstd.double().cpu()
    dz64, dg64, db64, gz64 = NU.bn_act_backward_ref(z64, cot64, mean_k, rstd_k, g64, b64, active=active)
    xh = (z64 - mean_k) * rstd_k
    s1, s2 = gz64.abs().sum(0), (gz64 * xh).abs().sum(0)        # (see the module docstring: sums of magnitudes)
    mag_dz = g64.abs() * rstd_k * (gz64.abs() + s1 / M + xh.abs() * s2 / M)
    e_dz = ((dzf[:, :C].double().cpu() - dz64).abs() / NU.ulp32(mag_dz.clamp_min(1e-30))).max().item()
    e_dg = ((dg.double().cpu() - dg64).abs() / NU.ulp32((gz64 * xh).abs().sum(0).clamp_min(1e-30))).max().item()
    e_db = ((db.double().cpu() - db64).abs() / NU.ulp32(gz64.abs().sum(0).clamp_min(1e-30))).max().item()
    figure("dz_ulp", e_dz), figure("dgamma_ulp", e_dg), figure("dbeta_ulp", e_db)
    assert e_dz <= DZ_ULPS and e_dg <= DPARAM_ULPS and e_db <= DPARAM_ULPS
    check_padded(dzb, dzf, M, C)
    check_bf16(dzb.cpu(), dz64, C, "dz_bf16_ulp", DZ_ULPS * NU.ulp32(mag_dz.clamp_min(1e-30)))


@pytest.mark.parametrize("dtype", [torch.float32, BF16], ids=["f32", "bf16"])
def test_given_statistics_forward(D, dtype):
    """given mean / rstd: y against fp64 with those statistics; no buffer is touched, mean / rstd are not written"""
    M, C = 40, 64
    c = make_case(M, C, dtype, 77)
    R = Runner(D, M, C, dtype)
    g = torch.Generator().manual_seed(5)
    R.mean.copy_(torch.randn(C, generator=g))
    R.rstd.copy_(torch.rand(C, generator=g) + 0.5)
    mean0, rstd0 = R.mean.clone(), R.rstd.clone()
    yb, yf = R.forward(c["z"], c["gamma"], c["beta"], res=c["res"], given=True)
    torch.cuda.synchronize()
    z64, res64, g64, b64 = (c[k].double().cpu() for k in ("z", "res", "gamma", "beta"))
    y64, _ = NU.bn_act_ref(z64, mean0.cpu(), rstd0.cpu(), g64, b64, residual=res64)
    mag = (z64.abs() + mean0.double().cpu().abs()) * rstd0.double().cpu() * g64.abs() + b64.abs() + res64.abs()
    e_y = ((yf[:, :C].double().cpu() - y64).abs() / NU.ulp32(mag)).max().item()
    figure("y_given_ulp", e_y)
    assert e_y <= Y_ULPS
    assert torch.equal(R.mean, mean0) and torch.equal(R.rstd, rstd0)
    check_bf16(yb.cpu(), y64, C, "y_given_bf16_ulp", Y_ULPS * NU.ulp32(mag))


@pytest.mark.parametrize("momentum", [0.1, 0.01])
def test_running_buffers_follow_batchnorm1d(D, momentum):
    """three calls against nn.BatchNorm1d on the same device.  Bound: torch's own batch statistics are fp32 reductions over M rows
    (error up to M * 2^-24 of the statistic's scale, var + mean^2), ours are within 2 ulp; each of the three updates adds three
    roundings to either side: M * 2^-24 * max(var + mean^2) + 12 ulp of the buffer."""
    M, C = 96, 64
    bn = torch.nn.BatchNorm1d(C, momentum=momentum).cuda().train()
    R = Runner(D, M, C, torch.float32)
    rm, rv = torch.zeros(C, device="cuda"), torch.ones(C, device="cuda")
    nbt = torch.zeros((), dtype=torch.int64, device="cuda")
    g = torch.Generator().manual_seed(9)
    scale = 0.0
    for k in range(3):
        z = (torch.randn(M, C, generator=g) * (k + 1) + 0.5 * k).cuda()
        bn(z)
        R.forward(z, bn.weight.detach(), bn.bias.detach(), buffers=(rm, rv, nbt), momentum=momentum)
        scale = max(scale, (z.var(0) + z.mean(0) ** 2).max().item())
    torch.cuda.synchronize()
    assert int(nbt) == 3 == int(bn.num_batches_tracked)
    for ours, theirs, name in ((rm, bn.running_mean, "running_mean"), (rv, bn.running_var, "running_var")):
        err = (ours.double() - theirs.double()).abs()
        bound = M * 2.0 ** -24 * scale + 12 * NU.ulp32(theirs.double())
        figure(name + "_err_over_bound", (err / bound).max().item())
        assert torch.all(err <= bound), name


def keep_of(y):
    return y != 0


DROP_CASES = [(torch.float32, 1024), (BF16, 1024), (torch.float32, 50), (BF16, 50)]
DROP_IDS = ["f32-1024", "bf16-1024", "f32-50", "bf16-50"]


@pytest.mark.parametrize("dtype,C", DROP_CASES, ids=DROP_IDS)
def test_dropout(D, dtype, C):
    """p = 0.25 at 1 024 rows: binomial bounds on the keep fractions (sigma = sqrt(p (1 - p) / n)), kept elements are the p = 0
    output x 4/3, (seed, offset) reproduce the mask, another offset gives an independent one, the backward pass regenerates it.
    fp32 and bf16 inputs (four and eight elements, one and two Philox calls, per lane) at C = 1 024, and at C = 50, where rows do
    not hold whole groups of four elements and every element's word is looked up on its own."""
    M = 1024
    p, seed, off = 0.25, 1234567, 40
    g = torch.Generator().manual_seed(3)
    z = rows_of(torch.randn(M, C, generator=g).to(dtype).cuda(), C)
    gamma, beta = torch.ones(C, device="cuda"), torch.full((C,), 8.0, device="cuda")   # pre-activations xhat + 8 > 0: y != 0 <=> kept
    R = Runner(D, M, C, dtype)
    _, y0 = R.forward(z, gamma, beta)                                  # p = 0, no seed
    _, y0s = R.forward(z, gamma, beta, p=0.0, rng=(seed, off))
    assert torch.equal(y0, y0s), "p = 0 must not depend on the seed"
    assert torch.all(y0[:, :C] > 0)
    _, y1 = R.forward(z, gamma, beta, p=p, rng=(seed, off), given=True)
    _, y1b = R.forward(z, gamma, beta, p=p, rng=(seed, off), given=True)
    _, y2 = R.forward(z, gamma, beta, p=p, rng=(seed, off + 4), given=True)
    assert torch.equal(y1, y1b), "the same (seed, offset) must reproduce the output bit for bit"
    k1, k2 = keep_of(y1[:, :C]), keep_of(y2[:, :C])
    sig = math.sqrt(p * (1 - p))
    total = k1.double().mean().item()
    figure("keep_total", total)
    assert abs(total - 0.75) <= 5 * sig / math.sqrt(M * C)              # 5 sigma (2.1e-3 at C = 1 024)
    cols, rows = k1.double().mean(0), k1.double().mean(1)
    figure("keep_col_dev", (cols - 0.75).abs().max().item()), figure("keep_row_dev", (rows - 0.75).abs().max().item())
    assert (cols - 0.75).abs().max().item() <= 6 * sig / math.sqrt(M)   # 6 sigma = 0.081
    assert (rows - 0.75).abs().max().item() <= 6 * sig / math.sqrt(C)   # 0.081 at C = 1 024, 0.37 at C = 50
    agree = (k1 == k2).double().mean().item()
    figure("keep_agreement", agree)
    assert abs(agree - 0.625) <= 5 * math.sqrt(0.625 * 0.375 / (M * C))  # independent masks agree with 0.75^2 + 0.25^2; 5 sigma
    want = y0[:, :C].double() * (4.0 / 3.0)
    err = ((y1[:, :C].double() - want).abs() / NU.ulp32(want))[k1].max().item()
    figure("kept_scale_ulp", err)
    assert err <= 1.0
    # the mask is a function of (row * C + column) alone: the bf16 and the fp32 instantiation draw the same one
    other = torch.float32 if dtype == BF16 else BF16
    _, yo = Runner(D, M, C, other).forward(rows_of(z[:, :C].to(other), C), gamma, beta, p=p, rng=(seed, off))
    assert torch.equal(keep_of(yo[:, :C]), k1)

    # backward with the same (seed, offset): the fp64 restatement fed the mask read back from the forward output
    cot = rows_of(torch.randn(M, C, generator=g).to(dtype).cuda(), C)
    _, dzf, dg, db = R.backward(z, cot, gamma, beta, p=p, rng=(seed, off))
    torch.cuda.synchronize()
    mean_k, rstd_k = R.mean.double().cpu(), R.rstd.double().cpu()
    z64, cot64, g64, b64 = z[:, :C].double().cpu(), cot[:, :C].double().cpu(), gamma.double().cpu(), beta.double().cpu()
    dz64, dg64, db64, gz64 = NU.bn_act_backward_ref(z64, cot64, mean_k, rstd_k, g64, b64, keep=k1.cpu(), inv_keep=4.0 / 3.0,
                                                    active=torch.ones(M, C, dtype=torch.bool))
    xh = (z64 - mean_k) * rstd_k
    mag_dz = g64.abs() * rstd_k * (gz64.abs() + gz64.abs().sum(0) / M + xh.abs() * (gz64 * xh).abs().sum(0) / M)
    e_dz = ((dzf[:, :C].double().cpu() - dz64).abs() / NU.ulp32(mag_dz)).max().item()
    e_dg = ((dg.double().cpu() - dg64).abs() / NU.ulp32((gz64 * xh).abs().sum(0))).max().item()
    e_db = ((db.double().cpu() - db64).abs() / NU.ulp32(gz64.abs().sum(0))).max().item()
    figure("drop_dz_ulp", e_dz), figure("drop_dgamma_ulp", e_dg), figure("drop_dbeta_ulp", e_db)
    assert e_dz <= DZ_ULPS and e_dg <= DPARAM_ULPS and e_db <= DPARAM_ULPS


@pytest.mark.parametrize("dtype,C", DROP_CASES, ids=DROP_IDS)
@pytest.mark.parametrize("p", [0.0, 0.25])
def test_zero_output_means_zero_gz(D, p, dtype, C):
    """a cotangent that is non-zero only where the forward branch output is zero gives gz = 0 everywhere, exactly: dbeta, dgamma
    and dz are zeros.  A third of the pre-activations here are ROUNDING RESIDUALS: every column takes three values, and beta is
    minus the rounded product xhat * gamma of the first, so fma(xhat, gamma, beta) is what that rounding lost -- positive, negative
    or zero from column to column.  A backward pass that formed the pre-activation by any other sequence of roundings than the
    forward pass (a separate multiply and add gives exactly 0 there) would let cotangent through, or hold some back."""
    M = 1030
    g = torch.Generator().manual_seed(21)
    R = Runner(D, M, C, dtype)
    R.mean.copy_(torch.randn(C, generator=g))
    R.rstd.copy_(torch.rand(C, generator=g) + 0.5)
    gamma = (torch.rand(C, generator=g) + 0.5).cuda()
    vals = torch.stack([torch.randn(C, generator=g), torch.full((C,), 30.0), torch.full((C,), -30.0)]).to(dtype).cuda()   # residual, > 0, < 0
    pick = torch.randint(0, 3, (M, C), generator=g).cuda()
    z = rows_of(torch.gather(vals, 0, pick), C)
    beta = -(((vals[0].float() - R.mean) * R.rstd) * gamma)
    rng = (99, 8)
    _, y = R.forward(z, gamma, beta, p=p, rng=rng, given=True)
    zero = y[:, :C] == 0
    tiny = (pick == 0) & ~zero
    figure("residual_preactivations_positive", tiny.double().sum().item() / (pick == 0).double().sum().item())
    assert 0.1 < tiny.double().sum().item() / (pick == 0).double().sum().item() < 0.9 * (1 - p) + 0.05
    cot = rows_of(torch.where(zero, torch.randn(M, C, generator=g).cuda() + 2.0, torch.zeros((), device="cuda")).to(dtype), C)
    _, dzf, dg, db = R.backward(z, cot, gamma, beta, p=p, rng=rng)
    torch.cuda.synchronize()
    assert torch.all(db == 0) and torch.all(dg == 0) and torch.all(dzf[:, :C] == 0)
    # and the complement passes through whole: dbeta = the number of non-zero outputs / (1 - p)
    cot2 = rows_of(torch.where(zero, torch.zeros((), device="cuda"), torch.ones((), device="cuda")).to(dtype), C)
    _, _, _, db2 = R.backward(z, cot2, gamma, beta, p=p, rng=rng)
    want = (~zero).double().sum(0) * float(torch.tensor(1.0, dtype=torch.float32) / torch.tensor(1.0 - p, dtype=torch.float32))
    assert ((db2.double() - want).abs() <= NU.ulp32(want.clamp_min(1.0))).all()


@pytest.mark.parametrize("dtype,C", [(torch.float32, 48), (BF16, 48), (torch.float32, 50), (BF16, 1024)],
                         ids=["f32-48", "bf16-48", "f32-50", "bf16-1024"])
def test_single_output_calls(D, dtype, C):
    """what the module issues: exactly one of the two outputs, the other pointer NULL -- the same bits as a call that asks for both,
    forward (batch statistics, residual, dropout) and backward"""
    M, p, rng = 70, 0.25, (7, 12)
    c = make_case(M, C, dtype, 5 * C)
    z, res, cot = (rows_of(c[k], C) for k in ("z", "res", "cot"))
    R = Runner(D, M, C, dtype)
    yb, yf = R.forward(z, c["gamma"], c["beta"], res=res, p=p, rng=rng)
    dzb, dzf, dg, db = R.backward(z, cot, c["gamma"], c["beta"], p=p, rng=rng)
    for which in ("bf16", "f32"):
        y1b, y1f = R.forward(z, c["gamma"], c["beta"], res=res, p=p, rng=rng, which=which)
        d1b, d1f, dg1, db1 = R.backward(z, cot, c["gamma"], c["beta"], p=p, rng=rng, which=which)
        if which == "bf16":
            assert y1f is None and d1f is None and torch.equal(y1b, yb) and torch.equal(d1b, dzb)
        else:
            assert y1b is None and d1b is None and torch.equal(y1f, yf) and torch.equal(d1f, dzf)
        assert torch.equal(dg1, dg) and torch.equal(db1, db)
    assert not torch.isnan(yf[:, :C]).any() and not torch.isnan(dzf[:, :C]).any() and (yf[:, :C] != 0).any()


@pytest.mark.parametrize("N,K", [(64, 32), (48, 40), (1024, 1024)])
def test_fold(D, N, K):
    """W' within 1 ulp of |W'|, b' within 2 ulp of |beta| + |mean gamma rstd|, rstd within 1 ulp, against fp64"""
    g = torch.Generator().manual_seed(N + K)
    W = torch.randn(N, K, generator=g).cuda()
    gamma = ((torch.rand(N, generator=g) + 0.5) * torch.where(torch.rand(N, generator=g) < 0.3, -1.0, 1.0)).cuda()
    beta = (torch.rand(N, generator=g) - 0.5).cuda()
    rm = torch.randn(N, generator=g).cuda()
    rv = (torch.rand(N, generator=g) * 4 + 1e-3).cuda()
    Wo, bo, ro = D.ops.bn_fold(W, gamma, beta, rm, rv, EPS)
    torch.cuda.synchronize()
    rs = 1.0 / torch.sqrt(rv.double() + EPS)
    W64 = (gamma.double() * rs)[:, None] * W.double()
    b64 = beta.double() - rm.double() * gamma.double() * rs
    e_w = ((Wo.double() - W64).abs() / NU.ulp32(W64)).max().item()
    e_b = ((bo.double() - b64).abs() / NU.ulp32(beta.double().abs() + (rm.double() * gamma.double() * rs).abs())).max().item()
    e_r = ((ro.double() - rs).abs() / NU.ulp32(rs)).max().item()
    figure("fold_w_ulp", e_w), figure("fold_b_ulp", e_b), figure("fold_rstd_ulp", e_r)
    assert e_w <= 1.0 and e_b <= 2.0 and e_r <= 1.0
    _, b2, r2 = D.ops.bn_fold(None, gamma, beta, rm, rv, EPS, want_weight=False)
    assert torch.equal(b2, bo) and torch.equal(r2, ro)
