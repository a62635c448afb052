"""GPU tests of the entry points a replayable posenet step needs, through the C-ABI: the device-stream BatchNorm launches
(dhaug_bn_act_forward_dr, dhaug_bn_act_backward_partials_dr, dhaug_bn_act_backward_dr), dhaug_u64_add and dhaug_adam_clip_step_lr.

The yardstick is the existing entry point, not fp64: a new entry is the same kernel instantiated a second time, so for equal
(seed, offset) / equal lr it must give the SAME BITS.  Every comparison first runs the existing entry twice: where it repeats its own
bits (it has no atomics, so it should -- the test prints the spread it finds), bit equality is required of the new entry; if it ever
did not, the new entry would be held to the existing entry's own call-to-call spread of that output instead (same())."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
EPS = 1e-5
SEED = 0x9E3779B97F4A7C15            # a seed with both words in use (passed as uint64; stored in the cell as the same bits)


@pytest.fixture(scope="module")
def D():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import argparse
    from dhaug_amd import _lib, ops
    return argparse.Namespace(_lib=_lib, ops=ops, call=_lib.call)


def p_(t):
    return None if t is None else t.data_ptr()


def ceil_to(v, m):
    return (v + m - 1) // m * m


def i64(v):
    """the int64 with the bits of the uint64 v"""
    v &= (1 << 64) - 1
    return v - (1 << 64) if v >= (1 << 63) else v


def bits(t):
    return t.contiguous().view({4: torch.int32, 2: torch.int16, 8: torch.int64}[t.element_size()])


def same(name, new, old1, old2):
    """new against old1 within the existing entry's own call-to-call spread |old1 - old2| (0: bit equality)"""
    if torch.equal(bits(old1), bits(old2)):
        print("FIGURE %s existing entry repeats its bits" % name)
        assert torch.equal(bits(new), bits(old1)), name
        return
    spread = (old1.double() - old2.double()).abs().max().item()
    print("FIGURE %s existing entry does NOT repeat its bits: spread %.3e" % (name, spread))
    assert (new.double() - old1.double()).abs().max().item() <= spread, name


def rows(t, ld, dtype):
    """(M, C) values in a NaN-filled (M, ld) buffer: a read beyond a row's C columns poisons the result"""
    buf = torch.full((t.shape[0], ld), float("nan"), dtype=dtype, device="cuda")
    buf[:, :t.shape[1]] = t.to(dtype).cuda()
    return buf


class Layer:
    """one BatchNorm layer's forward and backward through either family of entry points; rng = ("imm", seed, offset) or
    ("cell", cell tensor, delta)"""

    def __init__(self, D, M, C, dtype, seed):
        self.D, self.M, self.C, self.zb = D, M, C, int(dtype == BF16)
        g = torch.Generator().manual_seed(seed)
        ld = ceil_to(C, 8) + 8
        self.z = rows(torch.randn(M, C, generator=g) * 2 + 0.5, ld, dtype)
        self.res = rows(torch.randn(M, C, generator=g), ld, dtype)
        self.cot = rows(torch.randn(M, C, generator=g), ld, dtype)
        self.gamma = (torch.rand(C, generator=g) + 0.5).cuda()
        self.beta = ((torch.rand(C, generator=g) * 2 - 1) * 0.25).cuda()
        self.ws = D.ops.bn_workspace(C, "cuda")

    def run(self, rng, p, residual):
        M, C, call = self.M, self.C, self.D.call
        dr = "_dr" if rng[0] == "cell" else ""
        a0, a1 = (p_(rng[1]), rng[2]) if dr else (rng[1], rng[2])
        out = dict(mean=torch.empty(C, device="cuda"), rstd=torch.empty(C, device="cuda"),
                   running_mean=torch.full((C,), 3.0, device="cuda"), running_var=torch.full((C,), 5.0, device="cuda"),
                   nbt=torch.full((1,), 41, dtype=torch.int64, device="cuda"))
        for k in ("yb", "dzb"):
            out[k] = torch.full((M, ceil_to(C, 16) + 16), 7.0, dtype=BF16, device="cuda")
        for k in ("yf", "dzf"):
            out[k] = torch.full((M, ceil_to(C, 4) + 4), 7.0, device="cuda")
        out["dgamma"], out["dbeta"] = torch.empty(C, device="cuda"), torch.empty(C, device="cuda")
        res = self.res if residual else None
        call("dhaug_bn_partials", p_(self.z), self.zb, self.z.stride(0), M, C, p_(self.ws), None)
        call("dhaug_bn_act_forward" + dr, p_(self.z), self.zb, self.z.stride(0), p_(res), 0 if res is None else res.stride(0),
             p_(self.gamma), p_(self.beta), p_(out["mean"]), p_(out["rstd"]), p_(self.ws), p_(out["running_mean"]),
             p_(out["running_var"]), p_(out["nbt"]), 0.1, EPS, p, a0, a1, p_(out["yb"]), out["yb"].stride(0), p_(out["yf"]),
             out["yf"].stride(0), M, C, None)
        head = (p_(self.z), self.zb, self.z.stride(0), p_(self.cot), self.cot.stride(0), p_(self.gamma), p_(self.beta), p_(out["mean"]),
                p_(out["rstd"]), p, a0, a1)
        call("dhaug_bn_act_backward_partials" + dr, *head, M, C, p_(self.ws), None)
        call("dhaug_bn_act_backward" + dr, *head, p_(self.ws), p_(out["dzb"]), out["dzb"].stride(0), p_(out["dzf"]),
             out["dzf"].stride(0), p_(out["dgamma"]), p_(out["dbeta"]), M, C, None)
        torch.cuda.synchronize()
        return out


def compare_family(L, seed, base, delta, p, residual, tag):
    cell = torch.tensor([i64(seed), i64(base)], dtype=torch.int64, device="cuda")
    imm = ("imm", seed, (base + delta) & ((1 << 64) - 1))
    old1, old2 = L.run(imm, p, residual), L.run(imm, p, residual)
    new = L.run(("cell", cell, delta), p, residual)
    assert cell.tolist() == [i64(seed), i64(base)]                  # the launches read the cell, they do not move it
    for k in ("yb", "yf", "mean", "rstd", "running_mean", "running_var", "nbt", "dzb", "dzf", "dgamma", "dbeta"):
        same("%s %s" % (tag, k), new[k], old1[k], old2[k])
    assert int(new["nbt"].item()) == 42
    assert torch.all(new["yf"][:, L.C:] == 7.0) and torch.all(new["yb"][:, ceil_to(L.C, 16):] == 7.0)     # nothing beyond the rows
    return old1, new


# M: one row pass (2), several (33: two passes of 32 rows) and more rows than the 32-chunk cap covers in one pass each
# (1 100 > 32 x 32); C: one column strip (1, 31 for both types; 33 for bf16) and a ragged second strip (33, 65 for fp32; 65 for bf16)
@pytest.mark.parametrize("dtype", [torch.float32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("C", [1, 31, 33, 65])
@pytest.mark.parametrize("M", [2, 33, 1100])
def test_dr_kernels_give_the_existing_kernels_bits(D, M, C, dtype):
    L = Layer(D, M, C, dtype, 100 * M + C)
    got = {}
    for residual in (False, True):
        for p in (0.0, 0.25):
            got[residual, p] = compare_family(L, SEED, 1000, 8, p, residual,
                                              "M%d C%d %s res%d p%g" % (M, C, str(dtype)[6:], residual, p))[1]
    # the mask is there at all: without a residual, dropout zeroes about a quarter of the outputs on top of the ReLU's
    if M * C >= 1000:
        zeros = {p: (got[False, p]["yf"][:, :C] == 0).double().mean().item() for p in (0.0, 0.25)}
        assert zeros[0.25] > zeros[0.0] + 0.05, zeros


def test_dr_offset_is_a_full_64_bit_sum(D):
    """base = 2^32 - 2 and delta = 4: the sum carries into the high word.  A sum truncated to 32 bits would be offset 2, whose mask
    the existing entry shows to be another one"""
    M, C = 33, 65
    L = Layer(D, M, C, torch.float32, 5)
    base, delta = (1 << 32) - 2, 4
    old, new = compare_family(L, SEED, base, delta, 0.25, True, "carry")
    truncated = L.run(("imm", SEED, (base + delta) & 0xFFFFFFFF), 0.25, True)
    assert not torch.equal(truncated["yf"], old["yf"]) and not torch.equal(truncated["dzf"], old["dzf"])
    # and p = 0 reads no cell: NULL is accepted and the result is the existing entry's
    none = L.run(("cell", None, 0), 0.0, False)
    ref = L.run(("imm", 0, 0), 0.0, False)
    for k in ("yf", "yb", "dzf", "dgamma", "running_var"):
        assert torch.equal(bits(none[k]), bits(ref[k])), k


def test_u64_add_carries_and_accumulates(D):
    cell = torch.tensor([i64(SEED), (1 << 32) - 3, 77], dtype=torch.int64, device="cuda")
    D.ops.u64_add(cell[1:2], 5)
    torch.cuda.synchronize()
    assert cell.tolist() == [i64(SEED), (1 << 32) + 2, 77]            # carried across 2^32; the neighbours are untouched
    D.ops.u64_add(cell[1:2], 12)
    D.ops.u64_add(cell[1:2], (1 << 40) + 1)
    torch.cuda.synchronize()
    assert cell.tolist() == [i64(SEED), (1 << 32) + 2 + 12 + (1 << 40) + 1, 77]
    low = torch.tensor([0xFFFFFFFF], dtype=torch.int64, device="cuda")
    assert D._lib.lib().dhaug_u64_add(ctypes.c_void_p(low.data_ptr()), 1, None) == 0
    torch.cuda.synchronize()
    assert low.item() == 1 << 32


def adam_state(n, seed, off):
    """(param, grad, exp_avg, exp_avg_sq); off = 1: the gradient starts 4 bytes off the 16-byte grid"""
    g = torch.Generator().manual_seed(seed)
    p = torch.randn(n, generator=g).cuda()
    gbuf = torch.randn(n + off, generator=g).cuda()
    grad = gbuf[off:]
    assert grad.data_ptr() % 16 == 4 * off
    m = (torch.randn(n, generator=g) * 0.01).cuda()
    v = (torch.rand(n, generator=g) * 1e-4).cuda()
    return p, grad, m, v


def adam_run(D, state, lr, max_norm, steps, lr_dev):
    p, g, m, v = (t.clone() if k != 1 else t for k, t in enumerate(state))
    n = p.numel()
    ws = D.ops.posetrain_workspace()
    step = torch.zeros(1, dtype=torch.int32, device="cuda")
    norm = torch.full((1,), float("nan"), device="cuda")
    cell = torch.full((1,), lr, dtype=torch.float32, device="cuda")
    for _ in range(steps):
        D.call("dhaug_grad_sumsq", p_(g), n, 0.5, p_(ws), p_(step), None)
        if lr_dev:
            D.call("dhaug_adam_clip_step_lr", p_(p), p_(g), p_(m), p_(v), n, p_(cell), 0.9, 0.999, 1e-8, p_(step), 0.5, max_norm, p_(ws),
                   p_(norm), None)
        else:
            D.call("dhaug_adam_clip_step", p_(p), p_(g), p_(m), p_(v), n, lr, 0.9, 0.999, 1e-8, p_(step), 0.5, max_norm, p_(ws),
                   p_(norm), None)
    torch.cuda.synchronize()
    assert int(step.item()) == steps
    return dict(param=p, exp_avg=m, exp_avg_sq=v, norm=norm)


@pytest.mark.parametrize("clip", [False, True], ids=["unclipped", "clipped"])
@pytest.mark.parametrize("off", [0, 1], ids=["aligned", "grad+4B"])
@pytest.mark.parametrize("n", [1, 5, 4099])
def test_adam_lr_from_the_device_gives_the_existing_bits(D, n, off, clip):
    state = adam_state(n, 7 * n + off, off)
    gnorm = (state[1] * 0.5).norm().item()
    max_norm = gnorm * (0.25 if clip else 4.0)                     # coef 0.25, or nothing to clip
    old1, old2 = (adam_run(D, state, 1e-3, max_norm, 2, False) for _ in range(2))
    new = adam_run(D, state, 1e-3, max_norm, 2, True)
    for k in ("param", "exp_avg", "exp_avg_sq", "norm"):
        same("adam n%d off%d clip%d %s" % (n, off, clip, k), new[k], old1[k], old2[k])
    assert not torch.equal(new["param"], state[0])
    assert abs(new["norm"].item() / gnorm - 1) < 1e-5


@pytest.mark.parametrize("clip", [False, True], ids=["unclipped", "clipped"])
def test_adam_with_a_zero_lr_moves_the_moments_only(D, clip):
    state = adam_state(4099, 3, 0)
    max_norm = (state[1] * 0.5).norm().item() * (0.25 if clip else 4.0)
    new = adam_run(D, state, 0.0, max_norm, 2, True)
    assert torch.equal(bits(new["param"]), bits(state[0]))
    assert not torch.equal(new["exp_avg"], state[2]) and not torch.equal(new["exp_avg_sq"], state[3])
    ref = adam_run(D, state, 0.0, max_norm, 2, False)
    for k in ("param", "exp_avg", "exp_avg_sq"):
        assert torch.equal(bits(new[k]), bits(ref[k])), k
