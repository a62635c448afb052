"""GPU tests of the SemGCN joint-mix kernels (csrc/dhaug_graph.hip) through ops.graph_mix / ops.graph_adj_grad / ops.graph_wcat,
each against an fp64 einsum on the same STORED inputs (a bf16 operand is compared as the bf16 values it holds), with every output
pre-filled with NaN inside a wider buffer whose other columns must stay NaN.

Bounds.  A result is a sum of at most 16 products and a bias: 17 fmaf / add roundings, each at most 2^-24 of the running sum, which
never exceeds S = sum |A||h| + |bias|; 32 * 2^-24 * S covers them with room for the products' own roundings.  A bf16 output adds one
rounding, 2^-9 |z|, bounded by 2^-8 |ref|.  The adjacency gradient is accumulated in fp64 from exact products (fp32 x fp32 fits
fp64): each partial sum has at most a few hundred terms per lane, so 1e-12 * sum |g||h| is orders above its rounding."""
import os
import sys

import pytest
import torch

import gcn_util as CU

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
BF16, F32 = torch.bfloat16, torch.float32
NAN = float("nan")


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    sys.path.insert(0, ROOT)
    from dhaug_amd import ops as O
    return O


def gen(seed):
    return torch.Generator().manual_seed(seed)


def make_A(seed):
    """asymmetric, rows not normalised, mixed signs: a transposition or a normalisation assumed by the kernel shows"""
    return (torch.randn(16, 16, generator=gen(seed)) * 0.7).cuda()


def one_in(t):
    """the same values as a view that starts one element into a larger buffer (4-byte aligned only)"""
    buf = torch.empty(t.numel() + 5, dtype=t.dtype, device=t.device)
    v = buf[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4
    return v


def rows_in(B, width, dtype, seed, ld=None, offset=0):
    """(16 B, width) random rows as a column block [offset, offset + width) of a (16 B, ld) buffer whose other columns are NaN"""
    ld = width if ld is None else ld
    buf = torch.full((16 * B, ld), NAN, dtype=dtype, device="cuda")
    v = buf[:, offset:offset + width]
    v.copy_(torch.randn(16 * B, width, generator=gen(seed)).to(dtype))
    return v


def out_in(B, width, dtype, extra=8):
    buf = torch.full((16 * B, width + extra), NAN, dtype=dtype, device="cuda")
    return buf, buf[:, :width]


def check_mix(ops, B, C, src_dtype=F32, out_dtype=None, ldh=None, offset=0, bias=True, odd=False, seed=0):
    """forward and adjoint of one shape"""
    out_dtype = src_dtype if out_dtype is None else out_dtype
    A = make_A(seed + 1)
    bv = torch.randn(C, generator=gen(seed + 2)).cuda() if bias else None
    if odd:
        A, bv = one_in(A), (one_in(bv) if bias else None)
    A64 = A.double()
    off = A64 - torch.diag(torch.diagonal(A64))
    pad = lambda w: -(-w // 16) * 16 if out_dtype == BF16 else w
    tol = lambda S, ref: 32 * 2.0 ** -24 * S + (2.0 ** -8 * ref.abs() if out_dtype == BF16 else 0)

    # forward
    H = rows_in(B, 2 * C, src_dtype, seed + 3, ldh, offset)
    h0, h1 = H[:, :C].double().reshape(B, 16, C), H[:, C:2 * C].double().reshape(B, 16, C)
    ref = CU.mix_ref(h0, h1, A64, None if bv is None else bv.double())
    S = CU.mix_ref(h0.abs(), h1.abs(), A64.abs(), None if bv is None else bv.double().abs())
    buf, out = out_in(B, pad(C), out_dtype)
    z = ops.graph_mix(H, A, bv, C, out=out)
    assert z is out and torch.isnan(buf[:, pad(C):]).all(), "columns beyond the output's own were written"
    got = out.double().reshape(B, 16, -1)
    assert not torch.isnan(got).any(), "an element of the output was left unwritten"
    assert ((got[..., :C] - ref).abs() <= tol(S, ref)).all(), ((got[..., :C] - ref).abs().max().item(), "forward", B, C)
    assert (got[..., C:] == 0).all(), "the pad columns of a bf16 output must be exactly zero"
    # the allocating form gives the same bits
    assert torch.equal(ops.graph_mix(H, A, bv, C, out_bf16=out_dtype == BF16), out)

    # adjoint
    G = rows_in(B, C, src_dtype, seed + 4, None if ldh is None else ldh - C, offset)
    g = G.double().reshape(B, 16, C)
    ref0, ref1 = torch.einsum("i,bic->bic", torch.diagonal(A64), g), torch.einsum("ij,bic->bjc", off, g)
    S0, S1 = torch.einsum("i,bic->bic", torch.diagonal(A64).abs(), g.abs()), torch.einsum("ij,bic->bjc", off.abs(), g.abs())
    buf, out = out_in(B, pad(2 * C), out_dtype)
    d = ops.graph_mix(G, A, None, C, transpose=True, out=out)
    assert d is out and torch.isnan(buf[:, pad(2 * C):]).all()
    got = out.double().reshape(B, 16, -1)
    assert not torch.isnan(got).any()
    assert ((got[..., :C] - ref0).abs() <= tol(S0, ref0)).all(), ("adjoint, dh0", B, C)
    assert ((got[..., C:2 * C] - ref1).abs() <= tol(S1, ref1)).all(), ((got[..., C:2 * C] - ref1).abs().max().item(), "adjoint, dh1", B, C)
    assert (got[..., 2 * C:] == 0).all()
    return H, G


def check_adj(ops, H, G, C, pairs=None, seed=0):
    """the adjacency gradient on the operands of a mix case"""
    B = H.shape[0] // 16
    if pairs is None:
        pairs = list(zip(*CU.pattern()))
    pt = torch.tensor(pairs, dtype=torch.int32, device="cuda").reshape(-1, 2)
    g = G.double().reshape(B, 16, C)
    h0, h1 = H[:, :C].double().reshape(B, 16, C), H[:, C:2 * C].double().reshape(B, 16, C)
    full, S = torch.einsum("bic,bjc->ij", g, h1), torch.einsum("bic,bjc->ij", g.abs(), h1.abs())
    diag, Sd = torch.einsum("bic,bic->i", g, h0), torch.einsum("bic,bic->i", g.abs(), h0.abs())
    eye = torch.eye(16, dtype=torch.bool, device="cuda")
    ref, S = torch.where(eye, torch.diag(diag), full), torch.where(eye, torch.diag(Sd), S)
    listed = torch.zeros(16, 16, dtype=torch.bool, device="cuda")
    listed[pt[:, 0].long(), pt[:, 1].long()] = True
    out = torch.full((16, 16), NAN, device="cuda")
    dA = ops.graph_adj_grad(G, H, pt, C, out=out)
    assert dA is out and not torch.isnan(out).any(), "an entry of dA was left as allocated"
    assert (out[~listed] == 0).all(), "entries off the pair list must be exactly zero"
    # the fp32 result is the fp64 sum rounded once: half an ulp of the result on top of the accumulation bound
    err = (out.double() - ref).abs()[listed]
    bound = (1e-12 * S + 2.0 ** -24 * ref.abs())[listed]
    assert (err <= bound).all(), (err.max().item(), B, C, len(pairs))
    again = ops.graph_adj_grad(G, H, pt, C)
    assert torch.equal(again, out), "two calls on the same input differ"


CASES = {
    "B1_C16": dict(B=1, C=16),
    "B1_C3_ld6_elements": dict(B=1, C=3, ldh=6),
    "B5_C20_ld40": dict(B=5, C=20, ldh=40),
    "B5_C18_pitch_off_grid": dict(B=5, C=18),
    "bf16_C32": dict(B=3, C=32, src_dtype=BF16),
    "bf16_C24_pad": dict(B=3, C=24, src_dtype=BF16),
    "bf16_C20_pad_elements": dict(B=2, C=20, src_dtype=BF16),
    "bf16_C128_B40": dict(B=40, C=128, src_dtype=BF16),
    "f32_C128_B40": dict(B=40, C=128),
    "f32_to_bf16_C24": dict(B=2, C=24, src_dtype=F32, out_dtype=BF16),
    "bf16_to_f32_C16": dict(B=2, C=16, src_dtype=BF16, out_dtype=F32),
    "block_of_wider_buffer_aligned": dict(B=3, C=16, ldh=2 * 16 + 24, offset=4),
    "block_of_wider_buffer_odd_base": dict(B=3, C=16, ldh=2 * 16 + 24, offset=1),
    "bf16_block_of_wider_buffer": dict(B=3, C=16, src_dtype=BF16, ldh=2 * 16 + 16, offset=8),
    "bias_and_A_one_element_in": dict(B=2, C=16, odd=True),
    "C3_bias_and_A_one_element_in": dict(B=2, C=3, odd=True),
    "no_bias": dict(B=2, C=8, bias=False),
    # C = 4 in fp32 is one work item per pose: one workgroup plus one item; a second pass of the grid-stride loop plus one item
    "one_block_plus_one_item": dict(B=CU.MIX_BLOCK + 1, C=4),
    "second_pass": dict(B=CU.MIX_BLOCK * CU.MIX_MAX_BLOCKS + 1, C=4),
    "second_pass_bf16": dict(B=CU.MIX_BLOCK * CU.MIX_MAX_BLOCKS // 2 + 1, C=16, src_dtype=BF16),
}


@pytest.mark.parametrize("name", list(CASES))
def test_graph_mix_and_adjacency_gradient(ops, name):
    case = CASES[name]
    if name.startswith("one_block"):
        assert CU.mix_items(case["B"], 4, F32, False) == CU.MIX_BLOCK + 1
    if name == "second_pass":
        assert CU.mix_items(case["B"], 4, F32, False) == CU.MIX_BLOCK * CU.MIX_MAX_BLOCKS + 1
    if name == "second_pass_bf16":
        assert CU.mix_items(case["B"], 16, BF16, True) == CU.MIX_BLOCK * CU.MIX_MAX_BLOCKS + 2
    H, G = check_mix(ops, seed=len(name), **case)
    check_adj(ops, H, G, case["C"])


@pytest.mark.parametrize("B,C,dtype", [(1, 16, F32), (5, 18, F32), (3, 24, BF16), (70, 3, F32)])
def test_adjacency_gradient_pair_lists(ops, B, C, dtype):
    """a list of one pair, of all 256, of the skeleton's pattern in another order, with a repeated and an out-of-range pair; more
    poses than workgroups (B = 70 > ADJ_MAX_BLOCKS: two poses per workgroup, a ragged last one)"""
    H, G = rows_in(B, 2 * C, dtype, 1), rows_in(B, C, dtype, 2)
    check_adj(ops, H, G, C, [(3, 2)])
    check_adj(ops, H, G, C, [(7, 7)])
    check_adj(ops, H, G, C, [(i, j) for i in range(16) for j in range(16)])
    check_adj(ops, H, G, C, list(zip(*CU.pattern()))[::-1] + [(0, 0)])
    # a pair outside the 16 joints names no entry
    pt = torch.tensor([(1, 2), (16, 0), (-1, 3), (2, 1)], dtype=torch.int32, device="cuda")
    out = torch.full((16, 16), NAN, device="cuda")
    ops.graph_adj_grad(G, H, pt, C, out=out)
    want = torch.full((16, 16), NAN, device="cuda")
    ops.graph_adj_grad(G, H, pt[[0, 3]].contiguous(), C, out=want)
    assert torch.equal(out, want) and int((out != 0).sum()) == 2
    # an empty list: all zeros
    ops.graph_adj_grad(G, H, pt[:0].contiguous(), C, out=out.fill_(NAN))
    assert (out == 0).all()


@pytest.mark.parametrize("n_in,n_out", [(2, 128), (128, 128), (128, 3), (5, 7)])
def test_graph_wcat(ops, n_in, n_out):
    """Wcat = [W[0]^T ; W[1]^T] and its adjoint are exact copies; W may start on a 4-byte boundary"""
    W = one_in(torch.randn(2, n_in, n_out, generator=gen(3)).cuda())
    cat = ops.graph_wcat(W, True)
    assert cat.shape == (2 * n_out, n_in) and torch.equal(cat, torch.cat([W[0].t(), W[1].t()], 0))
    back = ops.graph_wcat(cat, False)
    assert back.shape == W.shape and torch.equal(back, W)


def test_wrapper_errors(ops):
    A, H = make_A(0), rows_in(1, 32, F32, 0)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        ops.graph_mix(H.cpu(), A, None, 16)
    with pytest.raises(ValueError, match="16 rows per pose"):
        ops.graph_mix(H[:8], A, None, 16)
    with pytest.raises(ValueError, match=">= 34"):
        ops.graph_mix(H, A, None, 17)
    with pytest.raises(ValueError, match="adjoint takes no bias"):
        ops.graph_mix(H, A, torch.zeros(16, device="cuda"), 16, transpose=True)
    with pytest.raises(ValueError, match="A must be"):
        ops.graph_mix(H, A[:8], None, 16)
    with pytest.raises(ValueError, match="out must be"):
        ops.graph_mix(H, A, None, 16, out=torch.empty(16, 15, device="cuda"))
    with pytest.raises(ValueError, match="pairs must be"):
        ops.graph_adj_grad(H[:, :16], H, torch.zeros(257, 2, dtype=torch.int32, device="cuda"), 16)
    # an empty batch is a no-op
    assert ops.graph_mix(H[:0], A, None, 16).shape == (0, 16)
