"""GPU tests of the tap-layout kernels (csrc/dhaug_taps.hip): dhaug_conv_taps_pack_bf16, dhaug_conv_taps_permute_f32 and
dhaug_tap_gather.  All three move data, so every comparison is bit for bit, against torch indexing plus the existing
ops.cast_pad_bf16 / ops.cast_transpose_bf16.  Outputs are pre-filled with NaN and carry eight or sixteen columns beyond the
minimum: an unwritten element fails, and so does a written column that is not the operand's own (the zeroed pad of `nn` is its own).

    entry point                     tests
    dhaug_conv_taps_pack_bf16       test_pack_matches_cast_of_the_permuted_matrix (46 shapes: ragged N, N beyond one tile, k = 1, 3, 5)
    dhaug_conv_taps_permute_f32     test_permute_both_directions, test_permute_sizes_follow_the_kernel_constants
    dhaug_tap_gather                test_gather_windows, test_gather_many_rows_loops_over_the_capped_grid
The argument errors of the three are in tests/test_multiframe_cpu.py (they come back before any launch, so they need no GPU)."""
import os
import sys

import pytest
import torch

import multiframe_util as MU

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    sys.path.insert(0, ROOT)
    from dhaug_amd import ops
    return ops


def bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF16 else torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a), bits(b))


def nan_buffer(rows, cols, dtype):
    return torch.full((rows, cols), float("nan"), dtype=dtype, device="cuda")


def weight(N, Cin, k, seed):
    g = torch.Generator().manual_seed(seed)
    W = torch.randn(N, Cin, k, generator=g)
    flat = W.view(-1)
    # rounding ties of the bf16 cast (round to nearest even, both directions), a negative zero and a value below bf16's normal range
    special = torch.tensor([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, -0.0, 1e-40, -(1.0 + 2.0 ** -8)])
    n = min(flat.numel(), special.numel())
    flat[:n] = special[:n]
    return W.cuda()


PACK_N, PACK_CIN = (1, 15, 16, 48, 1024), (16, 32, 64)


@pytest.mark.parametrize("k", [1, 3, 5])
def test_pack_matches_cast_of_the_permuted_matrix(ops, k):
    shapes = [(N, Cin, k) for N in PACK_N for Cin in PACK_CIN] + ([(1024, 1024, 3)] if k == 3 else [])
    for N, Cin, _ in shapes:
        W = weight(N, Cin, k, 100 * N + Cin + k)
        W2d = W.permute(0, 2, 1).reshape(N, k * Cin).contiguous()
        want_nt, want_nn = ops.cast_pad_bf16(W2d, k * Cin), ops.cast_transpose_bf16(W2d)
        Np = (N + 15) // 16 * 16
        assert want_nn.shape == (k * Cin, Np) and bool((want_nn[:, N:] == 0).all())
        # into wider buffers: the columns beyond the operands stay as they were
        nt_buf, nn_buf = nan_buffer(N, k * Cin + 8, BF16), nan_buffer(k * Cin, Np + 16, BF16)
        nt, nn = ops.conv_taps_pack_bf16(W, nt=nt_buf[:, :k * Cin], nn=nn_buf[:, :Np])
        assert same_bits(nt, want_nt), (N, Cin, k)
        assert same_bits(nn, want_nn), (N, Cin, k)
        assert bool(nt_buf[:, k * Cin:].isnan().all()) and bool(nn_buf[:, Np:].isnan().all()), (N, Cin, k)
        # allocated by the wrapper; and without the transposed operand
        nt2, nn2 = ops.conv_taps_pack_bf16(W)
        assert same_bits(nt2, want_nt) and same_bits(nn2, want_nn)
        nt3, nn3 = ops.conv_taps_pack_bf16(W, want_nn=False)
        assert nn3 is None and same_bits(nt3, want_nt)


# N * Cin * k one below, at and one above what one workgroup covers per pass, and a size at which the capped grid loops
PERMUTE_SHAPES = [(31, 11, 3), (16, 16, 4), (41, 5, 5), (700, 1000, 3)]


def test_permute_sizes_follow_the_kernel_constants():
    span = MU.PERMUTE_SPAN
    totals = [N * C * k for N, C, k in PERMUTE_SHAPES]
    assert totals[:3] == [span - 1, span, span + 1]
    assert totals[3] > MU.MAX_BLOCKS * span and totals[3] % MU.PERMUTE_VEC == 0 and totals[0] % MU.PERMUTE_VEC != 0


@pytest.mark.parametrize("N,Cin,k", PERMUTE_SHAPES)
def test_permute_both_directions(ops, N, Cin, k):
    g = torch.Generator().manual_seed(N + Cin + k)
    W = torch.randn(N, Cin, k, generator=g).cuda()
    want = W.permute(0, 2, 1).reshape(N, k * Cin).contiguous()
    out = torch.full((N, k * Cin), float("nan"), device="cuda")
    got = ops.conv_taps_permute_f32(W, N, Cin, k, True, out=out)
    assert got is out and same_bits(got, want)
    assert same_bits(ops.conv_taps_permute_f32(W, N, Cin, k, True), want)
    # back: the round trip is the identity
    back = ops.conv_taps_permute_f32(want, N, Cin, k, False, out=torch.full((N, Cin, k), float("nan"), device="cuda"))
    assert same_bits(back, W)
    # accumulate onto a seeded destination: one fp32 addition per element
    dst0 = torch.randn(N, Cin, k, generator=g).cuda()
    dst = dst0.clone()
    ops.conv_taps_permute_f32(want, N, Cin, k, False, out=dst, accumulate=True)
    assert same_bits(dst, dst0 + W)
    ops.conv_taps_permute_f32(want, N, Cin, k, False, out=dst, accumulate=False)
    assert same_bits(dst, W)


GATHER_CASES = [(3, 1, 1), (3, 3, 1), (3, 9, 1), (5, 3, 1), (3, 1, 3), (1, 1, 1)]
GATHER_T_OUT = (1, MU.GATHER_ROWS - 1, MU.GATHER_ROWS, MU.GATHER_ROWS + 1)


@pytest.mark.parametrize("dtype", [torch.float32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("k,dilation,stride", GATHER_CASES)
def test_gather_windows(ops, k, dilation, stride, dtype):
    for C in (16, 32, 48, 1024):
        for nseq in (1, 3):
            for t_out in GATHER_T_OUT:
                t_in = (t_out - 1) * stride + (k - 1) * dilation + 1 + (stride - 1)      # (a remainder the stride leaves unused)
                assert t_in < 32 and (t_in - (k - 1) * dilation - 1) // stride + 1 == t_out
                g = torch.Generator().manual_seed(C + 7 * nseq + t_out)
                x_buf = torch.randn(nseq * t_in, C + 16, generator=g)
                # column 0 encodes (sequence, frame) exactly, in bf16 too: a read across a sequence boundary shows
                seq, frame = torch.arange(nseq * t_in) // t_in, torch.arange(nseq * t_in) % t_in
                x_buf[:, 0] = (32 * seq + frame).float()
                x_buf = x_buf.to(dtype).cuda()
                x = x_buf[:, :C]
                s, t, j = torch.meshgrid(torch.arange(nseq), torch.arange(t_out), torch.arange(k), indexing="ij")
                idx = (s * t_in + t * stride + j * dilation).reshape(-1).cuda()
                want = x[idx].reshape(nseq * t_out, k * C)
                code = want.float()[:, 0::C].reshape(nseq, t_out, k).cpu()
                assert torch.equal(code, (32 * s + t * stride + j * dilation).float())
                case = (C, nseq, t_out)
                ob_buf = nan_buffer(nseq * t_out, k * C + 16, BF16)
                if dtype == BF16:
                    ob, of = ops.tap_gather(x, nseq, t_in, C, k, dilation, stride, out_bf16=ob_buf[:, :k * C])
                    assert of is None and same_bits(ob, want), case
                    assert same_bits(ops.tap_gather(x, nseq, t_in, C, k, dilation, stride)[0], want), case
                else:
                    of_buf = nan_buffer(nseq * t_out, k * C + 16, torch.float32)
                    ob, of = ops.tap_gather(x, nseq, t_in, C, k, dilation, stride, out_bf16=ob_buf[:, :k * C], out_f32=of_buf[:, :k * C])
                    assert same_bits(of, want), case
                    assert same_bits(ob, ops.cast_pad_bf16(want.contiguous(), k * C)), case
                    assert bool(of_buf[:, k * C:].isnan().all()), case
                    only_b, none = ops.tap_gather(x, nseq, t_in, C, k, dilation, stride, want_bf16=True, want_f32=False)
                    assert none is None and same_bits(only_b, ob), case
                    none, only_f = ops.tap_gather(x, nseq, t_in, C, k, dilation, stride)
                    assert none is None and same_bits(only_f, want), case
                assert bool(ob_buf[:, k * C:].isnan().all()), case


def test_gather_many_rows_loops_over_the_capped_grid(ops):
    """more output rows than MAX_BLOCKS workgroups cover in one pass: the grid-stride loop over row passes"""
    C, k, nseq, t_in = 16, 3, 3, MU.MAX_BLOCKS * MU.GATHER_ROWS // 3 + 40
    t_out = t_in - 2
    assert nseq * t_out > MU.MAX_BLOCKS * MU.GATHER_ROWS
    x = torch.randn(nseq * t_in, C, generator=torch.Generator().manual_seed(3)).cuda()
    idx = (torch.arange(nseq).view(-1, 1, 1) * t_in + torch.arange(t_out).view(1, -1, 1) + torch.arange(k).view(1, 1, -1)).reshape(-1).cuda()
    ob, of = ops.tap_gather(x, nseq, t_in, C, k, want_bf16=True, want_f32=True)
    want = x[idx].reshape(nseq * t_out, k * C)
    assert same_bits(of, want) and same_bits(ob, ops.cast_pad_bf16(want, k * C))
