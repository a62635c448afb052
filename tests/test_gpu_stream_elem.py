"""The streaming kernels behind every training step (csrc/dhaug_elem.hip): operand packing, column sums, activation backward, the
rank-one logit step and the three Adam forms, kernel by kernel against plain restatements (tests/stream_elem_util.py) at ragged
rows (1, 63, 64, 65, 1000), ragged columns (1 .. 257, as far as an entry point's contract allows) and ONE shape per kernel that
makes its capped grid-stride loop take a second, ragged trip (stream_elem_util.MP_*, derived from the launch arithmetic).

A  data movement and rounding, bit for bit: torch's .to(bfloat16) / .to(float16) round to nearest even and every residual of the
   splits is one fp32 subtraction, so the host replay is exact.  Sources are column blocks of NaN-filled buffers, outputs sit
   behind NaN-payload guards, leading dimensions go beyond the width.  Special values: +-0, +-inf, rounding ties both ways, the
   largest fp32 that must become bf16 inf, fp32 subnormals (kept, as torch keeps them); NaN in is NaN out.
   dhaug_rank1_mask_bf16 decides y > 0 on the bf16 bits, dhaug_act_backward_bf16 with a float compare: they agree on every finite
   mask (+-0, +-inf, +-subnormal planted).  A NaN mask is OUTSIDE rank1_mask's contract (the sign bit of the NaN decides) and is not
   tested.  Its pad columns [N, pad) are zeros of the seed's sign (seed * 0), as the replay's are.
B  column sums on integers in [-8, 8]: exact in both types, every partial sum below 2^24, so the order of the atomics does not
   matter and the result equals the int64 sum; the fold of rows r and r + M/2 on randn halves that cancel: exactly 0.0.
C  Adam against fp64 / fp32 restatements of adam_kernel's formula with pose_elem_util.rule; the fused two-launch step against the
   four launches bit for bit, the unfused side of the large case against the fp64 rule.
D  bounds: every output behind guards, inputs unchanged, columns beyond the width keep their payload.
   (Argument errors need no device: tests/test_cpu_boundary.py::test_stream_elem_argument_errors; that the comparisons used here
   can fail: test_stream_elem_references_reject_emulated_faults.)

entry point                               tests
dhaug_cast_pad_bf16                       test_cast_pad_sizes, test_casts_multi_pass, test_casts_nan_in_nan_out, test_stream_outputs_stay_in_bounds
dhaug_cast_transpose_bf16                 test_cast_transpose_sizes, test_casts_multi_pass, test_casts_nan_in_nan_out,
                                          test_stream_outputs_stay_in_bounds
dhaug_split_bf16                          test_split_bf16_paths, test_splits_multi_pass, test_casts_nan_in_nan_out, test_stream_outputs_stay_in_bounds
dhaug_split_f16                           test_split_f16_paths, test_splits_multi_pass, test_stream_outputs_stay_in_bounds
dhaug_repack_weights                      test_repack_weights_equals_the_casts, test_stream_outputs_stay_in_bounds
dhaug_colsum_f32, dhaug_colsum_bf16       test_colsum_exact, test_colsum_f32_vector_switch, test_colsum_fold_cancels, test_colsum_randn,
                                          test_colsum_empty, test_stream_outputs_stay_in_bounds
dhaug_act_backward_bf16                   test_act_backward_bf16_strided, test_act_backward_bf16_in_place, test_act_backward_multi_pass,
                                          test_stream_outputs_stay_in_bounds
dhaug_act_backward_f32                    test_act_backward_f32_and_add_sizes, test_stream_outputs_stay_in_bounds
dhaug_add_f32                             test_act_backward_f32_and_add_sizes, test_stream_outputs_stay_in_bounds
dhaug_rank1_mask_bf16                     test_rank1_mask_reference, test_rank1_mask_multi_pass, test_rank1_mask_wrapper_needs_a_padded_mask,
                                          test_stream_outputs_stay_in_bounds
dhaug_rank1_bits_bf16                     test_rank1_bits_reference, test_stream_outputs_stay_in_bounds
dhaug_adam_step                           test_adam_step_sizes, test_stream_outputs_stay_in_bounds
dhaug_adam_step_dev, dhaug_counter_add    test_adam_step_dev_sizes, test_stream_outputs_stay_in_bounds
dhaug_adam_repack_step                    test_fused_adam_equals_unfused_small_nets, test_fused_adam_wraps_its_grid
"""
import argparse
import os
import sys
import time

import pytest
import torch

import stream_elem_util as S
from test_gpu_pose_elem import PAYLOAD16, Guarded, bits, dev, ptr, same_bits, stream

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
F64, F32, BF16, F16 = torch.float64, torch.float32, torch.bfloat16, torch.float16
NAN = float("nan")


@pytest.fixture(scope="module")
def M():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    sys.path.insert(0, ROOT)
    import dhaug_amd
    L = dhaug_amd._lib.lib()
    from dhaug_amd import fused, ops, optim
    return argparse.Namespace(L=L, ops=ops, lib=dhaug_amd._lib, fused=fused, optim=optim)


def framed(x, ld, lead=0, fill=NAN):
    """x (rows, cols) on the device as the column block [lead, lead + cols) of a `fill`-filled (rows, ld) buffer"""
    rows, cols = x.shape
    wide = torch.full((rows, ld), fill, dtype=x.dtype, device="cuda")
    wide[:, lead:lead + cols] = x.cuda()
    return wide, wide[:, lead:lead + cols]


def dgen(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


def guarded_rows(rows, ld, dtype):
    b = Guarded(rows * ld, dtype)
    return b, b.out.view(rows, ld)


def check_rows(b, view, width, ref, name, nan_ok=False):
    """guards intact, columns [0, width) equal ref bit for bit, columns beyond keep the payload"""
    b.check(name, written=False)
    assert S.rows_ok(view, width, ref.to(view.device), nan_ok, PAYLOAD16), name


# ====================================================================================================== A. the three casts
def _pads_even(cols):
    """pad_cols - cols of 0 (even cols) or 1 (odd cols), and of more than 2"""
    return [S.ceil_to(cols, 2), S.ceil_to(cols, 2) + 4]


@pytest.mark.parametrize("rows", S.RAGGED_ROWS)
def test_cast_pad_sizes(M, rows):
    for cols in S.RAGGED_COLS:
        x = S.special_matrix(rows, cols, S.SPECIAL_F32, seed=rows * 1000 + cols)
        wide, src = framed(x, cols + 3, lead=2)
        keep = wide.clone()
        for pad in _pads_even(cols):
            ld = pad + 6
            b, view = guarded_rows(rows, ld, BF16)
            rc = M.L.dhaug_cast_pad_bf16(ptr(src), src.stride(0), ptr(view), ld, rows, cols, pad, stream())
            assert rc == 0
            check_rows(b, view, pad, S.cast_pad_ref(x, pad), ("cast_pad", rows, cols, pad))
        assert S.same_bits_nan(wide, keep)
        assert same_bits(M.ops.cast_pad_bf16(dev(x)), S.cast_pad_ref(x, S.ceil_to(cols, 16)).cuda())


@pytest.mark.parametrize("rows", S.RAGGED_ROWS)
def test_cast_transpose_sizes(M, rows):
    for cols in S.RAGGED_COLS:
        x = S.special_matrix(rows, cols, S.SPECIAL_F32, seed=rows * 1000 + cols + 1)
        wide, src = framed(x, cols + 5, lead=1)
        for pad in (S.ceil_to(rows, 16), rows + 40):                       # (rows + 40: a whole tile row of zeros behind the data)
            ld = pad + 3
            b, view = guarded_rows(cols, ld, BF16)
            rc = M.L.dhaug_cast_transpose_bf16(ptr(src), src.stride(0), ptr(view), ld, rows, cols, pad, stream())
            assert rc == 0
            check_rows(b, view, pad, S.cast_transpose_ref(x, pad), ("cast_transpose", rows, cols, pad))


def test_casts_multi_pass(M):
    rows, cols, pad = S.MP_CAST_PAD
    n, per = S.items("cast_pad")
    assert per < n <= per + 256 and n % 256 != 0                           # a second trip of one partly filled workgroup
    x = torch.randn(rows, cols, device="cuda", generator=dgen(1))
    assert same_bits(M.ops.cast_pad_bf16(x, pad), S.cast_pad_ref(x, pad))
    rows, cols, pad = S.MP_CAST_TRANSPOSE
    n, per = S.items("cast_transpose")
    assert per < n and rows % 32 != 0 and pad % 32 != 0 and cols % 32 != 0  # the last tile is clipped in both directions
    x = torch.randn(rows, cols, device="cuda", generator=dgen(2))
    assert same_bits(M.ops.cast_transpose_bf16(x, pad), S.cast_transpose_ref(x, pad))


def test_casts_nan_in_nan_out(M):
    x = torch.randn(5, 12)
    x.reshape(-1)[:4] = S.f32_from_bits(S.NAN_F32)
    x.reshape(-1)[30:34] = S.f32_from_bits(S.NAN_F32)
    nan = torch.isnan(x)
    xd = dev(x)
    assert torch.equal(torch.isnan(M.ops.cast_pad_bf16(xd, 12)).cpu(), nan)
    assert torch.equal(torch.isnan(M.ops.cast_transpose_bf16(xd, 16)[:, :5]).cpu(), nan.t())
    s = M.ops.split_bf16(xd, 2, 6, 16)
    for k in range(3):
        assert torch.equal(torch.isnan(s[:, 16 * k:16 * k + 12]).cpu(), nan), k
    assert torch.isnan(M.ops.split_f16(xd, 2, 16)[:, :12]).cpu()[nan].all()


# =========================================================================================================== A. the splits
# source layouts: (name, lead columns, extra columns behind) -- which path split_kernel takes is decided by (ld % 4, base % 16)
def _layouts(cols):
    return [("aligned rows from the buffer's base: vector", 0, (-cols) % 4, False),
            ("column block at 4 floats, ld % 4 == 0: vector", 4, (-cols - 4) % 4 + 4, False),
            ("column block at 1 float: element", 1, (-cols - 1) % 4, True), ("ld % 4 != 0: element", 0, (-cols) % 4 + 1, True)]


SPLIT_COLS = [1, 7, 8, 9, 31, 33, 100, 257]                                # cols % 8 in {0, 1, 7} and two others


def _split_paths(M, layout, half, words, call):
    for rows in (1, 63, 65):
        for cols in SPLIT_COLS:
            x = S.special_matrix(rows, cols, words, seed=rows * 1000 + cols + 2)
            for name, lead, extra, element in _layouts(cols):
                ld = lead + cols + extra
                wide, src = framed(x, ld, lead=lead)
                assert (ld % 4 == 0 and src.data_ptr() % 16 == 0) == (not element), (name, ld)   # the layout selects the path it names
                for pad in (S.ceil_to(cols, 8), S.ceil_to(cols, 8) + 16):          # a straddling chunk; whole zero chunks behind it
                    w = len(layout) * pad
                    b, view = guarded_rows(rows, w, F16 if half else BF16)
                    assert call(src, ld, view, rows, cols, pad) == 0
                    ref = S.split_ref(x, layout, pad, half)
                    check_rows(b, view, w, ref, (name, rows, cols, pad), nan_ok=True)
                    got = view.view(rows, len(layout), pad)
                    assert not bits(got[:, :, cols:]).any()                         # pad columns of every segment
                    for s, k in enumerate(layout):                                 # the duplicated segments: equal bits
                        assert torch.equal(bits(got[:, s]), bits(got[:, layout.index(k)]))


@pytest.mark.parametrize("mode,terms", sorted(S.SPLIT_BF16_LAYOUT))
def test_split_bf16_paths(M, mode, terms):
    """every segment equals the replay hi = bf16(x), mid = bf16(x - hi), lo = bf16((x - hi) - mid) (inf - inf = NaN in mid / lo:
    compared as NaN), in each of the four source layouts, with cols % 8 in {0, 1, 7} and pad_cols - cols >= 8"""
    call = lambda src, ld, view, rows, cols, pad: M.L.dhaug_split_bf16(ptr(src), ld, ptr(view), rows, cols, pad, mode, terms, stream())
    _split_paths(M, S.SPLIT_BF16_LAYOUT[(mode, terms)], False, S.SPECIAL_F32, call)


@pytest.mark.parametrize("mode", sorted(S.SPLIT_F16_LAYOUT))
def test_split_f16_paths(M, mode):
    """the same with IEEE-half pieces hi = f16(x), lo = f16(x - hi), |x| < 65 504"""
    call = lambda src, ld, view, rows, cols, pad: M.L.dhaug_split_f16(ptr(src), ld, ptr(view), rows, cols, pad, mode, stream())
    _split_paths(M, S.SPLIT_F16_LAYOUT[mode], True, S.SPECIAL_F16_SAFE, call)


def test_splits_multi_pass(M):
    rows, cols, pad = S.MP_SPLIT
    n, per = S.items("split")
    assert per < n <= per + 256 and n % 256 != 0
    x = torch.randn(rows, cols, device="cuda", generator=dgen(3))
    assert same_bits(M.ops.split_bf16(x, 0, 3, pad), S.split_ref(x, S.SPLIT_BF16_LAYOUT[(0, 3)], pad, False))
    assert same_bits(M.ops.split_bf16(x, 2, 6, pad), S.split_ref(x, S.SPLIT_BF16_LAYOUT[(2, 6)], pad, False))
    assert same_bits(M.ops.split_f16(x, 0, pad), S.split_ref(x, S.SPLIT_F16_LAYOUT[0], pad, True))
    assert same_bits(M.ops.split_f16(x, 2, pad), S.split_ref(x, S.SPLIT_F16_LAYOUT[2], pad, True))


# ======================================================================================================= A. repack_weights
def _repack_descs(M, shapes, seed):
    """weights, their (nt, nn) outputs behind guards and the device descriptor array"""
    g = S.gen(seed)
    Ws = [dev(torch.randn(n, k, generator=g)) for n, k in shapes]
    descs = (M.lib.RepackDesc * len(shapes))()
    outs = []
    for i, W in enumerate(Ws):
        N, K = W.shape
        Kp, Np = S.ceil_to(K, 16), S.ceil_to(N, 16)
        nt, nn = Guarded(N * Kp, BF16), Guarded(K * Np, BF16)
        descs[i].W, descs[i].nt, descs[i].nn = W.data_ptr(), nt.out.data_ptr(), nn.out.data_ptr()
        descs[i].N, descs[i].K, descs[i].Kp, descs[i].Np = N, K, Kp, Np
        outs.append((nt, nn, Kp, Np))
    d = torch.frombuffer(bytearray(bytes(descs)), dtype=torch.uint8).cuda()
    return Ws, outs, d


def test_repack_weights_equals_the_casts(M):
    """blockIdx.y picks the descriptor (weights from 3 to 312 000 elements); the (520, 600) weight makes both loops wrap their 32
    workgroups (19 trips of pairs, 11 of tiles)"""
    Ws, outs, d = _repack_descs(M, S.REPACK_SHAPES, seed=21)
    assert M.L.dhaug_repack_weights(ptr(d), len(Ws), stream()) == 0
    for W, (nt, nn, Kp, Np) in zip(Ws, outs):
        N, K = W.shape
        nt.check(("nt", N, K)); nn.check(("nn", N, K))
        assert same_bits(nt.out.view(N, Kp), S.cast_pad_ref(W, Kp)) and same_bits(nn.out.view(K, Np), S.cast_transpose_ref(W, Np))
        assert same_bits(nt.out.view(N, Kp), M.ops.cast_pad_bf16(W, Kp)) and same_bits(nn.out.view(K, Np), M.ops.cast_transpose_bf16(W, Np))


# ==================================================================================================== A. activation backward
SLOPE = 0.01


@pytest.mark.parametrize("act", [0, 1, 2])
def test_act_backward_bf16_strided(M, act):
    """ld_g, ld_y, ld_dst all different, multiples of 8 beyond N; N = 8 included; +-0, +-inf, +-subnormal masks among randn"""
    for rows in S.RAGGED_ROWS:
        for N in (8, 16, 104, 256):
            g = S.gen(rows * 1000 + N + act)
            gv = torch.randn(rows, N, generator=g).to(BF16)
            yv = S.plant_mask(torch.randn(rows, N, generator=g).to(BF16), seed=rows + N)
            gw, gsrc = framed(gv, N + 8, lead=0)
            yw, ysrc = framed(yv, N + 16, lead=8)
            keep = (gw.clone(), yw.clone())
            ld = N + 24
            b, view = guarded_rows(rows, ld, BF16)
            rc = M.L.dhaug_act_backward_bf16(ptr(gsrc), N + 8, ptr(ysrc), N + 16, ptr(view), ld, rows, N, act, SLOPE, stream())
            assert rc == 0
            check_rows(b, view, N, S.act_backward_ref(gv, yv, act, SLOPE), ("act_backward_bf16", act, rows, N))
            assert S.same_bits_nan(gw, keep[0]) and S.same_bits_nan(yw, keep[1])


@pytest.mark.parametrize("act", [0, 1, 2])
def test_act_backward_bf16_in_place(M, act):
    """out is g itself: contiguous, and as a column block of a wider buffer whose other columns stay as they were (what the critic
    step issues after a GEMM that wrote into a wider buffer)"""
    for rows in (1, 65, 1000):
        for N in (8, 104):
            g = S.gen(rows + N + act)
            gv = torch.randn(rows, N, generator=g).to(BF16)
            yv = S.plant_mask(torch.randn(rows, N, generator=g).to(BF16), seed=rows + N + 1)
            ref = S.act_backward_ref(gv, yv, act, SLOPE).cuda()
            gd, yd = dev(gv), dev(yv)
            out = M.ops.act_backward(gd, yd, act, SLOPE, out=gd)
            assert out is gd and same_bits(gd, ref) and same_bits(yd, yv.cuda())
            gw, gsrc = framed(gv, N + 16, lead=8)
            yw, ysrc = framed(yv, N + 8, lead=0)
            M.ops.act_backward(gsrc, ysrc, act, SLOPE, out=gsrc)
            assert same_bits(gw[:, 8:8 + N], ref) and torch.isnan(gw[:, :8]).all() and torch.isnan(gw[:, 8 + N:]).all()


def test_act_backward_multi_pass(M):
    rows, N = S.MP_ACT_BF16
    n, per = S.items("act_bf16")
    assert per < n <= per + 256 and n % 256 != 0
    g, y = (torch.randn(rows, N, device="cuda", generator=dgen(4 + i)).to(BF16) for i in range(2))
    for act in (1, 2):
        assert same_bits(M.ops.act_backward(g, y, act, SLOPE), S.act_backward_ref(g, y, act, SLOPE))
    n = S.MP_FLAT
    g, y = (torch.randn(n, device="cuda", generator=dgen(6 + i)) for i in range(2))
    for act in (1, 2):
        assert same_bits(M.ops.act_backward(g, y, act, SLOPE), S.act_backward_ref(g, y, act, SLOPE))
    assert same_bits(M.ops.add_f32(g, y), g + y)


@pytest.mark.parametrize("n", [1, 255, 257, 1000])
def test_act_backward_f32_and_add_sizes(M, n):
    """one fp32 multiplication / addition per element: bit for bit (ops.add_f32's multi-pass size: test_act_backward_multi_pass)"""
    g = S.gen(n)
    gv, yv = torch.randn(n, generator=g), torch.randn(n, generator=g)
    yv[::7] = 0.0
    yv[3::11] = -0.0
    for act in (0, 1, 2):
        assert same_bits(M.ops.act_backward(dev(gv), dev(yv), act, SLOPE).cpu(), S.act_backward_ref(gv, yv, act, SLOPE))
    assert same_bits(M.ops.add_f32(dev(gv), dev(yv)).cpu(), gv + yv)


# ================================================================================================================ A. rank one
def _rank1_inputs(rows, N, pad, seed):
    """seed (rows, 3) column 0, weights (N, 5) column 0, mask (rows, pad) with the planted values: bf16, host"""
    g = S.gen(seed)
    sd = torch.randn(rows, 3, generator=g).to(BF16)
    w = torch.randn(N, 5, generator=g).to(BF16)
    y = S.plant_mask(torch.randn(rows, pad, generator=g).to(BF16), seed=seed + 1)
    return sd, w, y


@pytest.mark.parametrize("act,slope", [(1, 0.0), (2, 0.2)])
@pytest.mark.parametrize("N", [1, 100, 256, 1000, 1010])
def test_rank1_mask_reference(M, N, act, slope):
    """against bf16(bf16(seed * w) * (y > 0 ? 1 : dneg)) with every leading dimension beyond its minimum (N = 1010: pad_cols is
    exactly DHAUG_RANK1_MAX_N = 1024), and against dhaug_act_backward_bf16 of the same rank-one image"""
    pad = S.ceil_to(N, 16)
    assert N != 1010 or pad == 1024
    for rows in (1, 63, 65, 1000):
        sd, w, y = _rank1_inputs(rows, N, pad, seed=rows * 7 + N)
        sdd, wd = dev(sd), dev(w)
        yw, ysrc = framed(y, pad + 8, lead=0)
        ld = pad + 16
        b, view = guarded_rows(rows, ld, BF16)
        rc = M.L.dhaug_rank1_mask_bf16(ptr(sdd), 3, ptr(wd), 5, ptr(ysrc), pad + 8, ptr(view), ld, rows, N, pad, act, slope, stream())
        assert rc == 0
        ref = S.rank1_ref(sd[:, 0], w[:, 0], y, N, pad, slope if act == 2 else 0.0)
        check_rows(b, view, pad, ref, ("rank1_mask", N, act, rows))
        assert (view[:, N:pad].float() == 0.0).all()
        wz = torch.zeros(pad)
        wz[:N] = w[:, 0].float()
        image = (sd[:, :1].float() * wz[None, :]).to(BF16)
        via_act = M.ops.act_backward(dev(image), dev(y), act, slope)
        assert same_bits(view[:, :pad], via_act), ("rank1_mask vs act_backward", N, act, rows)


def test_rank1_mask_multi_pass(M):
    rows, N, pad = S.MP_RANK1
    n, per = S.items("rank1")
    assert per < n <= per + 256 and n % 256 != 0
    sd = torch.randn(rows, 1, device="cuda", generator=dgen(8)).to(BF16)
    w = torch.randn(N, 1, device="cuda", generator=dgen(9)).to(BF16)
    y = S.plant_mask(torch.randn(rows, pad, device="cuda", generator=dgen(10)).to(BF16), seed=3)
    got = M.ops.rank1_mask(sd, w[:, 0], y, N, 2, 0.2)
    assert same_bits(got, S.rank1_ref(sd[:, 0], w[:, 0], y, N, pad, 0.2))


def test_rank1_mask_wrapper_needs_a_padded_mask(M):
    """ops.rank1_mask returns (M, ceil16 n): a mask narrower than that (n = 100 in 104 columns) would leave columns [104, 112) of the
    result unwritten for the K-padded GEMM behind it; the wrapper refuses it (critic_step's mm() takes this path only with
    mask.shape[1] >= ceil16 K), and with the padded mask every column of a poisoned output is written"""
    sd, w, y = _rank1_inputs(65, 100, 112, seed=5)
    sdd, wd, yd = dev(sd), dev(w), dev(y)
    out = torch.full((65, 112), NAN, dtype=BF16, device="cuda")
    with pytest.raises(AssertionError):
        M.ops.rank1_mask(sdd, wd[:, 0], yd[:, :104], 100, 1, 0.0, out=out)
    got = M.ops.rank1_mask(sdd, wd[:, 0], yd, 100, 1, 0.0, out=out)
    assert got is out and not torch.isnan(out).any() and (out[:, 100:].float() == 0.0).all()
    assert same_bits(out, S.rank1_ref(sd[:, 0], w[:, 0], y, 100, 112, 0.0).cuda())


@pytest.mark.parametrize("act,slope", [(1, 0.0), (2, 0.2)])
@pytest.mark.parametrize("rows", [1, 33, 100, 128, 1000])
def test_rank1_bits_reference(M, rows, act, slope):
    """the same reference with the mask as a sign-bit array (N = 256); rows not a multiple of 32, the array sized by encode_bits"""
    sd, w, y = _rank1_inputs(rows, 256, 256, seed=rows)
    yd = dev(y)
    bitsarr = M.fused.encode_bits(yd.float() > 0)
    assert bitsarr.numel() == (rows + 127) // 128 * 4 * 4 * 64
    ld = 256 + 8
    b, view = guarded_rows(rows, ld, BF16)
    sdd, wd = dev(sd), dev(w)
    rc = M.L.dhaug_rank1_bits_bf16(ptr(sdd), 3, ptr(wd), 5, ptr(bitsarr), ptr(view), ld, rows, act, slope, stream())
    assert rc == 0
    check_rows(b, view, 256, S.rank1_ref(sd[:, 0], w[:, 0], y, 256, 256, slope if act == 2 else 0.0), ("rank1_bits", rows, act))


# ============================================================================================================ B. column sums
COLSUM_M = [1, 2, 3, 63, 64, 65, 72, 1000, 1001]
COLSUM_N = [1, 63, 64, 65, 257]


def _colsum_abi(M, dtype, src, ld, out, rows, N, accumulate):
    fn = M.L.dhaug_colsum_bf16 if dtype == BF16 else M.L.dhaug_colsum_f32
    return fn(ptr(src), ld, ptr(out), rows, N, accumulate, stream())


def _exact(name, got, x):
    assert S.exact_sums_ok(got, x), name


@pytest.mark.parametrize("dtype", [F32, BF16])
def test_colsum_exact(M, dtype):
    for rows in COLSUM_M:
        for N in COLSUM_N:
            x = S.int_matrix(rows + 5, N, seed=rows * 1000 + N)
            # ld > N: a column block of a NaN-filled buffer; five more rows behind (a row slice src[:rows] of a taller buffer)
            wide, src = framed(x.to(dtype), N + 3, lead=2)
            wide[rows:] = NAN
            out = Guarded(N, F32)
            assert _colsum_abi(M, dtype, src, N + 3, out.out, rows, N, 0) == 0
            out.check(("colsum", dtype, rows, N))
            _exact(("colsum", dtype, rows, N), out.out, x[:rows])
            out.out.fill_(5.0)
            assert _colsum_abi(M, dtype, src, N + 3, out.out, rows, N, 1) == 0
            out.check(("colsum accumulate", dtype, rows, N))
            _exact(("colsum accumulate", dtype, rows, N), out.out - 5.0, x[:rows])
            if N in (1, 65):                                                  # the wrapper, ld = N (N = 1: ld = 1), a row slice
                tall = x.to(dtype).cuda()
                got = M.ops.colsum(tall[:rows])
                _exact(("ops.colsum", dtype, rows, N), got, x[:rows])
                acc = torch.full((N,), -3.0, device="cuda")
                M.ops.colsum(tall[:rows], out=acc, accumulate=True)
                _exact(("ops.colsum accumulate", dtype, rows, N), acc + 3.0, x[:rows])


# fp32, both sides of the vector switch (N % 4 == 0, ld % 4 == 0, 16-byte base, Mw >= 4 096 rows walked):
# (rows, N, ld, lead, which kernel)
VECTOR_SWITCH = [(8190, 8, 8, 0, "scalar: Mw = 4 095"), (8192, 8, 8, 0, "vector, folded"), (4097, 8, 12, 4, "vector, odd M: no fold"),
                 (8192, 6, 8, 0, "scalar: N % 4 != 0"), (8192, 8, 12, 1, "scalar: base offset by one float"),
                 (8192, 260, 264, 4, "vector, two column blocks")]


@pytest.mark.parametrize("rows,N,ld,lead,which", VECTOR_SWITCH)
def test_colsum_f32_vector_switch(M, rows, N, ld, lead, which):
    x = S.int_matrix(rows, N, seed=rows + N + lead)
    wide, src = framed(x, ld, lead=lead)
    vector = N % 4 == 0 and ld % 4 == 0 and src.data_ptr() % 16 == 0 and (rows // 2 if rows % 2 == 0 else rows) >= 4096
    assert vector == which.startswith("vector"), which
    out = Guarded(N, F32)
    assert _colsum_abi(M, F32, src, ld, out.out, rows, N, 0) == 0
    out.check(which)
    _exact(which, out.out, x)
    if rows % 2 == 0:
        y = S.folded(torch.randn(rows, N, generator=S.gen(rows + N)))
        wide, src = framed(y, ld, lead=lead)
        assert _colsum_abi(M, F32, src, ld, out.out, rows, N, 0) == 0
        assert float(out.out.abs().max()) == 0.0, which


@pytest.mark.parametrize("dtype", [F32, BF16])
def test_colsum_fold_cancels(M, dtype):
    """second half the exact negative of the first on randn data: every column is exactly 0.0 for every even M (72: the batch the
    kernel's comment names), in both types"""
    for rows in [m for m in COLSUM_M if m % 2 == 0] + [8190, 8192]:
        for N in (1, 64, 65):
            y = S.folded(torch.randn(rows, N, generator=S.gen(rows + N)).to(dtype))
            got = M.ops.colsum(dev(y))
            assert float(got.abs().max()) == 0.0, (dtype, rows, N)


@pytest.mark.parametrize("dtype,rows,N", [(F32, 1001, 65), (BF16, 1001, 65), (F32, 8192, 64)])
def test_colsum_randn(M, dtype, rows, N):
    """one randn case per kernel at the bound of test_colsum_f32_vector_path: 8 * (3e-7 * sqrt(M) * 4)"""
    x = torch.randn(rows, N, generator=S.gen(rows)).to(dtype)
    err = S.maxabs(M.ops.colsum(dev(x)), x.double().sum(0))
    bound = 3e-7 * rows ** 0.5 * 4 * 8
    print("colsum randn %s %d x %d: err %.3e bound %.3e" % (dtype, rows, N, err, bound))
    assert err <= bound


@pytest.mark.parametrize("dtype", [F32, BF16])
def test_colsum_empty(M, dtype):
    """M = 0: zeros without accumulate, out left alone with it"""
    src = torch.empty(0, 9, dtype=dtype, device="cuda")
    out = Guarded(9, F32)
    assert _colsum_abi(M, dtype, None, 9, out.out, 0, 9, 0) == 0
    out.check("empty")
    assert not bits(out.out).any()
    out.out.copy_(torch.arange(9.0))
    assert _colsum_abi(M, dtype, None, 9, out.out, 0, 9, 1) == 0
    assert torch.equal(out.out.cpu(), torch.arange(9.0))
    assert not bits(M.ops.colsum(src)).any()


# ================================================================================================================== C. Adam
def _adam_run(M, n, devcount):
    c = S.adam_case(n)
    p, m, v = dev(c["p0"]), torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
    count = torch.zeros(1, dtype=torch.int32, device="cuda")
    for step, gr in zip(S.ADAM_STEPS, c["grads"]):
        g = dev(gr)
        if devcount:
            count.fill_(step - 1)                                         # the wrapper advances it; the kernel reads it on the device
            M.ops.adam_step_dev(p, g, m, v, count, S.ADAM_LR, S.ADAM_BETAS, S.ADAM_EPS, S.ADAM_GSCALE)
            assert int(count.item()) == step
        else:
            M.ops.adam_step(p, g, m, v, step, S.ADAM_LR, S.ADAM_BETAS, S.ADAM_EPS, S.ADAM_GSCALE)
        assert same_bits(g.cpu(), gr)
    name = "adam_step%s n=%d" % ("_dev" if devcount else "", n)
    S.adam_check(name, (p, m, v), c)
    if n > 1:                                                             # g = m = v = 0: the parameter keeps its bits
        z = S.ADAM_ZERO_AT
        assert same_bits(p[z:z + 1].cpu(), c["p0"][z:z + 1]) and m[z].item() == 0.0 and v[z].item() == 0.0, name


@pytest.mark.parametrize("n", S.ADAM_SIZES)
def test_adam_step_sizes(M, n):
    """steps 1, 2, 3, 1000 with grad_scale 0.5 against the fp64 restatement: max|gpu - ref64| <= max(2e-7, 4 max|ref32 - ref64|)
    for p, m and v; the bound for p stays below lr / 10 (a skipped element is off by about lr); more than 99 % of p moved by lr / 2"""
    _adam_run(M, n, devcount=False)


@pytest.mark.parametrize("n", S.ADAM_SIZES)
def test_adam_step_dev_sizes(M, n):
    _adam_run(M, n, devcount=True)


def _fused_pair(M, build, lr=1e-4):
    """two FusedAdam optimizers over identically initialised parameters: the two-launch step and the four launches it replaces"""
    opts = []
    for fused in (True, False):
        old = M.optim.FUSED_STEP
        M.optim.FUSED_STEP = fused
        try:
            opts.append(M.optim.FusedAdam(build(), lr=lr, betas=(0.5, 0.9)))
        finally:
            M.optim.FUSED_STEP = old
    return opts


def _fused_step(M, opts, grads):
    for fused, opt in zip((True, False), opts):
        opt.zero_grad()
        for p, g in zip(opt._params, grads):
            p.grad.copy_(g)
        old = M.optim.FUSED_STEP
        M.optim.FUSED_STEP = fused
        try:
            opt.step()
        finally:
            M.optim.FUSED_STEP = old


def _fused_equal(a, b, step):
    assert int(a.step_dev.item()) == step == int(b.step_dev.item())
    for name in ("flat_param", "exp_avg", "exp_avg_sq"):
        assert torch.equal(bits(getattr(a, name)), bits(getattr(b, name))), (step, name)


NETS = {"90 tiles of 64 x 64, ragged both ways": [S.NN_TILE_WEIGHT, (520,), (3, 520), (3,)],
        "K < 16 and N = 1": [(1, 7), (1,), (5, 3), (5,)]}


@pytest.mark.parametrize("net", sorted(NETS))
def test_fused_adam_equals_unfused_small_nets(M, net):
    """dhaug_adam_repack_step against counter_add + adam_step_dev + repack_weights, bit for bit over four steps: parameters,
    moments, step count, both packed copies with their pads -- and the copies against torch's casts of the updated weights"""
    shapes = NETS[net]

    def build():
        g = S.gen(31)
        return [torch.nn.Parameter(dev(torch.randn(*s, generator=g))) for s in shapes]
    a, b = opts = _fused_pair(M, build)
    g = S.gen(32)
    for step in range(1, 5):
        _fused_step(M, opts, [dev(torch.randn(*s, generator=g) * 0.1) for s in shapes])
        _fused_equal(a, b, step)
        assert len(a._packs[2]) == len(b._packs[2]) == sum(1 for s in shapes if len(s) == 2)
        for (pa, nta, nna), (pb, ntb, nnb) in zip(a._packs[2], b._packs[2]):
            N, K = pa.shape
            assert same_bits(nta, ntb) and same_bits(nna, nnb), (step, N, K)
            assert same_bits(nta, S.cast_pad_ref(pa.detach(), S.ceil_to(K, 16))), (step, N, K)
            assert same_bits(nna, S.cast_transpose_ref(pa.detach(), S.ceil_to(N, 16))), (step, N, K)


def test_fused_adam_wraps_its_grid(M):
    """one 1-D parameter of 8 192 x 4 096 + 4 097 elements: adam_nt_kernel's 8 192 workgroups take a second trip of two items, the
    last with ONE element, on the non-matrix branch.  Fused against unfused bit for bit; the unfused side against the fp64 rule on a
    strided sample of 2^20 elements that holds the last 5 000.  (About 1.1 GB on the device; prints its wall time.)"""
    t0 = time.time()
    n = S.MP_ADAM_NT
    items, per = S.items("adam_nt")
    assert items == per + 2 and n % S.ADAM_NT_ITEM == 1
    lr = 1e-4

    def build():
        return [torch.nn.Parameter(torch.randn(n, device="cuda", generator=dgen(41)))]
    a, b = opts = _fused_pair(M, build, lr)
    stride = (n - 5000) // (2 ** 20 - 5000)
    idx = torch.cat([torch.arange(0, n - 5000, stride, device="cuda")[:2 ** 20 - 5000], torch.arange(n - 5000, n, device="cuda")])
    assert idx.numel() == 2 ** 20 and int(idx[-1]) == n - 1
    p0 = b.flat_param[idx].clone()
    ref = {dt: (p0.to(dt), torch.zeros(idx.numel(), dtype=dt, device="cuda"), torch.zeros(idx.numel(), dtype=dt, device="cuda"))
           for dt in (F64, F32)}
    d = torch.randn(n, device="cuda", generator=dgen(42))
    for step, scale in zip(S.ADAM_STEPS, S.ADAM_GRAD_SCALES):
        for o in opts:
            o.step_dev.fill_(step - 1)
        grad = d * scale
        _fused_step(M, opts, [grad])
        _fused_equal(a, b, step)
        for dt in (F64, F32):
            ref[dt] = S.adam_ref(ref[dt][0], grad[idx], ref[dt][1], ref[dt][2], step, dt, lr=lr, gscale=1.0)
        del grad
    got = (b.flat_param[idx], b.exp_avg[idx], b.exp_avg_sq[idx])
    bounds = S.adam_check("FusedAdam (four launches), sample of 2^20", got, dict(p0=p0, ref64=ref[F64], ref32=ref[F32]), lr)
    torch.cuda.synchronize()
    print("test_fused_adam_wraps_its_grid: %d elements, bounds p %.3e m %.3e v %.3e, wall time %.2f s" % ((n,) + tuple(bounds) + (time.time() - t0,)))


# ================================================================================================================ D. bounds
def _stream_bounds_cases(M, R):
    """(name, inputs, outputs {name: (numel, dtype)}, inout {name: tensor}, call(i, o) -> rc, kept {out name: (rows, ld, width)}):
    every entry point of the table at R rows.  inout buffers (Adam's p, m, v) are guarded outputs filled before the call; `kept`
    names outputs whose columns [width, ld) belong to the caller."""
    L, s = M.L, stream
    g = S.gen(R)
    rn = lambda *shape: dev(torch.randn(*shape, generator=g))
    rb = lambda *shape: dev(torch.randn(*shape, generator=g).to(BF16))
    count = torch.full((1,), 2, dtype=torch.int32, device="cuda")
    ybits = M.fused.encode_bits(torch.randn(R, 256, generator=g) > 0).cuda()
    Ws, routs, rdesc = _repack_descs(M, [(R, 30), (3, R)], seed=R)
    cases = [
        ("cast_pad", dict(x=rn(R, 30)), dict(o=(R * 40, BF16)), {}, lambda i, o: L.dhaug_cast_pad_bf16(i["x"], 30, o["o"], 40, R, 30, 32, s()),
         dict(o=(R, 40, 32))),
        ("cast_transpose", dict(x=rn(R, 30)), dict(o=(30 * (R + 23), BF16)), {},
         lambda i, o: L.dhaug_cast_transpose_bf16(i["x"], 30, o["o"], R + 23, R, 30, R + 15, s()), dict(o=(30, R + 23, R + 15))),
        ("colsum_f32", dict(x=rn(R, 65)), dict(o=(65, F32)), {}, lambda i, o: L.dhaug_colsum_f32(i["x"], 65, o["o"], R, 65, 0, s()), {}),
        ("colsum_bf16", dict(x=rb(R, 65)), dict(o=(65, F32)), {}, lambda i, o: L.dhaug_colsum_bf16(i["x"], 65, o["o"], R, 65, 0, s()), {}),
        ("act_backward_bf16", dict(g=rb(R, 16), y=rb(R, 16)), dict(o=(R * 24, BF16)), {},
         lambda i, o: L.dhaug_act_backward_bf16(i["g"], 16, i["y"], 16, o["o"], 24, R, 16, 2, 0.01, s()), dict(o=(R, 24, 16))),
        ("act_backward_f32", dict(g=rn(R * 7), y=rn(R * 7)), dict(o=(R * 7, F32)), {},
         lambda i, o: L.dhaug_act_backward_f32(i["g"], i["y"], o["o"], R * 7, 2, 0.01, s()), {}),
        ("add_f32", dict(a=rn(R * 7), b=rn(R * 7)), dict(o=(R * 7, F32)), {}, lambda i, o: L.dhaug_add_f32(i["a"], i["b"], o["o"], R * 7, s()), {}),
        ("rank1_mask", dict(sd=rb(R, 1), w=rb(100, 1), y=rb(R, 112)), dict(o=(R * 120, BF16)), {},
         lambda i, o: L.dhaug_rank1_mask_bf16(i["sd"], 1, i["w"], 1, i["y"], 112, o["o"], 120, R, 100, 112, 1, 0.0, s()), dict(o=(R, 120, 112))),
        ("rank1_bits", dict(sd=rb(R, 1), w=rb(256, 1), bits=ybits), dict(o=(R * 264, BF16)), {},
         lambda i, o: L.dhaug_rank1_bits_bf16(i["sd"], 1, i["w"], 1, i["bits"], o["o"], 264, R, 2, 0.2, s()), dict(o=(R, 264, 256))),
        ("adam_step", dict(g=rn(R * 7)), {}, dict(p=rn(R * 7), m=rn(R * 7) * 0.1, v=rn(R * 7).abs()),
         lambda i, o: L.dhaug_adam_step(o["p"], i["g"], o["m"], o["v"], R * 7, 1e-4, 0.5, 0.9, 1e-8, 3, 1.0, s()), {}),
        ("adam_step_dev", dict(g=rn(R * 7), count=count), {}, dict(p=rn(R * 7), m=rn(R * 7) * 0.1, v=rn(R * 7).abs()),
         lambda i, o: L.dhaug_adam_step_dev(o["p"], i["g"], o["m"], o["v"], R * 7, 1e-4, 0.5, 0.9, 1e-8, i["count"], 1.0, s()), {}),
    ]
    for mode, terms in sorted(S.SPLIT_BF16_LAYOUT):
        w = len(S.SPLIT_BF16_LAYOUT[(mode, terms)]) * 40
        cases.append(("split_bf16 mode %d terms %d" % (mode, terms), dict(x=rn(R, 33)), dict(o=(R * w, BF16)), {},
                      lambda i, o, mode=mode, terms=terms: L.dhaug_split_bf16(i["x"], 33, o["o"], R, 33, 40, mode, terms, s()), {}))
    for mode in sorted(S.SPLIT_F16_LAYOUT):
        w = len(S.SPLIT_F16_LAYOUT[mode]) * 40
        cases.append(("split_f16 mode %d" % mode, dict(x=rn(R, 33)), dict(o=(R * w, F16)), {},
                      lambda i, o, mode=mode: L.dhaug_split_f16(i["x"], 33, o["o"], R, 33, 40, mode, s()), {}))
    return cases, (Ws, routs, rdesc)


@pytest.mark.parametrize("R", [1, 63, 65])
def test_stream_outputs_stay_in_bounds(M, R):
    cases, (Ws, routs, rdesc) = _stream_bounds_cases(M, R)
    for name, ins, outs, inout, call, kept in cases:
        keep = {k: v.clone() for k, v in ins.items()}
        bufs = {k: Guarded(n, dt) for k, (n, dt) in outs.items()}
        for k, t in inout.items():
            bufs[k] = Guarded(t.numel(), t.dtype)
            bufs[k].out.copy_(t)
        rc = call({k: ptr(v) for k, v in ins.items()}, {k: ptr(b.out) for k, b in bufs.items()})
        torch.cuda.synchronize()
        assert rc == 0, name
        for k, b in bufs.items():
            b.check((name, k, R), written=k not in kept)
            if k in kept:
                rows, ld, width = kept[k]
                view = b.out.view(rows, ld)
                assert (bits(view[:, :width]) != PAYLOAD16).all() and (bits(view[:, width:]) == PAYLOAD16).all(), (name, k, R)
            if k in inout:
                assert not same_bits(b.out, inout[k]), (name, k, R)                # (the step did arrive)
        assert all(same_bits(ins[k], keep[k]) for k in ins), name
    keep = [W.clone() for W in Ws]
    assert M.L.dhaug_repack_weights(ptr(rdesc), len(Ws), stream()) == 0
    for W, k, (nt, nn, Kp, Np) in zip(Ws, keep, routs):
        nt.check(("repack nt", R)); nn.check(("repack nn", R))
        assert same_bits(W, k)
