"""Shared by tests/test_fk_tail_cpu.py and tests/test_gpu_fk_tail.py: a plain-integer Philox4x32-10 and the generator tail's jitter
layout (include/dhaug.h, dhaug_gen_tail_forward_critics), the per-column error rule, and the oracle's gradients in fp64 and fp32.

The per-column rule is the rule of tests/test_gpu_attn_kernels.py applied to every column of a (rows, columns) result: with
scale_c = max over rows of |ref64[:, c]|, e_c = max |got - ref64| / scale_c and s_c the same figure for the oracle run in fp32,
    e_c <= 4 max(s_c, 2^-23) + allowance        for every column with scale_c > 0,
    got[:, c] == 0 exactly                      where scale_c == 0 (a column nothing can move).
A bound per tensor lets the small columns hide behind the large ones: the head gradient's root columns carry a factor 10 and are
~75 times the smallest column."""
import numpy as np
import torch

from oracle import dhaug_oracle as O

M32 = 0xFFFFFFFF
M64 = 0xFFFFFFFFFFFFFFFF
ONE_ROUNDING = 2.0 ** -23
# tanh_fast (csrc/dhaug_fk.hip) documents |error| <= 1.2e-7 absolute.  A head gradient g * scale * (1 - th^2) sees an error d of th
# as 2 |th| d <= 2 d in its last factor, and through the angle th * range / 2 (degrees) as a first-order change of g of the same
# relative size; four such terms, like the factor 4 of the rule.  Derived, not measured.
TANH_ALLOWANCE = 4 * 1.2e-7
FK_DEAD_ANGLE_COLUMNS = [4, 9, 22, 27, 32, 33]          # angle slots that move no joint (include/dhaug.h, dhaug_fk_backward)
HEAD_DEAD_COLUMNS = [23, 27, 31]                        # head columns feeding slots 27 and 32, and the unused column 31

# the three known-answer vectors of Random123 (kat_vectors, philox4x32 10): counter, key, result
PHILOX_KAT = [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((M32, M32, M32, M32), (M32, M32), (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


def philox4x32_10(counter, key):
    """Philox4x32-10 on Python integers: counter (c0, c1, c2, c3), key (k0, k1) -> (r0, r1, r2, r3)"""
    c0, c1, c2, c3 = (int(v) & M32 for v in counter)
    k0, k1 = (int(v) & M32 for v in key)
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & M32, (p0 >> 32) ^ c3 ^ k1, p0 & M32
        k0, k1 = (k0 + 0x9E3779B9) & M32, (k1 + 0xBB67AE85) & M32
    return c0, c1, c2, c3


def jitter_reference(seed, offset, rows):
    """the (len(rows), 8) fp32 jitter dhaug_gen_tail_forward_critics draws for the pose indices `rows`: half h in {0, 1} is one Philox
    call on the counter (lo, hi of the index; lo, hi of the 64-bit sum offset + h) under the key (lo, hi of the seed) and feeds columns
    4 h .. 4 h + 3; column 4 h + q = ((r[q] mod 400) - 200) / 1000, correctly rounded"""
    seed, offset = int(seed) & M64, int(offset) & M64
    out = np.empty((len(rows), 8), np.float32)
    for n, idx in enumerate(rows):
        idx = int(idx) & M64
        for h in (0, 1):
            ctr = (offset + h) & M64
            r = philox4x32_10((idx & M32, idx >> 32, ctr & M32, ctr >> 32), (seed & M32, seed >> 32))
            for q in range(4):
                out[n, 4 * h + q] = np.float32(int(r[q] % 400) - 200) / np.float32(1000)
    return out


def column_errors(got, ref64, stock32):
    """per column: (scale_c, e_c, s_c) as float64 tensors; e_c and s_c are 0 where scale_c is 0"""
    ref = ref64.detach().double().cpu().reshape(ref64.shape[0], -1)
    got = got.detach().double().cpu().reshape(ref.shape)
    stock = stock32.detach().double().cpu().reshape(ref.shape)
    scale = ref.abs().max(0).values
    div = torch.where(scale > 0, scale, torch.ones_like(scale))
    e = (got - ref).abs().max(0).values / div
    s = (stock - ref).abs().max(0).values / div
    live = scale > 0
    return scale, torch.where(live, e, torch.zeros_like(e)), torch.where(live, s, torch.zeros_like(s))


def check_columns(name, got, ref64, stock32, allowance=0.0):
    """the per-column rule of the module docstring; prints the worst column's figures before it asserts and returns the worst ratio
    e_c / (4 max(s_c, 2^-23) + allowance)"""
    assert got.dtype == torch.float32 and tuple(got.reshape(got.shape[0], -1).shape) == tuple(ref64.reshape(ref64.shape[0], -1).shape), name
    assert bool(torch.isfinite(got).all()), name
    scale, e, s = column_errors(got, ref64, stock32)
    bound = 4 * torch.maximum(s, torch.full_like(s, ONE_ROUNDING)) + allowance
    ratio = e / bound
    c = int(ratio.argmax())
    print("FIGURE %s worst column %d, ours %.4g, oracle_fp32 %.4g (scale %.4g, bound %.4g; %d columns, %d dead)"
          % (name, c, e[c].item(), s[c].item(), scale[c].item(), bound[c].item(), scale.numel(), int((scale == 0).sum())))
    g2 = got.detach().cpu().reshape(got.shape[0], -1)
    dead = [int(i) for i in torch.nonzero(scale == 0).flatten()]
    for i in dead:
        assert bool((g2[:, i] == 0).all()), "%s: column %d must be exactly 0" % (name, i)
    bad = [(int(i), e[i].item(), s[i].item(), int((got.detach().double().cpu().reshape(g2.shape)[:, i]
                                                  - ref64.detach().double().cpu().reshape(g2.shape)[:, i]).abs().argmax()))
           for i in torch.nonzero(ratio > 1).flatten()]
    assert not bad, "%s: (column, ours, oracle_fp32, worst row) beyond 4 max(s, 2^-23) + %.3g: %s" % (name, allowance, bad)
    return ratio.max().item()


def dead_columns(ref64):
    ref = ref64.detach().reshape(ref64.shape[0], -1)
    return [int(i) for i in torch.nonzero(ref.abs().max(0).values == 0).flatten()]


def fk_oracle(angles, bone_len, root, grad, dtype):
    """the CPU oracle's FK (16 joints) and its gradients through autograd in `dtype`: (out (N,48), grad_angles, grad_bone_len, grad_root)"""
    a, b, r = (t.detach().cpu().to(dtype).clone().requires_grad_(True) for t in (angles, bone_len, root))
    out = O.fk_forward16(a, b, r).reshape(-1, 48)
    (out * grad.detach().cpu().to(dtype).reshape(-1, 48)).sum().backward()
    return out.detach(), a.grad, b.grad, r.grad


def tail_oracle(head, bone_len, scaler, grad, use_preangle, dtype):
    """the oracle's generator tail and its head gradient in `dtype` (scaler None: no jitter): (fake (N,48), angles (N,37), grad_head)"""
    h = head.detach().cpu().to(dtype).clone().requires_grad_(True)
    sc = torch.zeros(h.shape[0], 8, dtype=dtype) if scaler is None else scaler.detach().cpu().to(dtype)
    fake, ang = O.gen_tail(h, bone_len.detach().cpu().to(dtype), sc, use_preangle=bool(use_preangle))
    (fake * grad.detach().cpu().to(dtype).reshape(-1, 48)).sum().backward()
    return fake.detach(), ang.detach(), h.grad


def tail_inputs(N, seed):
    """heads from randn with every seventh row times 4 (saturating tanh), bone lengths U(0.1, 0.5), jitter = integers in
    [-200, 200) / 1000, a cotangent from randn"""
    g = torch.Generator().manual_seed(seed)
    head = torch.randn(N, 35, generator=g)
    head[::7] *= 4.0
    bone_len = torch.rand(N, 15, generator=g) * 0.4 + 0.1
    scaler = torch.randint(-200, 200, (N, 8), generator=g).float() / 1000.0
    grad = torch.randn(N, 48, generator=g)
    return head, bone_len, scaler, grad
