"""CPU checks behind tests/test_gpu_fk_tail.py: the plain-integer Philox4x32-10 of tests/fk_tail_util.py against the published
known-answer vectors, the host build of the kernel's Philox and jitter draw (csrc/dhaug_fk_math.h) against it, and the per-column rule
on the host build of the FK arithmetic -- the source the device runs."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

import fk_tail_util as U
import golden_util as GU

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def host():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    return ctypes.CDLL(ge.build_hostcheck(verbose=False))


def test_python_philox_known_answers():
    for counter, key, want in U.PHILOX_KAT:
        assert U.philox4x32_10(counter, key) == want, (counter, key)


def test_host_philox_matches_python(host):
    rng = np.random.default_rng(11)
    counters = np.concatenate([np.array([k[0] for k in U.PHILOX_KAT], np.uint32), rng.integers(0, 2 ** 32, (1000, 4), dtype=np.uint32)])
    keys = np.concatenate([np.array([k[1] for k in U.PHILOX_KAT], np.uint32), rng.integers(0, 2 ** 32, (1000, 2), dtype=np.uint32)])
    counters, keys = np.ascontiguousarray(counters), np.ascontiguousarray(keys)
    out = np.zeros_like(counters)
    host.hostcheck_philox4x32(counters.ctypes.data_as(ctypes.c_void_p), keys.ctypes.data_as(ctypes.c_void_p),
                              out.ctypes.data_as(ctypes.c_void_p), ctypes.c_long(len(counters)))
    for i, (_, _, want) in enumerate(U.PHILOX_KAT):
        assert tuple(int(v) for v in out[i]) == want
    for i in range(len(counters)):
        assert tuple(int(v) for v in out[i]) == U.philox4x32_10(counters[i], keys[i]), i


@pytest.mark.parametrize("seed,offset", [(0, 0), (1234, 16), (2 ** 64 - 1, 2 ** 32 - 1), (0x0123456789abcdef, 2 ** 40 + 8),
                                         (7, 2 ** 64 - 1)])
def test_host_jitter_layout_matches_reference(host, seed, offset):
    """the draw of a pose, both halves, as the kernel computes it (jitter_half): counter words, which half feeds which columns, the
    high words of seed and offset, and the carry of offset + 1 out of a low word of 0xffffffff"""
    rows = np.array([0, 1, 63, 64, 260, 2 ** 32 - 1, 2 ** 32, 2 ** 40 + 5], np.uint64)
    out = np.zeros((len(rows), 8), np.float32)
    host.hostcheck_jitter(rows.ctypes.data_as(ctypes.c_void_p), ctypes.c_uint64(seed), ctypes.c_uint64(offset),
                          out.ctypes.data_as(ctypes.c_void_p), ctypes.c_long(len(rows)))
    ref = U.jitter_reference(seed, offset, rows)
    assert np.array_equal(out.view(np.uint32), ref.view(np.uint32))
    if offset & U.M32 == U.M32:
        # half 1 carries into the high word: it is not half 0 of the offset whose low word is 0
        other = U.jitter_reference(seed, offset - U.M32, rows)
        assert not np.array_equal(ref[:, 4:], other[:, :4])
        assert np.array_equal(ref[:, 4:], U.jitter_reference(seed, (offset + 1) & U.M64, rows)[:, :4])


def _host_fk(host, a, bl, rt, g):
    N = a.shape[0]
    P = ctypes.POINTER(ctypes.c_float)
    ptr = lambda x: x.ctypes.data_as(P)
    an, bn, rn, gn = (np.ascontiguousarray(t.numpy(), np.float32) for t in (a, bl, rt, g))
    out = np.zeros((N, 48), np.float32)
    host.hostcheck_fk_forward(ptr(an), ptr(bn), ptr(rn), ptr(out), ctypes.c_long(N))
    ga, gb, gr = np.full((N, 37), 7.0, np.float32), np.full((N, 15), 7.0, np.float32), np.full((N, 3), 7.0, np.float32)
    host.hostcheck_fk_backward(ptr(an), ptr(bn), ptr(gn), ptr(ga), ptr(gb), ptr(gr), ctypes.c_long(N))
    return tuple(torch.from_numpy(x) for x in (out, ga, gb, gr))


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_host_fk_per_column(host, seed):
    """csrc/dhaug_fk_math.h on the host, N = 193, root 0 in the forward: every gradient column and every forward coordinate within
    4 max(s_c, 2^-23) of the fp64 oracle, the dead angle columns exactly 0.  (Over seeds 0..9 the worst e_c / max(s_c, 2^-23) was 1.91,
    against the limit of 4.)"""
    N = 193
    a, bl, rt = GU.synth_fk_inputs(N, seed)
    g = torch.randn(N, 48, generator=torch.Generator().manual_seed(1000 + seed))
    zero = torch.zeros_like(rt)
    out, ga, gb, gr = _host_fk(host, a, bl, zero, g)
    r64, r32 = U.fk_oracle(a, bl, zero, g, torch.float64), U.fk_oracle(a, bl, zero, g, torch.float32)
    assert U.dead_columns(r64[1]) == U.FK_DEAD_ANGLE_COLUMNS and U.dead_columns(r64[0]) == [0, 1, 2]
    for name, got, i in (("host_fk_forward", out, 0), ("host_grad_angles", ga, 1), ("host_grad_bone_len", gb, 2), ("host_grad_root", gr, 3)):
        U.check_columns("%s_seed%d" % (name, seed), got, r64[i], r32[i])


def test_check_columns_rejects_what_a_tensor_bound_lets_through():
    """the rule on emulated faults: one small gradient column scaled by 1.003 (0.3 % of a column that is 1/75 of the tensor's
    scale: inside 1e-4 x max|ref| of the whole tensor), a dropped term in one short chain, a non-zero in a dead column"""
    N = 193
    a, bl, rt = GU.synth_fk_inputs(N, 5)
    g = torch.randn(N, 48, generator=torch.Generator().manual_seed(6))
    r64, r32 = U.fk_oracle(a, bl, rt, g, torch.float64), U.fk_oracle(a, bl, rt, g, torch.float32)
    U.check_columns("oracle_fp32_grad_angles", r32[1], r64[1], r32[1])
    bad = r32[1].clone(); bad[:, 19] *= 1.003
    with pytest.raises(AssertionError):
        U.check_columns("scaled", bad, r64[1], r32[1])
    bad = r32[1].clone(); bad[5, 27] = 1e-30
    with pytest.raises(AssertionError):
        U.check_columns("dead", bad, r64[1], r32[1])
    head, bone, sc, gt = U.tail_inputs(N, 7)
    t64, t32 = U.tail_oracle(head, bone, sc, gt, True, torch.float64), U.tail_oracle(head, bone, sc, gt, True, torch.float32)
    assert U.dead_columns(t64[2]) == U.HEAD_DEAD_COLUMNS
    U.check_columns("oracle_fp32_grad_head", t32[2], t64[2], t32[2], U.TANH_ALLOWANCE)
    scale = t64[2].abs().max(0).values
    small = int(torch.where(scale > 0, scale, scale.max()).argmin())
    bad = t32[2].clone(); bad[:, small] *= 1.0075                                      # 0.75 % of the smallest column
    assert (bad - t64[2]).abs().max().item() <= 1e-4 * t64[2].abs().max().item()       # the bound per tensor does not see it
    with pytest.raises(AssertionError):
        U.check_columns("small column", bad, t64[2], t32[2], U.TANH_ALLOWANCE)
