"""CPU side of the unit-level harness of dhaug_mlp_forward (tests/mlp_unit_util.py): every program the GPU test runs is built
here and held to the condition that makes its bit-for-bit comparison legitimate -- for every GEMM unit, row and feature,
sum|terms| < 2^22 q with q the largest power of two dividing every term, every operand a bf16 value, every column a unit reads
written by an earlier unit -- and to non-degenerate outputs (every column varies over the rows, no two columns equal).  No
program is excluded: one that misses the condition fails here and its data get fixed.  Plus the host's refusals of the unit
forms the kernel has no route for, which need no GPU (the library validates a program before it launches anything)."""
import ctypes
import os
import sys

import numpy as np
import pytest

import mlp_unit_util as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL_EXACT = [n for f in U.TIER1 + ("cap", "ship") for n in U.names(f)]


@pytest.mark.parametrize("name", ALL_EXACT)
def test_program_is_exact_and_not_degenerate(name):
    p = U.get(name)
    r = p.ref()                                                               # asserts the exactness condition for every unit
    assert p.tier == 1 and 0 < r["bits"] < U.EXACT_BITS
    assert all(not b.any() for b in r["bound"].values())
    U.nondegenerate(p)
    for T in p.tensors.values():                                              # every output sits in a wider tensor
        if T["data"] is None and not name.startswith("ship_"):              # (the shipped builders allocate their own outputs)
            assert T["ld"] > T["width"]


@pytest.mark.parametrize("name", U.names("real"))
def test_realistic_programs_have_finite_positive_bounds(name):
    p = U.get(name)
    r = p.ref()
    assert p.tier == 2 and p.mmax == 129
    for t, b in r["bound"].items():
        b = b[:, :p.tensors[t]["ncheck"]]
        assert np.isfinite(b).all() and (b > 0).all() and np.isfinite(r["out"][t]).all()
        # a bound is worth something only if it is small beside the values it guards
        assert np.median(b) < 0.02 * np.abs(r["out"][t][:, :b.shape[1]]).mean()


def test_the_families_cover_what_they_claim():
    singles = [U.get(n) for n in U.names("single")]
    seen = {(p.units[-1]["K"] if p.units[-1]["kind"] == U.GEMM else p.units[-2]["K"],
             p.units[-1]["N"] if p.units[-1]["kind"] == U.GEMM else p.units[-2]["N"]) for p in singles}
    assert {(K, N) for K in U.K1 for N in U.N1} <= seen
    g = [next(u for u in p.units if u["kind"] == U.GEMM) for p in singles]
    for K in U.K1:                                                            # every K and every N meets every activation and residual form
        assert {(u["act"]) for u in g if u["K"] == K} == {0, 1, 2}
        assert {(u["res"] < 0, u["res"] == u["dst"]) for u in g if u["K"] == K} == {(True, False), (False, True), (False, False)}
    for N in U.N1:
        assert {(u["act"]) for u in g if u["N"] == N} == {0, 1, 2}
        assert len({(u["res"] < 0, u["res"] == u["dst"]) for u in g if u["N"] == N and not u["flags"]}) == 3
        if N <= 64:
            assert {bool(u["flags"] & U.F_OUT_F32) for u in g if u["N"] == N} == {True, False}
    assert any(u["src"] == 2 for u in g) and any(u["dst"] == 2 for u in g) and any(u["res"] == 2 for u in g)
    loads = [(u["kind"], p.tensors[u["t"]]["ld"] != u["cols"]) for p in singles for u in p.units if u["kind"] in (U.LOAD_F32, U.LOAD_BF16)]
    assert {(U.LOAD_F32, True), (U.LOAD_F32, False), (U.LOAD_BF16, True), (U.LOAD_BF16, False)} <= set(loads)
    shapes = set()
    for n in U.names("two"):
        u = next(u for u in U.get(n).units if u["kind"] == U.GEMM)
        c1, c2 = (u["ksteps"] + 3) // 4, (u["ksteps2"] + 3) // 4
        shapes.add((c1 + c2) * 16 + c1)
    assert shapes == {33, 66, 132}
    stacks = [U.get(n) for n in U.names("stack")]
    runs = {sum(1 for u in p.units if u["kind"] == U.GEMM and u["ksteps"] == 16 and u["N"] > 224 and not u["flags"]) for p in stacks}
    assert {2, 3, 6, 7} <= runs
    assert {225, 232} <= {u["N"] for p in stacks for u in p.units if u["kind"] == U.GEMM}
    assert {1, 35, 64} <= {u["N"] for p in stacks for u in p.units if u["kind"] == U.GEMM and u["flags"] & U.F_OUT_F32}
    assert {n.split("_")[0] for n in U.names("cap")} == {"single", "two", "narrow", "stack", "parking", "stale"}
    assert all(U.get(n).mmax == U.M_CAP and U.get(n).cap == 2 for n in U.names("cap"))


def test_numpy_packer_follows_the_header_formula():
    rng = np.random.default_rng(5)
    W = U.bf16_round(rng.integers(-64, 65, size=(37, 150)).astype(np.float64) / 8)
    for K, k0 in ((100, 0), (64, 50), (9, 141)):
        blob = U.pack_wfrag(W, K, k0)
        ksteps = 4 * ((K + 63) // 64)
        assert blob.shape == (8 * ksteps * 512,)
        val = (blob.astype(np.uint32) << 16).view(np.float32)
        for s, ks, lane, j in ((0, 0, 0, 0), (1, 2, 36, 5), (1, 3, 63, 7), (0, ksteps - 1, 31, 0), (7, 1, 3, 3), (1, 0, 4, 1), (1, 0, 5, 0)):
            n, k = 32 * s + (lane & 31), 16 * ks + 8 * (lane >> 5) + j
            want = W[n, k0 + k] if (n < 37 and k < K) else 0.0
            assert val[((s * ksteps + ks) * 64 + lane) * 8 + j] == want, (K, k0, s, ks, lane, j)
        assert np.count_nonzero(val) == np.count_nonzero(W[:, k0:k0 + K])


def test_exactness_check_refuses_what_fp32_cannot_hold():
    """the condition itself: 2^22 + 1 as a sum of 1s and one 2^22 misses it, half of that passes; a non-bf16 operand is refused"""
    x = np.array([[2.0 ** 22, 1.0]])
    with pytest.raises(AssertionError, match="below 2\\^22"):
        U._exactness("t", x, np.array([[1.0, 1.0]]), [])
    assert U._exactness("t", np.array([[2.0 ** 20, 1.0]]), np.array([[1.0, 1.0]]), []) < 22
    assert U._exactness("t", np.array([[2.0 ** 30, 2.0 ** 20]]), np.array([[1.0, 1.0]]), []) < 11      # q is 2^20, not 1
    with pytest.raises(AssertionError, match="below 2\\^22"):                                          # the bias lowers q
        U._exactness("t", np.array([[2.0 ** 30, 2.0 ** 20]]), np.array([[1.0, 1.0]]), [np.array([1.0])])
    with pytest.raises(AssertionError, match="no bf16 value"):
        U._exactness("t", np.array([[257.0]]), np.array([[1.0]]), [])
    assert U.bf16_round(np.array([257.0, 259.0, -1.00390625, 3.0]))[:3].tolist() == [256.0, 260.0, -1.0]   # ties to even
    assert U.lowbit(np.array([0.0, 1.0, 6.0, -0.75, 2.0 ** -20 * 3])).tolist() == [np.inf, 1.0, 2.0, 0.25, 2.0 ** -20]


@pytest.fixture(scope="module")
def lib():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    ge.build_lib(verbose=False)
    import dhaug_amd  # noqa: F401
    from dhaug_amd import _lib
    return _lib


def test_host_refuses_unit_forms_without_a_route(lib):
    """validated before any launch, so no GPU is needed: the pointers are host memory that nothing dereferences"""
    L = lib.lib()
    buf = (ctypes.c_float * 4096)()
    base = ctypes.addressof(buf)
    ptr = ctypes.c_void_p(base + (-base) % 16)
    EINVAL, EUNSUPPORTED = -1, -3

    def unit(kind, **kw):
        u = lib.MlpUnit()
        u.kind, u.src, u.dst, u.res, u.src2 = kind, -1, -1, -1, -1
        for k, v in kw.items():
            setattr(u, k, v)
        return u

    def run(*units):
        arr = (lib.MlpUnit * len(units))(*units)
        return L.dhaug_mlp_forward(arr, len(units), 128, None)

    load = unit(U.LOAD_F32, dst=1, cols=64, ld=64, g=ptr)
    gemm = lambda **kw: unit(U.GEMM, **dict(dict(src=1, dst=0, ksteps=4, n=256, w=ptr, bias=ptr), **kw))
    for ks in (9, 10, 11, 12):                                                # K in 129..192: three chunks, no such shape
        assert run(load, gemm(ksteps=ks)) == EUNSUPPORTED
    assert run(load, gemm(n=65, flags=U.F_OUT_F32, g=ptr, ld=72)) == EUNSUPPORTED
    assert run(load, gemm(dst=1)) == EINVAL                                   # dst == src
    for ks in (1, 2, 3, 5, 6, 7):                                             # a second source starts on a chunk boundary of the first
        assert run(load, gemm(dst=2, n=100, src2=0, ksteps2=4, w2=ptr, ksteps=ks)) == EUNSUPPORTED
    # 128 + 40 columns as ksteps2 = 3 would be two chunks plus one: no such shape (the harness hands over the 128 it loaded)
    assert run(load, gemm(dst=2, n=100, src2=0, ksteps=8, ksteps2=3, w2=ptr)) == EUNSUPPORTED
    # an fp32 output is written from the accumulators without the residual step: a residual there is refused, not dropped
    assert run(load, gemm(n=35, flags=U.F_OUT_F32, g=ptr, ld=40, res=2)) == EINVAL
